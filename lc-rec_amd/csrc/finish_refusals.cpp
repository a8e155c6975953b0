// Stand-alone check of lcrec_finish_nearest_free's host-side argument checks, for a build with the host code under
// AddressSanitizer + UBSan (`make finish_refusals`): every refusal must come back with its code and a text naming the dimension,
// before anything touches a device -- so this runs on a build host without one.  Not part of liblcrec_hip.so.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/lcrec.h"

static int failures = 0;

static void expect(int rc, int want_rc, const char *word)
{
    const char *text = lcrec_last_error();
    const bool ok = rc == want_rc && strstr(text, word) && strstr(text, "finish_nearest_free");
    printf("%s rc=%d \"%s\"\n", ok ? "ok  " : "FAIL", rc, text);
    if (!ok) ++failures;
}

int main()
{
    std::vector<double> store(64);
    char *p = reinterpret_cast<char *>(((uintptr_t)store.data() + 15) & ~(uintptr_t)15);
    int64_t *i64 = reinterpret_cast<int64_t *>(p);
    float *f32 = reinterpret_cast<float *>(p);
    int64_t *i64_off4 = reinterpret_cast<int64_t *>(p + 4);
    float *f32_off4 = reinterpret_cast<float *>(p + 4), *f32_off8 = reinterpret_cast<float *>(p + 8);
    const int K3[3] = {48, 48, 48}, K0[3] = {48, 48, 0}, Kbig[3] = {48, 48, 4096}, K1[1] = {2048};
    const int es[] = {0, 8, 24, 128, -16};
    char word[64];
    for (int e : es) {
        snprintf(word, sizeof word, "e_dim=%d", e);
        expect(lcrec_finish_nearest_free(i64, 8, 3, K3, f32, e, f32, i64, i64, 1, i64, nullptr), LCREC_EUNSUPPORTED, word);
    }
    expect(lcrec_finish_nearest_free(i64, 8, 3, K0, f32, 16, f32, i64, i64, 1, i64, nullptr), LCREC_EINVAL, "K[2]=0");
    expect(lcrec_finish_nearest_free(i64, 8, 3, Kbig, f32, 64, f32, i64, i64, 1, i64, nullptr), LCREC_EUNSUPPORTED,
           "level 2 (K=4096, e=64) does not fit");
    expect(lcrec_finish_nearest_free(i64, 8, 1, K1, f32, 16, f32, i64, i64, 1, i64, nullptr), LCREC_EUNSUPPORTED,
           "level 0 (K=2048, e=16) does not fit");
    expect(lcrec_finish_nearest_free(i64, 8, 0, K3, f32, 16, f32, i64, i64, 1, i64, nullptr), LCREC_EINVAL, "L=0");
    expect(lcrec_finish_nearest_free(i64, 8, 17, K3, f32, 16, f32, i64, i64, 1, i64, nullptr), LCREC_EINVAL, "L=17");
    expect(lcrec_finish_nearest_free(i64, -1, 3, K3, f32, 16, f32, i64, i64, 1, i64, nullptr), LCREC_EINVAL, "n=-1");
    expect(lcrec_finish_nearest_free(i64, (int64_t)1 << 32, 3, K3, f32, 16, f32, i64, i64, 1, i64, nullptr), LCREC_EINVAL, "n=4294967296");
    expect(lcrec_finish_nearest_free(i64, 8, 3, K3, f32, 16, f32, i64, i64, -1, i64, nullptr), LCREC_EINVAL, "n_buckets=-1");
    expect(lcrec_finish_nearest_free(i64, 8, 3, K3, f32, 16, f32, i64, i64, (int64_t)1 << 31, i64, nullptr), LCREC_EINVAL,
           "n_buckets=2147483648");
    expect(lcrec_finish_nearest_free(i64, 8, 3, K3, f32_off8, 16, f32, i64, i64, 1, i64, nullptr), LCREC_EINVAL, "16-byte aligned");
    expect(lcrec_finish_nearest_free(i64, 8, 3, K3, f32, 16, f32_off4, i64, i64, 1, i64, nullptr), LCREC_EINVAL, "16-byte aligned");
    expect(lcrec_finish_nearest_free(i64_off4, 8, 3, K3, f32, 16, f32, i64, i64, 1, i64, nullptr), LCREC_EINVAL, "8-byte aligned");
    expect(lcrec_finish_nearest_free(i64, 8, 3, K3, f32, 16, f32, i64_off4, i64, 1, i64, nullptr), LCREC_EINVAL, "8-byte aligned");
    expect(lcrec_finish_nearest_free(i64, 8, 3, K3, f32, 16, f32, i64, i64_off4, 1, i64, nullptr), LCREC_EINVAL, "8-byte aligned");
    expect(lcrec_finish_nearest_free(i64, 8, 3, K3, f32, 16, f32, i64, i64, 1, i64_off4, nullptr), LCREC_EINVAL, "8-byte aligned");
    expect(lcrec_finish_nearest_free(i64, 8, 3, K3, f32, 16, f32, i64, i64, 1, nullptr, nullptr), LCREC_EINVAL, "counters_out is NULL");
    expect(lcrec_finish_nearest_free(i64, 8, 3, nullptr, f32, 16, f32, i64, i64, 1, i64, nullptr), LCREC_EINVAL, "K is NULL");
    expect(lcrec_finish_nearest_free(nullptr, 8, 3, K3, f32, 16, f32, i64, i64, 1, i64, nullptr), LCREC_EINVAL, "NULL pointer");
    expect(lcrec_finish_nearest_free(i64, 8, 3, K3, f32, 16, f32, nullptr, i64, 1, i64, nullptr), LCREC_EINVAL, "NULL pointer");
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
