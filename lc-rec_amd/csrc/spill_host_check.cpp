// Stand-alone check of the host code behind --spill, for a build with that code under AddressSanitizer + UBSan
// (`make spill_host_check && ./spill_host_check`): every argument refusal of lcrec_spill_nearest_free comes back with its code and
// a text that names the argument before anything touches a device, and lcrec_spill_nearest_free_workspace covers a flag per item.
// It runs on a build host without a device.  Not part of liblcrec_hip.so, never loaded into Python.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/lcrec.h"

static int failures = 0, checks = 0;

static void expect(int rc, int want_rc, const char *word)
{
    const char *text = lcrec_last_error();
    const bool ok = rc == want_rc && strstr(text, word) && strstr(text, "spill_nearest_free");
    printf("%s rc=%d \"%s\"\n", ok ? "ok  " : "FAIL", rc, text);
    ++checks;
    if (!ok) ++failures;
}

// the entry's twenty arguments, each with a value that passes every check (host memory: no call gets as far as a launch)
struct Args {
    int64_t *idx; int64_t n = 8, nf = 2; int L = 3; const int *K;
    const float *r2, *r1; int e = 16; const float *cb2, *cb1;
    const int64_t *tm, *to; int64_t nt = 1; const int64_t *sm, *so; int64_t ns = 1;
    int64_t *counters; void *ws; size_t wsb = 256;
    int call() const
    {
        return lcrec_spill_nearest_free(idx, n, nf, L, K, r2, r1, e, cb2, cb1, tm, to, nt, sm, so, ns, counters, ws, wsb, nullptr);
    }
};

int main()
{
    std::vector<double> store(64);
    char *p = reinterpret_cast<char *>(((uintptr_t)store.data() + 15) & ~(uintptr_t)15);
    int64_t *i64 = reinterpret_cast<int64_t *>(p), *i64_off4 = reinterpret_cast<int64_t *>(p + 4);
    float *f32 = reinterpret_cast<float *>(p), *f32_off4 = reinterpret_cast<float *>(p + 4), *f32_off8 = reinterpret_cast<float *>(p + 8);
    const int K3[3] = {48, 48, 48}, K1[1] = {48}, Kz2[3] = {48, 0, 48}, Kz1[3] = {48, 48, 0};
    const int Kfit[3] = {4, 256, 256}, Kbig[3] = {4, 512, 256}, Kwide[2] = {256, 2048};
    Args ok;
    ok.idx = i64; ok.K = K3; ok.r2 = ok.r1 = ok.cb2 = ok.cb1 = f32; ok.tm = ok.to = ok.sm = ok.so = i64; ok.counters = i64; ok.ws = p;
    Args a;
    char word[96];

    a = ok; a.L = 1; a.K = K1; expect(a.call(), LCREC_EINVAL, "L=1 (2 .. 16");
    a = ok; a.L = 0; expect(a.call(), LCREC_EINVAL, "L=0");
    a = ok; a.L = 17; expect(a.call(), LCREC_EINVAL, "L=17");
    a = ok; a.nf = -1; expect(a.call(), LCREC_EINVAL, "n_frozen=-1");
    a = ok; a.nf = 9; expect(a.call(), LCREC_EINVAL, "n_frozen=9 (0 .. n=8)");
    a = ok; a.n = -1; a.nf = 0; expect(a.call(), LCREC_EINVAL, "n=-1");
    a = ok; a.n = (int64_t)1 << 32; expect(a.call(), LCREC_EINVAL, "n=4294967296");
    a = ok; a.nt = -1; expect(a.call(), LCREC_EINVAL, "n_tuple_groups=-1");
    a = ok; a.nt = (int64_t)1 << 31; expect(a.call(), LCREC_EINVAL, "n_tuple_groups=2147483648");
    a = ok; a.ns = -1; expect(a.call(), LCREC_EINVAL, "n_super_buckets=-1");
    a = ok; a.ns = (int64_t)1 << 31; expect(a.call(), LCREC_EINVAL, "n_super_buckets=2147483648");
    const int es[] = {0, 8, 24, 128, -16};
    for (int e : es) {
        snprintf(word, sizeof word, "e_dim=%d", e);
        a = ok; a.e = e; expect(a.call(), LCREC_EUNSUPPORTED, word);
    }
    a = ok; a.K = Kz2; expect(a.call(), LCREC_EINVAL, "K[1]=0");
    a = ok; a.K = Kz1; expect(a.call(), LCREC_EINVAL, "K[2]=0");
    // 256 + 256 codes at e = 64 fit (144 896 B): the call goes on to its next check, here a NULL pointer
    a = ok; a.K = Kfit; a.e = 64; a.cb1 = nullptr; expect(a.call(), LCREC_EINVAL, "NULL pointer");
    a = ok; a.K = Kbig; a.e = 64;
    expect(a.call(), LCREC_EUNSUPPORTED, "levels 1 and 2 (K=512 and K=256, e=64) need 221696 B of LDS together: more than 160 KB");
    a = ok; a.L = 2; a.K = Kwide;
    expect(a.call(), LCREC_EUNSUPPORTED, "levels 0 and 1 (K=256 and K=2048, e=16) need 232960 B of LDS together");
    a = ok; a.r2 = f32_off8; expect(a.call(), LCREC_EINVAL, "16-byte aligned");
    a = ok; a.r1 = f32_off4; expect(a.call(), LCREC_EINVAL, "16-byte aligned");
    a = ok; a.cb2 = f32_off8; expect(a.call(), LCREC_EINVAL, "16-byte aligned");
    a = ok; a.cb1 = f32_off4; expect(a.call(), LCREC_EINVAL, "16-byte aligned");
    a = ok; a.idx = i64_off4; expect(a.call(), LCREC_EINVAL, "8-byte aligned");
    a = ok; a.tm = i64_off4; expect(a.call(), LCREC_EINVAL, "8-byte aligned");
    a = ok; a.to = i64_off4; expect(a.call(), LCREC_EINVAL, "8-byte aligned");
    a = ok; a.sm = i64_off4; expect(a.call(), LCREC_EINVAL, "8-byte aligned");
    a = ok; a.so = i64_off4; expect(a.call(), LCREC_EINVAL, "8-byte aligned");
    a = ok; a.counters = i64_off4; expect(a.call(), LCREC_EINVAL, "8-byte aligned");
    a = ok; a.counters = nullptr; expect(a.call(), LCREC_EINVAL, "counters_out is NULL");
    a = ok; a.K = nullptr; expect(a.call(), LCREC_EINVAL, "K is NULL");
    a = ok; a.idx = nullptr; expect(a.call(), LCREC_EINVAL, "NULL pointer");
    a = ok; a.r2 = nullptr; expect(a.call(), LCREC_EINVAL, "NULL pointer");
    a = ok; a.r1 = nullptr; expect(a.call(), LCREC_EINVAL, "NULL pointer");
    a = ok; a.cb2 = nullptr; expect(a.call(), LCREC_EINVAL, "NULL pointer");
    a = ok; a.cb1 = nullptr; expect(a.call(), LCREC_EINVAL, "NULL pointer");
    a = ok; a.tm = nullptr; expect(a.call(), LCREC_EINVAL, "NULL pointer");
    a = ok; a.to = nullptr; expect(a.call(), LCREC_EINVAL, "NULL pointer");
    a = ok; a.sm = nullptr; expect(a.call(), LCREC_EINVAL, "NULL pointer");
    a = ok; a.so = nullptr; expect(a.call(), LCREC_EINVAL, "NULL pointer");
    a = ok; a.ws = nullptr; expect(a.call(), LCREC_EWORKSPACE, "workspace of 0 bytes, 256 needed");
    a = ok; a.wsb = 255; expect(a.call(), LCREC_EWORKSPACE, "workspace of 255 bytes, 256 needed");
    a = ok; a.n = 300; expect(a.call(), LCREC_EWORKSPACE, "workspace of 256 bytes, 512 needed");

    const int64_t ns[] = {0, 1, 255, 256, 257, 1000000, 0xffffffffLL};
    for (int64_t n : ns) {
        const size_t w = lcrec_spill_nearest_free_workspace(n);
        const bool good = w >= (size_t)(n > 0 ? n : 1) && w % 256 == 0;
        ++checks;
        if (!good) { ++failures; printf("FAIL workspace(%lld) = %zu\n", (long long)n, w); }
    }
    printf("spill_host_check: %d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
