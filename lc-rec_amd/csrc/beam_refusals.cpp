// Stand-alone check of lcrec_rq_beam's host-side argument checks, for a build with the host code under AddressSanitizer +
// UBSan (`make beam_refusals`): every refusal must come back with its code and a text naming the argument, before anything
// touches a device -- so this runs on a build host without one.  Also the workspace query (0 for refused arguments) and the sizes
// behind it, and the largest level the entry admits: every level lcrec_rq_assign takes (rq_level_fits) and no other.  Not part of
// liblcrec_hip.so.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/lcrec.h"

namespace lcrec { bool rq_level_fits(int K, int e, int L); }   // rq_assign.hip (linked in with the library's objects)

static int failures = 0;

static void expect(int rc, int want_rc, const char *word)
{
    const char *text = lcrec_last_error();
    const bool ok = rc == want_rc && strstr(text, word) && strstr(text, "rq_beam");
    printf("%s rc=%d \"%s\"\n", ok ? "ok  " : "FAIL", rc, text);
    if (!ok) ++failures;
}

static void expect_size(size_t got, size_t want, const char *what)
{
    const bool ok = got == want;
    printf("%s %s = %zu (expected %zu)\n", ok ? "ok  " : "FAIL", what, got, want);
    if (!ok) ++failures;
}

static size_t up256(size_t v) { return (v + 255) / 256 * 256; }

int main()
{
    std::vector<double> store(64);
    char *p = reinterpret_cast<char *>(((uintptr_t)store.data() + 15) & ~(uintptr_t)15);
    float *f = reinterpret_cast<float *>(p), *f_off2 = reinterpret_cast<float *>(p + 2), *f_off8 = reinterpret_cast<float *>(p + 8);
    int64_t *q = reinterpret_cast<int64_t *>(p), *q_off4 = reinterpret_cast<int64_t *>(p + 4);
    void *ws = p, *ws_off8 = p + 8;
    const size_t big = (size_t)1 << 40;   // (a size only: nothing is read or written before the refusal)
    const int K3[3] = {48, 100, 7}, K0[3] = {48, 0, 7}, Kneg[3] = {48, 100, -5}, K1[1] = {300}, K2[2] = {48, 7};
    char word[96];

    // ---- every refusal, each before a device is touched
    expect(lcrec_rq_beam(f, 8, 16, f, nullptr, 3, 4, q, f, f, f, ws, big, nullptr), LCREC_EINVAL, "K is NULL");
    expect(lcrec_rq_beam(f, 8, 16, f, K3, 0, 4, q, f, f, f, ws, big, nullptr), LCREC_EINVAL, "L=0");
    expect(lcrec_rq_beam(f, 8, 16, f, K3, LCREC_MAX_LEVELS + 1, 4, q, f, f, f, ws, big, nullptr), LCREC_EINVAL, "L=17");
    expect(lcrec_rq_beam(f, -1, 16, f, K3, 3, 4, q, f, f, f, ws, big, nullptr), LCREC_EINVAL, "n=-1");
    for (int e : {0, 8, 24, 128, -16}) {
        snprintf(word, sizeof word, "e_dim=%d", e);
        expect(lcrec_rq_beam(f, 8, e, f, K3, 3, 4, q, f, f, f, ws, big, nullptr), LCREC_EINVAL, word);
    }
    for (int w : {0, 3, 5, 6, 7, 16, -2}) {
        snprintf(word, sizeof word, "width=%d", w);
        expect(lcrec_rq_beam(f, 8, 16, f, K3, 3, w, q, f, f, f, ws, big, nullptr), LCREC_EINVAL, word);
    }
    expect(lcrec_rq_beam(f, 8, 16, f, K0, 3, 4, q, f, f, f, ws, big, nullptr), LCREC_EINVAL, "K[1]=0");
    expect(lcrec_rq_beam(f, 8, 16, f, Kneg, 3, 4, q, f, f, f, ws, big, nullptr), LCREC_EINVAL, "K[2]=-5");
    expect(lcrec_rq_beam(nullptr, 8, 16, f, K3, 3, 4, q, f, f, f, ws, big, nullptr), LCREC_EINVAL, "z is NULL");
    expect(lcrec_rq_beam(f, 8, 16, nullptr, K3, 3, 4, q, f, f, f, ws, big, nullptr), LCREC_EINVAL, "codebooks is NULL");
    expect(lcrec_rq_beam(f, 8, 16, f, K3, 3, 4, nullptr, f, f, f, ws, big, nullptr), LCREC_EINVAL, "tuples_out is NULL");
    expect(lcrec_rq_beam(f, 8, 16, f, K3, 3, 4, q, nullptr, f, f, ws, big, nullptr), LCREC_EINVAL, "score_out is NULL");
    expect(lcrec_rq_beam(f, 8, 16, f, K3, 3, 4, q, f, nullptr, f, ws, big, nullptr), LCREC_EINVAL, "err_out is NULL");
    expect(lcrec_rq_beam(f_off8, 8, 16, f, K3, 3, 4, q, f, f, f, ws, big, nullptr), LCREC_EINVAL, "16-byte aligned");
    expect(lcrec_rq_beam(f, 8, 16, f_off8, K3, 3, 4, q, f, f, f, ws, big, nullptr), LCREC_EINVAL, "16-byte aligned");
    expect(lcrec_rq_beam(f, 8, 16, f, K3, 3, 4, q, f, f, f_off8, ws, big, nullptr), LCREC_EINVAL, "16-byte aligned");
    expect(lcrec_rq_beam(f, 8, 16, f, K3, 3, 4, q, f, f, f, ws_off8, big, nullptr), LCREC_EINVAL, "16-byte aligned");
    expect(lcrec_rq_beam(f, 8, 16, f, K3, 3, 4, q_off4, f, f, f, ws, big, nullptr), LCREC_EINVAL, "tuples_out must be 8-byte aligned");
    expect(lcrec_rq_beam(f, 8, 16, f, K3, 3, 4, q, f_off2, f, f, ws, big, nullptr), LCREC_EINVAL, "score_out and err_out must be 4-byte aligned");
    expect(lcrec_rq_beam(f, 8, 16, f, K3, 3, 4, q, f, f_off2, f, ws, big, nullptr), LCREC_EINVAL, "score_out and err_out must be 4-byte aligned");

    // ---- the workspace: residual halves [n][W][e] (none / one / two for L = 1 / 2 / more) and (L - 1) n W links
    expect_size(lcrec_rq_beam_workspace(8, 16, K3, 3, 4), 2 * up256(8 * 4 * 16 * 4) + up256(2 * 8 * 4 * 4), "workspace(n=8, e=16, L=3, W=4)");
    expect_size(lcrec_rq_beam_workspace(8, 16, K3, 3, 4), 4352, "workspace(n=8, e=16, L=3, W=4) in bytes");
    expect_size(lcrec_rq_beam_workspace(1000, 64, K3, 3, 8), 2 * 2048000 + 64000, "workspace(n=1000, e=64, L=3, W=8)");
    expect_size(lcrec_rq_beam_workspace(1000, 32, K2, 2, 2), 256000 + 8192, "workspace(n=1000, e=32, L=2, W=2): one half");
    expect_size(lcrec_rq_beam_workspace(7, 16, K3, 3, 1), 2 * 512 + 256, "workspace(n=7, e=16, L=3, W=1): rounded up");
    expect_size(lcrec_rq_beam_workspace(1000, 64, K1, 1, 8), 0, "workspace(L=1)");
    expect_size(lcrec_rq_beam_workspace(0, 32, K3, 3, 4), 0, "workspace(n=0)");
    expect_size(lcrec_rq_beam_workspace((int64_t)1 << 20, 32, K3, 3, 8), 2 * ((size_t)1 << 30) + ((size_t)1 << 26), "workspace(n=2^20, e=32, L=3, W=8)");
    expect_size(lcrec_rq_beam_workspace(8, 24, K3, 3, 4), 0, "workspace(e=24: refused)");
    expect_size(lcrec_rq_beam_workspace(8, 16, nullptr, 3, 4), 0, "workspace(K NULL: refused)");
    expect_size(lcrec_rq_beam_workspace(8, 16, K3, 0, 4), 0, "workspace(L=0: refused)");
    expect_size(lcrec_rq_beam_workspace(8, 16, K3, 3, 3), 0, "workspace(width=3: refused)");
    expect_size(lcrec_rq_beam_workspace(-1, 16, K3, 3, 4), 0, "workspace(n=-1: refused)");
    expect_size(lcrec_rq_beam_workspace(8, 16, K0, 3, 4), 0, "workspace(K[1]=0: refused)");
    expect(lcrec_rq_beam(f, 8, 16, f, K3, 3, 4, q, f, f, f, ws, 4351, nullptr), LCREC_EWORKSPACE, "workspace of 4351 bytes, 4352 needed");
    expect(lcrec_rq_beam(f, 8, 16, f, K3, 3, 4, q, f, f, f, nullptr, big, nullptr), LCREC_EWORKSPACE, "workspace of 0 bytes, 4352 needed");
    {   // one level needs no workspace, and resid_out is optional: past every check with n = 0, no launch
        const int rc = lcrec_rq_beam(f, 0, 16, f, K1, 1, 8, q, f, f, nullptr, nullptr, 0, nullptr);
        printf("%s L=1, n=0, no workspace, no resid_out: rc=%d\n", rc == LCREC_OK ? "ok  " : "FAIL", rc);
        if (rc != LCREC_OK) ++failures;
    }

    // ---- the largest level lcrec_rq_assign takes is past the argument checks (n = 0: no launch), the next one is refused
    for (int e : {16, 32, 64}) {
        const int L = 4;
        int top = 1;
        while (lcrec::rq_level_fits(top + 1, e, L)) ++top;
        const int fits[4] = {256, 256, 256, top}, over[4] = {256, 256, top + 1, 256};
        const int rc = lcrec_rq_beam(f, 0, e, f, fits, L, 8, q, f, f, f, ws, big, nullptr);
        printf("%s e=%d: K=%d admitted, rc=%d\n", rc == LCREC_OK ? "ok  " : "FAIL", e, top, rc);
        if (rc != LCREC_OK) ++failures;
        snprintf(word, sizeof word, "level 2 (K=%d, e=%d) does not fit", top + 1, e);
        expect(lcrec_rq_beam(f, 0, e, f, over, L, 8, q, f, f, f, ws, big, nullptr), LCREC_EUNSUPPORTED, word);
        expect_size(lcrec_rq_beam_workspace(8, e, over, L, 8), 0, "workspace(a level that does not fit: refused)");
        if (top >= (1 << 20)) { printf("FAIL e=%d: K=%d does not fit the 20 code bits of a link\n", e, top); ++failures; }
    }
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
