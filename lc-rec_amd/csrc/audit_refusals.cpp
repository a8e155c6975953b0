// Stand-alone check of lcrec_rq_audit's host-side argument checks, for a build with the host code under AddressSanitizer +
// UBSan (`make audit_refusals`): every refusal must come back with its code and a text naming the argument, before anything
// touches a device -- so this runs on a build host without one.  Also the workspace query, and the largest level the entry admits:
// every level lcrec_rq_assign takes (rq_level_fits) and no other.  Not part of liblcrec_hip.so.
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
    const bool ok = rc == want_rc && strstr(text, word) && strstr(text, "rq_audit");
    printf("%s rc=%d \"%s\"\n", ok ? "ok  " : "FAIL", rc, text);
    if (!ok) ++failures;
}

static void expect_size(size_t got, size_t want, const char *what)
{
    const bool ok = got == want;
    printf("%s %s = %zu (expected %zu)\n", ok ? "ok  " : "FAIL", what, got, want);
    if (!ok) ++failures;
}

int main()
{
    std::vector<double> store(64);
    char *p = reinterpret_cast<char *>(((uintptr_t)store.data() + 15) & ~(uintptr_t)15);
    float *f = reinterpret_cast<float *>(p), *f_off4 = reinterpret_cast<float *>(p + 4), *f_off8 = reinterpret_cast<float *>(p + 8);
    int64_t *q = reinterpret_cast<int64_t *>(p), *q_off4 = reinterpret_cast<int64_t *>(p + 4);
    int *r = reinterpret_cast<int *>(p), *r_off2 = reinterpret_cast<int *>(p + 2);
    uint32_t *u = reinterpret_cast<uint32_t *>(p), *u_off2 = reinterpret_cast<uint32_t *>(p + 2);
    void *ws = p, *ws_off8 = p + 8;
    const size_t big = (size_t)1 << 40;   // (a size only: nothing is read or written before the refusal)
    const int K3[3] = {48, 100, 7}, K0[3] = {48, 0, 7}, Kneg[3] = {48, 100, -5}, K1[1] = {300};
    char word[96];

    // ---- every refusal, each before a device is touched
    expect(lcrec_rq_audit(f, 8, 16, f, nullptr, 3, q, 0, f, f, r, q, f, f, u, ws, big, nullptr), LCREC_EINVAL, "K is NULL");
    expect(lcrec_rq_audit(f, 8, 16, f, K3, 0, q, 0, f, f, r, q, f, f, u, ws, big, nullptr), LCREC_EINVAL, "L=0");
    expect(lcrec_rq_audit(f, 8, 16, f, K3, LCREC_MAX_LEVELS + 1, q, 0, f, f, r, q, f, f, u, ws, big, nullptr), LCREC_EINVAL, "L=17");
    expect(lcrec_rq_audit(f, -1, 16, f, K3, 3, q, 0, f, f, r, q, f, f, u, ws, big, nullptr), LCREC_EINVAL, "n=-1");
    for (int e : {0, 8, 24, 128, -16}) {
        snprintf(word, sizeof word, "e_dim=%d", e);
        expect(lcrec_rq_audit(f, 8, e, f, K3, 3, q, 0, f, f, r, q, f, f, u, ws, big, nullptr), LCREC_EINVAL, word);
    }
    expect(lcrec_rq_audit(f, 8, 16, f, K0, 3, q, 0, f, f, r, q, f, f, u, ws, big, nullptr), LCREC_EINVAL, "K[1]=0");
    expect(lcrec_rq_audit(f, 8, 16, f, Kneg, 3, q, 0, f, f, r, q, f, f, u, ws, big, nullptr), LCREC_EINVAL, "K[2]=-5");
    expect(lcrec_rq_audit(f, 8, 16, f, K3, 3, q, 2, f, f, r, q, f, f, u, ws, big, nullptr), LCREC_EINVAL, "idx_stride=2 < L=3");
    expect(lcrec_rq_audit(f, 8, 16, f, K3, 3, q, -1, f, f, r, q, f, f, u, ws, big, nullptr), LCREC_EINVAL, "idx_stride=-1");
    expect(lcrec_rq_audit(nullptr, 8, 16, f, K3, 3, q, 0, f, f, r, q, f, f, u, ws, big, nullptr), LCREC_EINVAL, "z is NULL");
    expect(lcrec_rq_audit(f, 8, 16, nullptr, K3, 3, q, 0, f, f, r, q, f, f, u, ws, big, nullptr), LCREC_EINVAL, "codebooks is NULL");
    expect(lcrec_rq_audit(f, 8, 16, f, K3, 3, nullptr, 0, f, f, r, q, f, f, u, ws, big, nullptr), LCREC_EINVAL, "idx is NULL");
    expect(lcrec_rq_audit(f, 8, 16, f, K3, 3, q, 0, nullptr, f, r, q, f, f, u, ws, big, nullptr), LCREC_EINVAL, "d_held_out is NULL");
    expect(lcrec_rq_audit(f, 8, 16, f, K3, 3, q, 0, f, nullptr, r, q, f, f, u, ws, big, nullptr), LCREC_EINVAL, "d_best_out is NULL");
    expect(lcrec_rq_audit(f, 8, 16, f, K3, 3, q, 0, f, f, nullptr, q, f, f, u, ws, big, nullptr), LCREC_EINVAL, "rank_out is NULL");
    expect(lcrec_rq_audit(f, 8, 16, f, K3, 3, q, 0, f, f, r, q, nullptr, f, u, ws, big, nullptr), LCREC_EINVAL, "err_out is NULL");
    expect(lcrec_rq_audit(f, 8, 16, f, K3, 3, q, 0, f, f, r, q, f, f, nullptr, ws, big, nullptr), LCREC_EINVAL, "flags_out is NULL");
    expect(lcrec_rq_audit(f_off8, 8, 16, f, K3, 3, q, 0, f, f, r, q, f, f, u, ws, big, nullptr), LCREC_EINVAL, "16-byte aligned");
    expect(lcrec_rq_audit(f, 8, 16, f_off4, K3, 3, q, 0, f, f, r, q, f, f, u, ws, big, nullptr), LCREC_EINVAL, "16-byte aligned");
    expect(lcrec_rq_audit(f, 8, 16, f, K3, 3, q, 0, f_off8, f, r, q, f, f, u, ws, big, nullptr), LCREC_EINVAL, "16-byte aligned");
    expect(lcrec_rq_audit(f, 8, 16, f, K3, 3, q, 0, f, f_off4, r, q, f, f, u, ws, big, nullptr), LCREC_EINVAL, "16-byte aligned");
    expect(lcrec_rq_audit(f, 8, 16, f, K3, 3, q, 0, f, f, r, q, f_off8, f, u, ws, big, nullptr), LCREC_EINVAL, "16-byte aligned");
    expect(lcrec_rq_audit(f, 8, 16, f, K3, 3, q, 0, f, f, r, q, f, f_off4, u, ws, big, nullptr), LCREC_EINVAL, "16-byte aligned");
    expect(lcrec_rq_audit(f, 8, 16, f, K3, 3, q, 0, f, f, r, q, f, f, u, ws_off8, big, nullptr), LCREC_EINVAL, "16-byte aligned");
    expect(lcrec_rq_audit(f, 8, 16, f, K3, 3, q_off4, 0, f, f, r, q, f, f, u, ws, big, nullptr), LCREC_EINVAL, "idx and best_out must be 8-byte aligned");
    expect(lcrec_rq_audit(f, 8, 16, f, K3, 3, q, 0, f, f, r, q_off4, f, f, u, ws, big, nullptr), LCREC_EINVAL, "idx and best_out must be 8-byte aligned");
    expect(lcrec_rq_audit(f, 8, 16, f, K3, 3, q, 0, f, f, r_off2, q, f, f, u, ws, big, nullptr), LCREC_EINVAL, "rank_out and flags_out must be 4-byte aligned");
    expect(lcrec_rq_audit(f, 8, 16, f, K3, 3, q, 0, f, f, r, q, f, f, u_off2, ws, big, nullptr), LCREC_EINVAL, "rank_out and flags_out must be 4-byte aligned");

    // ---- the workspace: the residual between the levels, none for one level; too small or missing is LCREC_EWORKSPACE
    expect_size(lcrec_rq_audit_workspace(8, 16, K3, 3), 512, "workspace(n=8, e=16, L=3)");
    expect_size(lcrec_rq_audit_workspace(1000, 64, K3, 3), 256000, "workspace(n=1000, e=64, L=3)");
    expect_size(lcrec_rq_audit_workspace(1000, 64, K1, 1), 0, "workspace(L=1)");
    expect_size(lcrec_rq_audit_workspace(0, 32, K3, 3), 0, "workspace(n=0)");
    expect_size(lcrec_rq_audit_workspace(8, 24, K3, 3), 0, "workspace(e=24: refused)");
    expect_size(lcrec_rq_audit_workspace(8, 16, nullptr, 3), 0, "workspace(K NULL: refused)");
    expect_size(lcrec_rq_audit_workspace(8, 16, K3, 0), 0, "workspace(L=0: refused)");
    expect(lcrec_rq_audit(f, 8, 16, f, K3, 3, q, 0, f, f, r, q, f, f, u, ws, 511, nullptr), LCREC_EWORKSPACE, "workspace of 511 bytes, 512 needed");
    expect(lcrec_rq_audit(f, 8, 16, f, K3, 3, q, 0, f, f, r, q, f, f, u, nullptr, big, nullptr), LCREC_EWORKSPACE, "workspace of 0 bytes, 512 needed");

    // ---- the largest level lcrec_rq_assign takes is past the argument checks (n = 0: no launch), the next one is refused
    for (int e : {16, 32, 64}) {
        const int L = 4;
        int top = 1;
        while (lcrec::rq_level_fits(top + 1, e, L)) ++top;
        const int fits[4] = {256, 256, 256, top}, over[4] = {256, 256, top + 1, 256};
        const int rc = lcrec_rq_audit(f, 0, e, f, fits, L, q, 0, f, f, r, q, f, f, u, ws, big, nullptr);
        printf("%s e=%d: K=%d admitted, rc=%d\n", rc == LCREC_OK ? "ok  " : "FAIL", e, top, rc);
        if (rc != LCREC_OK) ++failures;
        snprintf(word, sizeof word, "level 2 (K=%d, e=%d) does not fit", top + 1, e);
        expect(lcrec_rq_audit(f, 0, e, f, over, L, q, 0, f, f, r, q, f, f, u, ws, big, nullptr), LCREC_EUNSUPPORTED, word);
        if (e == 64 && top != 576) { printf("FAIL e=64, L=4: the largest admitted level is K=%d, the documents say 576\n", top); ++failures; }
    }
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
