// Stand-alone check of lcrec_extend_finish_beam's host-side argument checks, for a build with the host code under AddressSanitizer
// + UBSan (`make extend_finish_beam_refusals`): every refusal must come back with its code and a text naming the argument and the
// entry, before anything touches a device -- so this runs on a build host without one.  n_frozen outside 0 .. n is refused too, and
// n_frozen == n asks for no array but the counters.  Also the workspace query: 0 for refused arguments, and lcrec_finish_beam_workspace's
// bytes for all others.  Not part of liblcrec_hip.so.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/lcrec.h"

static int failures = 0;

static void expect(int rc, int want_rc, const char *word)
{
    const char *text = lcrec_last_error();
    const bool ok = rc == want_rc && strstr(text, word) && strstr(text, "extend_finish_beam");
    printf("%s rc=%d \"%s\"\n", ok ? "ok  " : "FAIL", rc, text);
    if (!ok) ++failures;
}

static void expect_true(bool ok, const char *what, size_t got)
{
    printf("%s %s (%zu)\n", ok ? "ok  " : "FAIL", what, got);
    if (!ok) ++failures;
}

static size_t up256(size_t v) { return (v + 255) / 256 * 256; }

struct Args {
    int64_t *idx; int64_t n, nf; int L; const int *K; const int64_t *mem, *off; int64_t G, M; const float *eh; const int64_t *cand;
    const float *ce; int W; int *choice; int64_t *cnt; void *ws; size_t wsb;
};

static int run(const Args &a)
{
    return lcrec_extend_finish_beam(a.idx, a.n, a.nf, a.L, a.K, a.mem, a.off, a.G, a.M, a.eh, a.cand, a.ce, a.W, a.choice, a.cnt, a.ws, a.wsb, nullptr);
}

int main()
{
    std::vector<double> store(64);
    char *p = reinterpret_cast<char *>(((uintptr_t)store.data() + 15) & ~(uintptr_t)15);
    float *f = reinterpret_cast<float *>(p), *f_off2 = reinterpret_cast<float *>(p + 2);
    int64_t *q = reinterpret_cast<int64_t *>(p), *q_off4 = reinterpret_cast<int64_t *>(p + 4);
    int *c = reinterpret_cast<int *>(p), *c_off2 = reinterpret_cast<int *>(p + 2);
    const size_t big = (size_t)1 << 40;   // (a size only: nothing is read or written before the refusal)
    const int K3[3] = {48, 100, 7}, K0[3] = {48, 0, 7}, Kneg[3] = {48, 100, -5};
    int Kwide[13], K128[16];
    for (int &k : Kwide) k = 1 << 10;      // 130 bits
    for (int &k : K128) k = 1 << 8;        // 128 bits: admitted
    const Args good = {q, 8, 3, 3, K3, q, q, 2, 4, f, q, f, 4, c, q, p, big};
    char word[96];

    // ---- every refusal, each before a device is touched
    for (int W : {0, 3, 6, 16, -1}) {
        Args a = good; a.W = W;
        snprintf(word, sizeof word, "width=%d", W);
        expect(run(a), LCREC_EINVAL, word);
    }
    { Args a = good; a.L = 0; expect(run(a), LCREC_EINVAL, "L=0"); }
    { Args a = good; a.L = LCREC_MAX_LEVELS + 1; expect(run(a), LCREC_EINVAL, "L=17"); }
    { Args a = good; a.n = -1; expect(run(a), LCREC_EINVAL, "n=-1"); }
    { Args a = good; a.n = (int64_t)1 << 32; expect(run(a), LCREC_EINVAL, "n=4294967296"); }
    { Args a = good; a.nf = -1; expect(run(a), LCREC_EINVAL, "n_frozen=-1"); }
    { Args a = good; a.nf = 9; expect(run(a), LCREC_EINVAL, "n_frozen=9 (0 .. n=8)"); }
    { Args a = good; a.nf = (int64_t)1 << 40; expect(run(a), LCREC_EINVAL, "n_frozen=1099511627776"); }
    { Args a = good; a.n = 0; expect(run(a), LCREC_EINVAL, "n_frozen=3 (0 .. n=0)"); }
    { Args a = good; a.M = -1; expect(run(a), LCREC_EINVAL, "n_members=-1"); }
    { Args a = good; a.G = -1; expect(run(a), LCREC_EINVAL, "n_tuple_groups=-1"); }
    { Args a = good; a.K = nullptr; expect(run(a), LCREC_EINVAL, "K is NULL"); }
    { Args a = good; a.cnt = nullptr; expect(run(a), LCREC_EINVAL, "counters_out is NULL"); }
    { Args a = good; a.K = K0; expect(run(a), LCREC_EINVAL, "K[1]=0"); }
    { Args a = good; a.K = Kneg; expect(run(a), LCREC_EINVAL, "K[2]=-5"); }
    { Args a = good; a.idx = nullptr; expect(run(a), LCREC_EINVAL, "idx is NULL"); }
    { Args a = good; a.mem = nullptr; expect(run(a), LCREC_EINVAL, "tuple_members is NULL"); }
    { Args a = good; a.off = nullptr; expect(run(a), LCREC_EINVAL, "tuple_offsets is NULL"); }
    { Args a = good; a.eh = nullptr; expect(run(a), LCREC_EINVAL, "err_held is NULL"); }
    { Args a = good; a.cand = nullptr; expect(run(a), LCREC_EINVAL, "cand is NULL"); }
    { Args a = good; a.ce = nullptr; expect(run(a), LCREC_EINVAL, "cand_err is NULL"); }
    { Args a = good; a.choice = nullptr; expect(run(a), LCREC_EINVAL, "choice_out is NULL"); }
    { Args a = good; a.idx = q_off4; expect(run(a), LCREC_EINVAL, "must be 8-byte aligned"); }
    { Args a = good; a.mem = q_off4; expect(run(a), LCREC_EINVAL, "must be 8-byte aligned"); }
    { Args a = good; a.off = q_off4; expect(run(a), LCREC_EINVAL, "must be 8-byte aligned"); }
    { Args a = good; a.cand = q_off4; expect(run(a), LCREC_EINVAL, "must be 8-byte aligned"); }
    { Args a = good; a.cnt = q_off4; expect(run(a), LCREC_EINVAL, "must be 8-byte aligned"); }
    { Args a = good; a.ws = p + 4; expect(run(a), LCREC_EINVAL, "must be 8-byte aligned"); }
    { Args a = good; a.eh = f_off2; expect(run(a), LCREC_EINVAL, "must be 4-byte aligned"); }
    { Args a = good; a.ce = f_off2; expect(run(a), LCREC_EINVAL, "must be 4-byte aligned"); }
    { Args a = good; a.choice = c_off2; expect(run(a), LCREC_EINVAL, "must be 4-byte aligned"); }
    { Args a = good; a.K = Kwide; a.L = 13; expect(run(a), LCREC_EUNSUPPORTED, "tuples need 130 bits"); }
    {   // 128 bits pass the key check: the next refusal is the workspace's
        Args a = good; a.K = K128; a.L = 16; a.wsb = 1;
        expect(run(a), LCREC_EWORKSPACE, "workspace of 1 bytes");
    }

    // ---- the workspace query
    const size_t need = lcrec_extend_finish_beam_workspace(8, 4, 3, 4);
    expect_true(need % 256 == 0 && need > 6 * up256(8 * 8) + 6 * up256(16 * 8) + up256(16) + up256(4 * 4), "workspace(n=8, M=4, W=4) covers its arrays",
                need);
    const size_t more = lcrec_extend_finish_beam_workspace(1000, 300, 3, 8);
    expect_true(more > 6 * up256(8000) + 6 * up256(2400 * 8) + up256(2400) + up256(1200), "workspace(n=1000, M=300, W=8) covers its arrays", more);
    expect_true(lcrec_extend_finish_beam_workspace(0, 0, 1, 1) > 0, "workspace(n=0) is sized as one item", lcrec_extend_finish_beam_workspace(0, 0, 1, 1));
    expect_true(lcrec_extend_finish_beam_workspace(8, 4, 0, 4) == 0, "workspace(L=0: refused)", 0);
    expect_true(lcrec_extend_finish_beam_workspace(8, 4, 17, 4) == 0, "workspace(L=17: refused)", 0);
    expect_true(lcrec_extend_finish_beam_workspace(8, 4, 3, 3) == 0, "workspace(width=3: refused)", 0);
    expect_true(lcrec_extend_finish_beam_workspace(-1, 4, 3, 4) == 0, "workspace(n=-1: refused)", 0);
    expect_true(lcrec_extend_finish_beam_workspace(8, -1, 3, 4) == 0, "workspace(n_members=-1: refused)", 0);
    const struct { int64_t n, M; int L, W; } shapes[] = {{8, 4, 3, 4}, {1000, 300, 3, 8}, {0, 0, 1, 1}, {20000, 12000, 16, 8}, {8, 4, 3, 3}};
    for (const auto &s : shapes) {
        const size_t mine = lcrec_extend_finish_beam_workspace(s.n, s.M, s.L, s.W);
        expect_true(mine == lcrec_finish_beam_workspace(s.n, s.M, s.L, s.W), "workspace equals lcrec_finish_beam_workspace", mine);
    }
    {
        Args a = good; a.wsb = need - 1;
        snprintf(word, sizeof word, "workspace of %zu bytes, %zu needed", need - 1, need);
        expect(run(a), LCREC_EWORKSPACE, word);
        a.ws = nullptr; a.wsb = big;
        snprintf(word, sizeof word, "workspace of 0 bytes, %zu needed", need);
        expect(run(a), LCREC_EWORKSPACE, word);
    }
    {   // n_frozen == n: no array but the counters is asked for (the memset of the counters is the first thing that needs a device,
        // so the call is not made here; every check before it is, with n_frozen == n and a refusal behind it)
        Args a = good; a.nf = 8; a.W = 3;
        expect(run(a), LCREC_EINVAL, "width=3");
    }
    printf(failures ? "%d FAILED\n" : "all refusals ok\n", failures);
    return failures ? 1 : 0;
}
