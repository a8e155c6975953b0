// Stand-alone check of the host-side argument checks of lcrec_index_trie_build, lcrec_index_trie_find and
// lcrec_index_trie_mask_logits, for a build with the host code under AddressSanitizer + UBSan (`make trie_refusals`): every refusal
// must come back with its code and a text naming the argument before anything touches a device, so this runs on a build host
// without one.  Also the build's workspace query (0 for refused arguments and for n = 0) and the calls that pass every check with
// nothing to launch.  Not part of liblcrec_hip.so.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/lcrec.h"

static int failures = 0;

static void expect(int rc, int want_rc, const char *who, const char *word)
{
    const char *text = lcrec_last_error();
    const bool ok = rc == want_rc && strstr(text, word) && strstr(text, who);
    printf("%s rc=%d \"%s\"\n", ok ? "ok  " : "FAIL", rc, text);
    if (!ok) ++failures;
}

static void expect_true(bool ok, const char *what)
{
    printf("%s %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) ++failures;
}

int main()
{
    std::vector<double> store(64);
    char *p = reinterpret_cast<char *>(((uintptr_t)store.data() + 15) & ~(uintptr_t)15);
    int64_t *q = reinterpret_cast<int64_t *>(p), *q_off4 = reinterpret_cast<int64_t *>(p + 4);
    int *u = reinterpret_cast<int *>(p), *u_off2 = reinterpret_cast<int *>(p + 2);
    float *f = reinterpret_cast<float *>(p), *f_off2 = reinterpret_cast<float *>(p + 2);
    void *ws = p, *ws_off8 = p + 8;
    const size_t big = (size_t)1 << 40;   // (a size only: nothing is read or written before the refusal)
    const int K3[3] = {48, 100, 7}, K0[3] = {48, 0, 7}, Kneg[3] = {48, 100, -5};
    int K256[LCREC_MAX_LEVELS + 1], K512[LCREC_MAX_LEVELS];
    for (int l = 0; l <= LCREC_MAX_LEVELS; ++l) K256[l] = 256;
    for (int l = 0; l < LCREC_MAX_LEVELS; ++l) K512[l] = 512;

    auto fresh = [&]() {
        lcrec_index_trie t;
        memset(&t, 0, sizeof t);
        t.order = q; t.counts = q; t.child = q; t.code = u; t.first = q;
        return t;
    };
    auto built = [&]() {
        lcrec_index_trie t = fresh();
        t.n = 8; t.L = 3;
        for (int l = 0; l < 3; ++l) t.K[l] = K3[l];
        return t;
    };

    // ---- lcrec_index_trie_build(idx, idx_stride, n, L, K, trie, workspace, bytes, stream)
    const char *who = "trie_build";
    lcrec_index_trie t = fresh();
    expect(lcrec_index_trie_build(q, 0, 8, 3, nullptr, &t, ws, big, nullptr), LCREC_EINVAL, who, "K is NULL");
    expect(lcrec_index_trie_build(q, 0, 8, 0, K3, &t, ws, big, nullptr), LCREC_EINVAL, who, "L=0");
    expect(lcrec_index_trie_build(q, 0, 8, LCREC_MAX_LEVELS + 1, K256, &t, ws, big, nullptr), LCREC_EINVAL, who, "L=17");
    expect(lcrec_index_trie_build(q, 0, -1, 3, K3, &t, ws, big, nullptr), LCREC_EINVAL, who, "n=-1");
    expect(lcrec_index_trie_build(q, 0, 8, 3, K0, &t, ws, big, nullptr), LCREC_EINVAL, who, "K[1]=0");
    expect(lcrec_index_trie_build(q, 0, 8, 3, Kneg, &t, ws, big, nullptr), LCREC_EINVAL, who, "K[2]=-5");
    expect(lcrec_index_trie_build(q, 0, 8, LCREC_MAX_LEVELS, K512, &t, ws, big, nullptr), LCREC_EINVAL, who, "144 key bits (> 128)");
    expect(lcrec_index_trie_build(q, 2, 8, 3, K3, &t, ws, big, nullptr), LCREC_EINVAL, who, "idx_stride=2 < L=3");
    expect(lcrec_index_trie_build(q, -1, 8, 3, K3, &t, ws, big, nullptr), LCREC_EINVAL, who, "idx_stride=-1");
    expect(lcrec_index_trie_build(nullptr, 0, 8, 3, K3, &t, ws, big, nullptr), LCREC_EINVAL, who, "idx is NULL");
    expect(lcrec_index_trie_build(q_off4, 0, 8, 3, K3, &t, ws, big, nullptr), LCREC_EINVAL, who, "idx must be 8-byte aligned");
    expect(lcrec_index_trie_build(q, 0, 8, 3, K3, nullptr, ws, big, nullptr), LCREC_EINVAL, who, "trie is NULL");
    {
        lcrec_index_trie b = fresh(); b.order = nullptr;
        expect(lcrec_index_trie_build(q, 0, 8, 3, K3, &b, ws, big, nullptr), LCREC_EINVAL, who, "trie->order is NULL");
        b = fresh(); b.counts = nullptr;
        expect(lcrec_index_trie_build(q, 0, 8, 3, K3, &b, ws, big, nullptr), LCREC_EINVAL, who, "trie->counts is NULL");
        b = fresh(); b.child = nullptr;
        expect(lcrec_index_trie_build(q, 0, 8, 3, K3, &b, ws, big, nullptr), LCREC_EINVAL, who, "trie->child is NULL");
        b = fresh(); b.code = nullptr;
        expect(lcrec_index_trie_build(q, 0, 8, 3, K3, &b, ws, big, nullptr), LCREC_EINVAL, who, "trie->code is NULL");
        b = fresh(); b.first = nullptr;
        expect(lcrec_index_trie_build(q, 0, 8, 3, K3, &b, ws, big, nullptr), LCREC_EINVAL, who, "trie->first is NULL");
        b = fresh(); b.child = q_off4;
        expect(lcrec_index_trie_build(q, 0, 8, 3, K3, &b, ws, big, nullptr), LCREC_EINVAL, who, "must be 8-byte aligned");
        b = fresh(); b.code = u_off2;
        expect(lcrec_index_trie_build(q, 0, 8, 3, K3, &b, ws, big, nullptr), LCREC_EINVAL, who, "trie->code must be 4-byte aligned");
    }
    expect(lcrec_index_trie_build(q, 0, 8, 3, K3, &t, ws_off8, big, nullptr), LCREC_EINVAL, who, "workspace must be 16-byte aligned");
    const size_t need = lcrec_index_trie_build_workspace(8, 3);
    expect_true(need >= 11 * 256 && need % 256 == 0, "workspace(n=8): eleven arrays of 256 bytes and the sorts' scratch");
    expect_true(lcrec_index_trie_build_workspace(8, 16) == need, "workspace(n=8) does not depend on L");
    expect_true(lcrec_index_trie_build_workspace(0, 3) == 0, "workspace(n=0) = 0");
    expect_true(lcrec_index_trie_build_workspace(-1, 3) == 0, "workspace(n=-1: refused) = 0");
    expect_true(lcrec_index_trie_build_workspace(8, 0) == 0 && lcrec_index_trie_build_workspace(8, 17) == 0, "workspace(L=0, L=17: refused) = 0");
    {
        char word[96];
        snprintf(word, sizeof word, "workspace of %zu bytes, %zu needed", need - 1, need);
        expect(lcrec_index_trie_build(q, 0, 8, 3, K3, &t, ws, need - 1, nullptr), LCREC_EWORKSPACE, who, word);
        snprintf(word, sizeof word, "workspace of 0 bytes, %zu needed", need);
        expect(lcrec_index_trie_build(q, 0, 8, 3, K3, &t, nullptr, big, nullptr), LCREC_EWORKSPACE, who, word);
    }

    // ---- lcrec_index_trie_find(trie, prefix, prefix_stride, B, depth, node_out, depth_out, stream)
    who = "trie_find";
    t = built();
    expect(lcrec_index_trie_find(nullptr, q, 0, 4, 3, q, u, nullptr), LCREC_EINVAL, who, "trie is NULL");
    {
        lcrec_index_trie b = built(); b.L = 0;
        expect(lcrec_index_trie_find(&b, q, 0, 4, 0, q, u, nullptr), LCREC_EINVAL, who, "L=0");
        b = built(); b.L = 17;
        expect(lcrec_index_trie_find(&b, q, 0, 4, 0, q, u, nullptr), LCREC_EINVAL, who, "L=17");
        b = built(); b.n = -2;
        expect(lcrec_index_trie_find(&b, q, 0, 4, 3, q, u, nullptr), LCREC_EINVAL, who, "n=-2");
        b = built(); b.K[2] = 0;
        expect(lcrec_index_trie_find(&b, q, 0, 4, 3, q, u, nullptr), LCREC_EINVAL, who, "K[2]=0");
        b = built(); b.code = nullptr;
        expect(lcrec_index_trie_find(&b, q, 0, 4, 3, q, u, nullptr), LCREC_EINVAL, who, "trie->code is NULL");
    }
    expect(lcrec_index_trie_find(&t, q, 0, -1, 3, q, u, nullptr), LCREC_EINVAL, who, "B=-1");
    expect(lcrec_index_trie_find(&t, q, 0, 4, -1, q, u, nullptr), LCREC_EINVAL, who, "depth=-1 outside [0, L=3]");
    expect(lcrec_index_trie_find(&t, q, 0, 4, 4, q, u, nullptr), LCREC_EINVAL, who, "depth=4 outside [0, L=3]");
    expect(lcrec_index_trie_find(&t, q, 2, 4, 3, q, u, nullptr), LCREC_EINVAL, who, "prefix_stride=2 < depth=3");
    expect(lcrec_index_trie_find(&t, q, -3, 4, 3, q, u, nullptr), LCREC_EINVAL, who, "prefix_stride=-3");
    expect(lcrec_index_trie_find(&t, nullptr, 0, 4, 3, q, u, nullptr), LCREC_EINVAL, who, "prefix is NULL");
    expect(lcrec_index_trie_find(&t, q, 0, 4, 3, nullptr, u, nullptr), LCREC_EINVAL, who, "node_out is NULL");
    expect(lcrec_index_trie_find(&t, q_off4, 0, 4, 3, q, u, nullptr), LCREC_EINVAL, who, "must be 8-byte aligned");
    expect(lcrec_index_trie_find(&t, q, 0, 4, 3, q_off4, u, nullptr), LCREC_EINVAL, who, "must be 8-byte aligned");
    expect(lcrec_index_trie_find(&t, q, 0, 4, 3, q, u_off2, nullptr), LCREC_EINVAL, who, "depth_out must be 4-byte aligned");
    expect_true(lcrec_index_trie_find(&t, q, 0, 0, 3, q, u, nullptr) == LCREC_OK, "find, B = 0: LCREC_OK, no launch");
    expect_true(lcrec_index_trie_find(&t, nullptr, 0, 0, 0, nullptr, nullptr, nullptr) == LCREC_OK, "find, B = 0 with no buffers: LCREC_OK");

    // ---- lcrec_index_trie_mask_logits(trie, node, B, depth, token_ids, eos, logits, ld, V, stream)
    who = "trie_mask";
    expect(lcrec_index_trie_mask_logits(nullptr, q, 4, 1, u, 2, f, 100, 100, nullptr), LCREC_EINVAL, who, "trie is NULL");
    {
        lcrec_index_trie b = built(); b.L = 0;
        expect(lcrec_index_trie_mask_logits(&b, q, 4, 0, u, 2, f, 100, 100, nullptr), LCREC_EINVAL, who, "L=0");
        b = built(); b.K[0] = -1;
        expect(lcrec_index_trie_mask_logits(&b, q, 4, 1, u, 2, f, 100, 100, nullptr), LCREC_EINVAL, who, "K[0]=-1");
        b = built(); b.counts = nullptr;
        expect(lcrec_index_trie_mask_logits(&b, q, 4, 1, u, 2, f, 100, 100, nullptr), LCREC_EINVAL, who, "trie->counts is NULL");
    }
    expect(lcrec_index_trie_mask_logits(&t, q, -1, 1, u, 2, f, 100, 100, nullptr), LCREC_EINVAL, who, "B=-1");
    expect(lcrec_index_trie_mask_logits(&t, q, 4, -1, u, 2, f, 100, 100, nullptr), LCREC_EINVAL, who, "depth=-1 outside [0, L=3]");
    expect(lcrec_index_trie_mask_logits(&t, q, 4, 4, u, 2, f, 100, 100, nullptr), LCREC_EINVAL, who, "depth=4 outside [0, L=3]");
    expect(lcrec_index_trie_mask_logits(&t, q, 4, 1, u, 2, f, 100, 0, nullptr), LCREC_EINVAL, who, "V=0");
    expect(lcrec_index_trie_mask_logits(&t, q, 4, 1, u, 2, f, 99, 100, nullptr), LCREC_EINVAL, who, "ld=99 < V=100");
    expect(lcrec_index_trie_mask_logits(&t, nullptr, 4, 1, u, 2, f, 100, 100, nullptr), LCREC_EINVAL, who, "node is NULL");
    expect(lcrec_index_trie_mask_logits(&t, q, 4, 1, u, 2, nullptr, 100, 100, nullptr), LCREC_EINVAL, who, "logits is NULL");
    expect(lcrec_index_trie_mask_logits(&t, q_off4, 4, 1, u, 2, f, 100, 100, nullptr), LCREC_EINVAL, who, "node must be 8-byte aligned");
    expect(lcrec_index_trie_mask_logits(&t, q, 4, 1, u, 2, f_off2, 100, 100, nullptr), LCREC_EINVAL, who, "must be 4-byte aligned");
    expect(lcrec_index_trie_mask_logits(&t, q, 4, 1, u_off2, 2, f, 100, 100, nullptr), LCREC_EINVAL, who, "must be 4-byte aligned");
    expect_true(lcrec_index_trie_mask_logits(&t, q, 0, 1, u, 2, f, 100, 100, nullptr) == LCREC_OK, "mask, B = 0: LCREC_OK, no launch");
    expect_true(lcrec_index_trie_mask_logits(&t, nullptr, 0, 3, nullptr, -1, nullptr, 101, 100, nullptr) == LCREC_OK,
                "mask, B = 0 with no buffers: LCREC_OK");

    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
