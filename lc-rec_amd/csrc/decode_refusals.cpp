// Stand-alone check of lcrec_decode_tuples' host-side argument checks, for a build with the host code under AddressSanitizer +
// UBSan (`make decode_refusals`): every refusal must come back with its code and a text naming the argument -- a layer by its
// number -- before anything touches a device, so this runs on a build host without one.  Also the workspace queries (0 for refused
// arguments) and the plan of the chunk walk at a few chunkings.  Not part of liblcrec_hip.so.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/lcrec.h"

static int failures = 0;

static void expect(int rc, int want_rc, const char *word)
{
    const char *text = lcrec_last_error();
    const bool ok = rc == want_rc && strstr(text, word) && strstr(text, "decode_tuples");
    printf("%s rc=%d \"%s\"\n", ok ? "ok  " : "FAIL", rc, text);
    if (!ok) ++failures;
}

static void expect_true(bool ok, const char *what)
{
    printf("%s %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) ++failures;
}

static void expect_size(size_t got, size_t want, const char *what)
{
    const bool ok = got == want;
    printf("%s %s = %zu (expected %zu)\n", ok ? "ok  " : "FAIL", what, got, want);
    if (!ok) ++failures;
}

static int64_t up256(int64_t v) { return (v + 255) / 256 * 256; }

int main()
{
    std::vector<double> store(64);
    char *p = reinterpret_cast<char *>(((uintptr_t)store.data() + 15) & ~(uintptr_t)15);
    float *f = reinterpret_cast<float *>(p), *f_off8 = reinterpret_cast<float *>(p + 8);
    int64_t *q = reinterpret_cast<int64_t *>(p), *q_off4 = reinterpret_cast<int64_t *>(p + 4);
    uint32_t *u = reinterpret_cast<uint32_t *>(p), *u_off2 = reinterpret_cast<uint32_t *>(p + 2);
    void *ws = p, *ws_off8 = p + 8;
    const size_t big = (size_t)1 << 40;   // (a size only: nothing is read or written before the refusal)
    const int K3[3] = {48, 100, 7}, K0[3] = {48, 0, 7}, Kneg[3] = {48, 100, -5};
    const int D[3] = {16, 40, 100}, D44[3] = {16, 44, 100}, D0[3] = {16, 40, 0}, Dneg[3] = {16, -8, 100};
    const float *const PP[2] = {f, f}, *const P_null1[2] = {f, nullptr}, *const P_null0[2] = {nullptr, f}, *const P_off[2] = {f, f_off8},
                       *const NN[2] = {nullptr, nullptr};
    char word[96];

    // ---- every refusal, each before a device is touched.  The full call: idx, stride, n, codebooks, K, L, dims, n_layers, W, b,
    // bn_scale, bn_shift, xq_out, out, x, l1, err_out, flags_out, workspace, bytes, stream
    expect(lcrec_decode_tuples(q, 0, 8, f, nullptr, 3, D, 2, PP, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "K is NULL");
    expect(lcrec_decode_tuples(q, 0, 8, f, K3, 3, nullptr, 2, PP, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "dims is NULL");
    expect(lcrec_decode_tuples(q, 0, 8, f, K3, 0, D, 2, PP, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "L=0");
    expect(lcrec_decode_tuples(q, 0, 8, f, K3, LCREC_MAX_LEVELS + 1, D, 2, PP, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "L=17");
    expect(lcrec_decode_tuples(q, 0, 8, f, K3, 3, D, 0, PP, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "n_layers=0");
    expect(lcrec_decode_tuples(q, 0, 8, f, K3, 3, D, LCREC_MAX_LAYERS + 1, PP, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "n_layers=17");
    expect(lcrec_decode_tuples(q, 0, -1, f, K3, 3, D, 2, PP, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "n=-1");
    expect(lcrec_debug_decode_tuples(q, 0, 8, f, K3, 3, D, 2, PP, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr, -4), LCREC_EINVAL, "chunk_rows=-4");
    for (int e : {0, 8, 24, 128, -16}) {
        const int De[3] = {e, 40, 100};
        snprintf(word, sizeof word, "e_dim=%d", e);
        expect(lcrec_decode_tuples(q, 0, 8, f, K3, 3, De, 2, PP, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, word);
    }
    expect(lcrec_decode_tuples(q, 0, 8, f, K0, 3, D, 2, PP, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "K[1]=0");
    expect(lcrec_decode_tuples(q, 0, 8, f, Kneg, 3, D, 2, PP, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "K[2]=-5");
    expect(lcrec_decode_tuples(q, 0, 8, f, K3, 3, D0, 2, PP, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "layer 1: dims[2]=0");
    expect(lcrec_decode_tuples(q, 0, 8, f, K3, 3, Dneg, 2, PP, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "layer 0: dims[1]=-8");
    // a width lcrec_linear_forward refuses: its code, and the layer by number -- also at n = 0, and whatever the chunking
    {
        lcrec_gemm_launch steps[4];
        const int theirs = lcrec_debug_linear_forward_plan(8, 44, 100, 256, steps, 4);
        expect_true(theirs == LCREC_EUNSUPPORTED, "lcrec_linear_forward's own plan refuses in_dim = 44 as LCREC_EUNSUPPORTED");
        expect(lcrec_decode_tuples(q, 0, 8, f, K3, 3, D44, 2, PP, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr), theirs, "layer 1 (in_dim=44, out_dim=100");
        expect(lcrec_decode_tuples(q, 0, 0, f, K3, 3, D44, 2, PP, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr), theirs, "layer 1 (in_dim=44, out_dim=100");
        expect(lcrec_debug_decode_tuples(q, 0, 8, f, K3, 3, D44, 2, PP, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr, 3), theirs, "layer 1 (in_dim=44, out_dim=100");
    }
    expect(lcrec_decode_tuples(q, 2, 8, f, K3, 3, D, 2, PP, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "idx_stride=2 < L=3");
    expect(lcrec_decode_tuples(q, -1, 8, f, K3, 3, D, 2, PP, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "idx_stride=-1");
    expect(lcrec_decode_tuples(nullptr, 0, 8, f, K3, 3, D, 2, PP, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "idx is NULL");
    expect(lcrec_decode_tuples(q, 0, 8, nullptr, K3, 3, D, 2, PP, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "codebooks is NULL");
    expect(lcrec_decode_tuples(q, 0, 8, f, K3, 3, D, 2, PP, PP, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, u, ws, big, nullptr), LCREC_EINVAL, "no output asked for");
    expect(lcrec_decode_tuples(q, 0, 8, f, K3, 3, D, 2, PP, PP, nullptr, nullptr, f, f, nullptr, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "x and err_out are given together");
    expect(lcrec_decode_tuples(q, 0, 8, f, K3, 3, D, 2, PP, PP, nullptr, nullptr, f, f, f, 0, nullptr, u, ws, big, nullptr), LCREC_EINVAL, "x and err_out are given together");
    expect(lcrec_decode_tuples(q, 0, 8, f, K3, 3, D, 2, nullptr, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "W is NULL");
    expect(lcrec_decode_tuples(q, 0, 8, f, K3, 3, D, 2, PP, nullptr, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "b is NULL");
    expect(lcrec_decode_tuples(q, 0, 8, f, K3, 3, D, 2, P_null1, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "layer 1: W[1] is NULL");
    expect(lcrec_decode_tuples(q, 0, 8, f, K3, 3, D, 2, PP, PP, PP, P_null0, f, f, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "layer 0: bn_scale and bn_shift");
    expect(lcrec_decode_tuples(q, 0, 8, f, K3, 3, D, 2, PP, PP, P_null1, nullptr, f, f, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "layer 0: bn_scale and bn_shift");
    expect(lcrec_decode_tuples(q, 0, 8, f, K3, 3, D, 2, P_off, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "layer 1: W[1] must be 16-byte aligned");
    expect(lcrec_decode_tuples(q, 0, 8, f_off8, K3, 3, D, 2, PP, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "16-byte aligned");
    expect(lcrec_decode_tuples(q, 0, 8, f, K3, 3, D, 2, PP, PP, nullptr, nullptr, f_off8, f, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "16-byte aligned");
    expect(lcrec_decode_tuples(q, 0, 8, f, K3, 3, D, 2, PP, PP, nullptr, nullptr, f, f_off8, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "16-byte aligned");
    expect(lcrec_decode_tuples(q, 0, 8, f, K3, 3, D, 2, PP, PP, nullptr, nullptr, f, f, f_off8, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "16-byte aligned");
    expect(lcrec_decode_tuples(q, 0, 8, f, K3, 3, D, 2, PP, PP, nullptr, nullptr, f, f, f, 0, f_off8, u, ws, big, nullptr), LCREC_EINVAL, "16-byte aligned");
    expect(lcrec_decode_tuples(q, 0, 8, f, K3, 3, D, 2, PP, PP, nullptr, nullptr, f, f, f, 0, f, u, ws_off8, big, nullptr), LCREC_EINVAL, "16-byte aligned");
    expect(lcrec_decode_tuples(q_off4, 0, 8, f, K3, 3, D, 2, PP, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, big, nullptr), LCREC_EINVAL, "idx must be 8-byte aligned");
    expect(lcrec_decode_tuples(q, 0, 8, f, K3, 3, D, 2, PP, PP, nullptr, nullptr, f, f, f, 0, f, u_off2, ws, big, nullptr), LCREC_EINVAL, "flags_out must be 4-byte aligned");

    // ---- the workspace: two activation buffers and the q slab; the last layer's output counts when `out` is not asked for
    expect_size(lcrec_decode_tuples_workspace(8, D, 2, K3, 3, 1), 2 * 1280 + 512, "workspace(n=8, 16-40-100, out given)");
    expect_size(lcrec_decode_tuples_workspace(8, D, 2, K3, 3, 0), 2 * 3328 + 512, "workspace(n=8, 16-40-100, out NULL)");
    expect_size(lcrec_decode_tuples_workspace(0, D, 2, K3, 3, 1), 2 * 256 + 256, "workspace(n=0: sized as one row)");
    expect_size(lcrec_decode_tuples_workspace(8, D, 1, K3, 3, 1), 512, "workspace(one layer, out given: the q slab alone)");
    expect_size(lcrec_decode_tuples_workspace(8, D44, 2, K3, 3, 1), 0, "workspace(in_dim=44: refused)");
    expect_size(lcrec_decode_tuples_workspace(8, D0, 2, K3, 3, 1), 0, "workspace(dims[2]=0: refused)");
    expect_size(lcrec_decode_tuples_workspace(8, D, 2, nullptr, 3, 1), 0, "workspace(K NULL: refused)");
    expect_size(lcrec_decode_tuples_workspace(8, nullptr, 2, K3, 3, 1), 0, "workspace(dims NULL: refused)");
    expect_size(lcrec_decode_tuples_workspace(8, D, 2, K0, 3, 1), 0, "workspace(K[1]=0: refused)");
    expect_size(lcrec_decode_tuples_workspace(-1, D, 2, K3, 3, 1), 0, "workspace(n=-1: refused)");
    expect_size(lcrec_debug_decode_tuples_workspace(8, D, 2, K3, 3, 1, -1), 0, "workspace(chunk_rows=-1: refused)");
    expect(lcrec_decode_tuples(q, 0, 8, f, K3, 3, D, 2, PP, PP, nullptr, nullptr, f, f, f, 0, f, u, ws, 3071, nullptr), LCREC_EWORKSPACE, "workspace of 3071 bytes, 3072 needed");
    expect(lcrec_decode_tuples(q, 0, 8, f, K3, 3, D, 2, PP, PP, nullptr, nullptr, f, nullptr, f, 0, f, u, nullptr, big, nullptr), LCREC_EWORKSPACE, "workspace of 0 bytes, 7168 needed");
    expect(lcrec_decode_tuples(q, 0, 8, f, K3, 3, D, 2, PP, PP, nullptr, nullptr, nullptr, f, nullptr, 0, nullptr, u, ws, 100, nullptr), LCREC_EWORKSPACE, "workspace of 100 bytes, 3072 needed");
    // past every check with nothing to do: n = 0 launches nothing; xq_out alone needs neither layers nor a workspace
    expect_true(lcrec_decode_tuples(q, 0, 0, f, K3, 3, D, 2, PP, PP, nullptr, nullptr, f, f, f, 1, f, u, ws, big, nullptr) == LCREC_OK, "n = 0: LCREC_OK");
    expect_true(lcrec_decode_tuples(q, 0, 0, f, K3, 3, D, 2, PP, NN, nullptr, nullptr, nullptr, f, nullptr, 0, nullptr, nullptr, ws, big, nullptr) == LCREC_OK,
                "n = 0, out alone, no biases, no flags: LCREC_OK");
    expect_true(lcrec_decode_tuples(q, 0, 0, f, K3, 3, D, 2, nullptr, nullptr, nullptr, nullptr, f, nullptr, nullptr, 0, nullptr, u, nullptr, 0, nullptr) == LCREC_OK,
                "n = 0, xq_out alone: no W, no b, no workspace");

    // ---- the plan at a few chunkings
    expect_true(lcrec_debug_decode_tuples_plan(8, D, 2, K3, 3, 1, 0, nullptr) == LCREC_EINVAL && strstr(lcrec_last_error(), "plan_out"), "plan: NULL plan_out is refused");
    const int n = 1000;
    for (int want_out : {0, 1}) {
        for (int64_t chunk : {(int64_t)0, (int64_t)1, (int64_t)64, (int64_t)100, (int64_t)n - 1, (int64_t)n, (int64_t)n + 1}) {
            lcrec_decode_plan pl;
            memset(&pl, 0xEE, sizeof pl);
            const int rc = lcrec_debug_decode_tuples_plan(n, D, 2, K3, 3, want_out, chunk, &pl);
            const int64_t rows = chunk == 0 || chunk > n ? n : chunk, widest = want_out ? 40 : 100;
            const bool ok = rc == LCREC_OK && pl.n == n && pl.chunk_rows == rows && pl.n_chunks == (n + rows - 1) / rows &&
                            pl.last_chunk_rows == n - (pl.n_chunks - 1) * rows && pl.widest == widest &&
                            pl.act_bytes == up256(rows * widest * 4) && pl.act_offset[0] == 0 && pl.act_offset[1] == pl.act_bytes &&
                            pl.q_offset == 2 * pl.act_bytes && pl.q_bytes == up256(rows * 16 * 4) && pl.total_bytes == pl.q_offset + pl.q_bytes &&
                            (size_t)pl.total_bytes == lcrec_debug_decode_tuples_workspace(n, D, 2, K3, 3, want_out, chunk);
            snprintf(word, sizeof word, "plan(n=1000, want_out=%d, chunk_rows=%lld): %lld chunks of %lld, %lld bytes", want_out, (long long)chunk,
                     (long long)pl.n_chunks, (long long)pl.chunk_rows, (long long)pl.total_bytes);
            expect_true(ok, word);
        }
    }
    {
        lcrec_decode_plan pl;
        expect_true(lcrec_debug_decode_tuples_plan(3 * lcrec_decode_tuples_chunk_rows() + 5, D, 2, K3, 3, 1, 0, &pl) == LCREC_OK && pl.n_chunks == 4 &&
                        pl.last_chunk_rows == 5 && pl.chunk_rows == lcrec_decode_tuples_chunk_rows(), "plan: the built-in chunk, three whole chunks and 5 rows");
        expect_true(lcrec_debug_decode_tuples_plan(0, D, 2, K3, 3, 1, 0, &pl) == LCREC_OK && pl.n_chunks == 0 && pl.last_chunk_rows == 0, "plan: n = 0 has no chunk");
    }
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
