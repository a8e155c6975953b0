// Beam-search residual quantiser: the W best whole tuples of every item (lcrec_rq_beam; opt-in, generate --beam W).
//
// lcrec_rq_assign walks the levels greedily: nearest code, subtract, move on.  This pass keeps W partial tuples per item, each with
// its own residual, scores all W * K children at a level and keeps the W best.  Beyond the reference, which is greedy throughout.
//
// The rule: rq_walk.h states the quantiser's arithmetic; include/lcrec.h, lcrec_rq_beam, is this pass's contract and
// tests/beam_ref.py restates it in numpy.  One live beam to start with: r = z_i, the empty tuple.  Per level l with P live beams:
//   s(p, k) = d(r_p, C_l[k]); a NaN counts as +inf and is reported as +inf
//   keep      the first min(W, P * K) candidates by (s ascending, p ascending, k ascending): the new beams, in that order
//   residual  of the new beam from (p, k): the residual of r_p behind C_l[k]
// and after the last level score = s of the last candidate, err = the chain of squares of r_L.
//
// Shape: one launch per level.  An item owns W consecutive lanes, one per parent beam, so 256 / W items per workgroup and an item
// never straddles a wave.  The level's codebook (row stride E + 4 floats) and its cc go to LDS once per workgroup as in audit.hip.
// A lane holds its parent's residual in E registers and sweeps k = 0 .. K-1 once -- every lane of the wave reads the same row,
// which LDS serves as a broadcast -- keeping its own W best (score, k) in registers, sorted, by a branch-free insertion that only
// runs when the candidate beats the list's tail (strict <, so the earlier code stays ahead on a tie).  Lanes of parents that are not
// live idle through the sweep.  The item's W lists are then merged in W rounds: every lane offers the head of its list, a butterfly
// of xor shuffles inside the item's lanes finds the least (score, p, k), the lane that offered it drops its head, and lane b keeps
// the winner of round b.  Lane b then reads its parent's residual back (the other half of the ping-pong workspace, or z), gathers
// the code row from LDS, takes the three operations and writes its residual and its (parent, code) link; the last level walks the
// links back to write the tuple.  No atomic, no barrier after the staging.  The grid is the number of workgroups resident at once,
// a grid-stride loop over blocks of 256 / W items does the rest.
#include "rq_walk.h"

namespace lcrec {

constexpr int BEAM_THREADS = 256;
constexpr int BEAM_MAX_PER_CU = 4;     // the register bound at e = 64 (112 .. 125 VGPRs for W > 1) and at e = 32, W = 8 (101); the
                                       // staged level's LDS may allow fewer.  (e = 64, W = 1: 136 VGPRs, 3 fit and the rest queue.)
constexpr int BEAM_CODE_BITS = 20;     // a link is parent << 20 | code: a level that fits in LDS has far fewer than 2^20 codes
constexpr int BEAM_NO_ENTRY = 0x7FFFFFFF;

struct BeamParams {
    const float *r_in;       // residual of parent p of item i at r_in[i * in_stride + p * E] (level 0: the latents, in_stride = E)
    int64_t in_stride;
    float *r_out;            // [n][W][E] residual of the new beams, or NULL (last level: resid_out)
    const float *cb;         // [K][E] this level's rows
    int64_t n;
    int K, L, l;
    int P_in, P_out;         // live beams entering and leaving the level
    int *links;              // [L][n][W]: beam b of item i at level l came from links[(l * n + i) * W + b] = parent << 20 | code
    int64_t *tuples;         // [n][W][L], written by the last level
    float *score, *err;      // [n][W], written by the last level
};

// (score, key) before (score', key'): score ascending, then the key, which is parent << 20 | code, or BEAM_NO_ENTRY behind everything
__device__ __forceinline__ bool beam_before(float s, int key, float s2, int key2) { return s < s2 || (s == s2 && key < key2); }

template <int E, int W>
__global__ __launch_bounds__(BEAM_THREADS) void rq_beam_level_kernel(BeamParams p)
{
    constexpr int S = E + 4;   // LDS row stride (floats)
    extern __shared__ __attribute__((aligned(16))) unsigned char beam_smem[];
    const int K = p.K;
    float *cbs = reinterpret_cast<float *>(beam_smem);   // [K][S]
    float *ccs = cbs + (size_t)K * S;                    // [K]
    const int tid = threadIdx.x;

    stage_level<E, S, BEAM_THREADS>(p.cb, K, cbs, ccs);

    constexpr int ITEMS = BEAM_THREADS / W;
    const int L = p.L, l = p.l;
    const int slot = tid % W;                            // the parent this lane sweeps for, then the new beam it becomes
    const float inf = __builtin_inff();
    for (int64_t base = (int64_t)blockIdx.x * ITEMS; base < p.n; base += (int64_t)gridDim.x * ITEMS) {
        const int64_t i = base + tid / W;
        if (i >= p.n) continue;                          // all W lanes of an item leave together (no barrier follows)

        // ---- this lane's W best codes for its parent, sorted; key < 0: no entry yet
        float s[W];
        int kk[W];
#pragma unroll
        for (int j = 0; j < W; ++j) { s[j] = inf; kk[j] = -1; }
        float x[E];
        if (slot < p.P_in) {
            load_row<E>(p.r_in + i * p.in_stride + (int64_t)slot * E, x);
            const float xx = sq_chain<E>(x);
            for (int k = 0; k < K; ++k) {
                const float d = nan_as_inf(code_distance<E, f32x4>(x, xx, cbs + k * S, ccs[k]));
                if (d < s[W - 1] || kk[W - 1] < 0) {
#pragma unroll
                    for (int j = W - 1; j >= 1; --j) {
                        const bool up = d < s[j - 1] || kk[j - 1] < 0;        // the entry above moves down into j
                        const bool here = d < s[j] || kk[j] < 0;             // ... or the candidate lands in j
                        s[j] = up ? s[j - 1] : (here ? d : s[j]);
                        kk[j] = up ? kk[j - 1] : (here ? k : kk[j]);
                    }
                    const bool first = d < s[0] || kk[0] < 0;
                    s[0] = first ? d : s[0];
                    kk[0] = first ? k : kk[0];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < W; ++j) kk[j] = kk[j] < 0 ? BEAM_NO_ENTRY : ((slot << BEAM_CODE_BITS) | kk[j]);

        // ---- merge the item's W lists: round b's winner goes to lane b
        float my_s = inf;
        int my_key = BEAM_NO_ENTRY;
#pragma unroll
        for (int b = 0; b < W; ++b) {
            float ws = s[0];
            int wk = kk[0];
#pragma unroll
            for (int m = 1; m < W; m <<= 1) {
                const float os = __shfl_xor(ws, m, 64);
                const int ok = __shfl_xor(wk, m, 64);
                const bool take = beam_before(os, ok, ws, wk);
                ws = take ? os : ws;
                wk = take ? ok : wk;
            }
            if (slot == b) { my_s = ws; my_key = wk; }
            const bool won = kk[0] == wk;                                     // keys of entries are distinct; no-entries all drop
#pragma unroll
            for (int j = 0; j < W - 1; ++j) {
                s[j] = won ? s[j + 1] : s[j];
                kk[j] = won ? kk[j + 1] : kk[j];
            }
            s[W - 1] = won ? inf : s[W - 1];
            kk[W - 1] = won ? BEAM_NO_ENTRY : kk[W - 1];
        }

        // ---- the new beam `slot`
        const int64_t o = i * W + slot;
        const bool last = l == L - 1;
        // a dead beam: only the outputs know of it.  (A live slot always wins an entry -- the P_in lists hold at least P_out of them --
        // so the second test never fires; it keeps an address from being formed out of the no-entry key.)
        if (slot >= p.P_out || my_key == BEAM_NO_ENTRY) {
            if (last) {
                for (int j = 0; j < L; ++j) p.tuples[o * L + j] = -1;
                p.score[o] = inf;
                p.err[o] = inf;
                if (p.r_out) {
#pragma unroll
                    for (int j = 0; j < E; ++j) x[j] = inf;
                    store_row<E>(p.r_out + o * E, x);
                }
            }
            continue;
        }
        const int parent = my_key >> BEAM_CODE_BITS, code = my_key & ((1 << BEAM_CODE_BITS) - 1);
        load_row<E>(p.r_in + i * p.in_stride + (int64_t)parent * E, x);
        residual_behind<E>(x, cbs + code * S);
        if (p.r_out) store_row<E>(p.r_out + o * E, x);
        if (!last) {
            p.links[((int64_t)l * p.n + i) * W + slot] = my_key;
            continue;
        }
        p.err[o] = sq_chain<E>(x);
        p.score[o] = my_s;
        p.tuples[o * L + l] = (int64_t)code;
        int at = parent;                                                      // back along the links of the earlier launches
        for (int j = l - 1; j >= 0; --j) {
            const int link = p.links[((int64_t)j * p.n + i) * W + at];
            p.tuples[o * L + j] = (int64_t)(link & ((1 << BEAM_CODE_BITS) - 1));
            at = link >> BEAM_CODE_BITS;
        }
    }
}

// Two halves of residuals [n][W][e] that the levels alternate between (one for L == 2, none for L == 1), then the links of the
// levels before the last, [L - 1][n][W] ints.
static size_t beam_half_bytes(int64_t n, int e, int width) { return align_up((size_t)n * width * e * sizeof(float), 256); }
static size_t beam_workspace_bytes(int64_t n, int e, int L, int width)
{
    if (L < 2 || n <= 0) return 0;
    return (size_t)(L == 2 ? 1 : 2) * beam_half_bytes(n, e, width) + align_up((size_t)(L - 1) * n * width * sizeof(int), 256);
}

static bool beam_width_ok(int width) { return width == 1 || width == 2 || width == 4 || width == 8; }

size_t rq_beam_workspace(int64_t n, int e, const int *K, int L, int width)
{
    if (!K || n < 0 || L < 1 || L > LCREC_MAX_LEVELS || !e_supported(e) || !beam_width_ok(width)) return 0;
    for (int l = 0; l < L; ++l)
        if (K[l] < 1 || !rq_level_fits(K[l], e, L)) return 0;
    return beam_workspace_bytes(n, e, L, width);
}

int rq_beam(const float *z, int64_t n, int e, const float *codebooks, const int *K, int L, int width, int64_t *tuples_out,
            float *score_out, float *err_out, float *resid_out, void *workspace, size_t workspace_bytes, hipStream_t stream)
{
    const char *who = "rq_beam";
    if (!K) return fail(LCREC_EINVAL, "%s: K is NULL", who);
    if (L < 1 || L > LCREC_MAX_LEVELS) return fail(LCREC_EINVAL, "%s: L=%d (1 .. %d)", who, L, LCREC_MAX_LEVELS);
    if (n < 0) return fail(LCREC_EINVAL, "%s: n=%lld", who, (long long)n);
    if (!e_supported(e)) return fail(LCREC_EINVAL, "%s: e_dim=%d (supported: 16, 32, 64)", who, e);
    if (!beam_width_ok(width)) return fail(LCREC_EINVAL, "%s: width=%d (supported: 1, 2, 4, 8)", who, width);
    for (int l = 0; l < L; ++l)
        if (K[l] < 1) return fail(LCREC_EINVAL, "%s: K[%d]=%d", who, l, K[l]);
    if (int rc = first_null(who, {{z, "z"}, {codebooks, "codebooks"}, {tuples_out, "tuples_out"}, {score_out, "score_out"},
                                  {err_out, "err_out"}}))
        return rc;
    if (((uintptr_t)z | (uintptr_t)codebooks | (uintptr_t)resid_out | (uintptr_t)workspace) & 15)
        return fail(LCREC_EINVAL, "%s: z, codebooks, resid_out and workspace must be 16-byte aligned", who);
    if ((uintptr_t)tuples_out & 7) return fail(LCREC_EINVAL, "%s: tuples_out must be 8-byte aligned", who);
    if (((uintptr_t)score_out | (uintptr_t)err_out) & 3) return fail(LCREC_EINVAL, "%s: score_out and err_out must be 4-byte aligned", who);
    for (int l = 0; l < L; ++l)
        if (!rq_level_fits(K[l], e, L))
            return fail(LCREC_EUNSUPPORTED, "%s: level %d (K=%d, e=%d) does not fit in 160 KB of LDS (lcrec_rq_assign refuses it too)", who,
                        l, K[l], e);
    const size_t need = beam_workspace_bytes(n, e, L, width);
    if (need && (!workspace || workspace_bytes < need))
        return fail(LCREC_EWORKSPACE, "%s: workspace of %zu bytes, %zu needed (lcrec_rq_beam_workspace)", who,
                    workspace ? workspace_bytes : (size_t)0, need);
    if (n == 0) return LCREC_OK;

    TraceScope trace(K_RQ_BEAM, stream);
    const int items = BEAM_THREADS / width;
    const int64_t blocks = (n + items - 1) / items;
    const size_t half = beam_half_bytes(n, e, width);
    float *halves[2] = {static_cast<float *>(workspace),
                        reinterpret_cast<float *>(static_cast<char *>(workspace) + (L > 2 ? half : 0))};
    int *links = L > 1 ? reinterpret_cast<int *>(static_cast<char *>(workspace) + (size_t)(L == 2 ? 1 : 2) * half) : nullptr;
    int64_t cb_off = 0;
    int live = 1;
    for (int l = 0; l < L; ++l) {
        BeamParams p;
        p.r_in = l == 0 ? z : halves[(l - 1) & 1];
        p.in_stride = l == 0 ? (int64_t)e : (int64_t)width * e;
        p.r_out = l == L - 1 ? resid_out : halves[l & 1];
        p.cb = codebooks + cb_off;
        p.n = n;
        p.K = K[l]; p.L = L; p.l = l;
        p.P_in = live;
        live = (int64_t)live * K[l] < width ? live * K[l] : width;
        p.P_out = live;
        p.links = links;
        p.tuples = tuples_out; p.score = score_out; p.err = err_out;
        const size_t lds = level_lds_bytes(K[l], e);
        const int64_t resident = (int64_t)CUS * resident_per_cu(lds, BEAM_MAX_PER_CU);
        const unsigned grid = (unsigned)(blocks < resident ? blocks : resident);
        const int rc = with_e(e, [&](auto ec) {
            constexpr int E = decltype(ec)::value;
            auto go = [&](auto kernel) { return launch_with_lds(kernel, grid, BEAM_THREADS, lds, stream, who, "rq_beam_level_kernel", p); };
            switch (width) {
            case 1: return go(rq_beam_level_kernel<E, 1>);
            case 2: return go(rq_beam_level_kernel<E, 2>);
            case 4: return go(rq_beam_level_kernel<E, 4>);
            default: return go(rq_beam_level_kernel<E, 8>);
            }
        });
        if (rc) return rc;
        cb_off += (int64_t)K[l] * e;
    }
    return LCREC_OK;
}

}  // namespace lcrec
