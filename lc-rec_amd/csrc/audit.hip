// Index audit: GIVEN tuples walked through the residual quantiser (lcrec_rq_audit; opt-in, audit_indices / generate --audit).
//
// The finishing, extending and spilling passes -- and the reference's own Sinkhorn rounds -- give some items a code that is not
// their nearest one.  This pass says what that cost, item by item and level by level: the distance of the held code, the best
// distance, and how many codes rank before the held one.  Beyond the reference, which only prints a collision rate.
//
// The rule: rq_walk.h states the quantiser's arithmetic; include/lcrec.h, lcrec_rq_audit, is this pass's contract and
// tests/audit_ref.py restates it in numpy.  r_0 = z_i; per level l, with d_l(k) the distance of code k, a NaN reported as +inf:
//   h       = the held code brought into [0, K_l) by lcrec_rq_apply_level's rule on the int64 value; clamped: flag bit l
//   d_held  = d_l(h);  best = first minimum of d_l in code order;  d_best = d_l(best)
//   rank    = #{k : d_l(k) < d_l(h)} + #{k < h : d_l(k) == d_l(h)}
//   r_{l+1} = the residual behind the HELD code
// and err = the chain of squares of r_L.
//
// Shape: one launch per level, one item per lane.  The level's codebook (row stride E + 4 floats: rows stay 16-byte aligned for
// ds_read_b128 and consecutive rows start 4 banks apart) and its cc go to LDS once per workgroup; the lane holds its residual in E
// registers.  It first evaluates d(h) on its own held row -- one gathered row per item, the only read in which the lanes of a wave
// differ -- then sweeps k = 0 .. K-1 once: all 64 lanes read the same row at the same time, which LDS serves as a broadcast, and
// the lane keeps the first minimum and counts its rank.  Nothing crosses lanes: no shuffle, no atomic, no barrier after the
// staging.  The grid is the number of workgroups resident at once (256 CUs x what the level's LDS allows, at most 8); a grid-stride
// loop over blocks of 256 items does the rest, so a file of production size makes several trips.  Between the levels the residual
// lives in the workspace, each lane reading and rewriting its own row.
#include "rq_walk.h"

namespace lcrec {

constexpr int AUD_THREADS = 256;
constexpr int AUD_MAX_PER_CU = 8;     // the register bound at e = 16 / 32 (63 / 62 VGPRs; 4 at e = 64, where a level
                                      // above 148 codes allows fewer anyway); the staged level's LDS usually allows fewer

struct AuditParams {
    const float *r_in;       // [n][E] residual entering the level (level 0: the latents)
    float *r_out;            // [n][E] residual behind the held code, or NULL; may be r_in (a lane rewrites the row it read)
    const float *cb;         // [K][E] this level's rows
    const int64_t *idx;      // held code of item i at idx[i * idx_stride] (already offset to this level's column)
    int64_t idx_stride;
    int64_t n;
    int K, L, l;
    float *d_held, *d_best;  // [n][L]
    int *rank;               // [n][L]
    int64_t *best;           // [n][L] or NULL
    float *err;              // [n], written by the last level
    uint32_t *flags;         // [n], written by level 0, or-ed into by the later ones
};

template <int E>
__global__ __launch_bounds__(AUD_THREADS) void rq_audit_level_kernel(AuditParams p)
{
    constexpr int S = E + 4;   // LDS row stride (floats)
    extern __shared__ __attribute__((aligned(16))) unsigned char aud_smem[];
    const int K = p.K;
    float *cbs = reinterpret_cast<float *>(aud_smem);   // [K][S]
    float *ccs = cbs + (size_t)K * S;                   // [K]
    const int tid = threadIdx.x;

    stage_level<E, S, AUD_THREADS>(p.cb, K, cbs, ccs);

    const int L = p.L, l = p.l;
    for (int64_t base = (int64_t)blockIdx.x * AUD_THREADS; base < p.n; base += (int64_t)gridDim.x * AUD_THREADS) {
        const int64_t i = base + tid;
        if (i >= p.n) continue;                          // tail lanes of the last block (no barrier follows)
        float x[E];
        load_row<E>(p.r_in + i * E, x);
        const float xx = sq_chain<E>(x);

        const int64_t held = p.idx[i * p.idx_stride];
        const int h = (int)(held < 0 ? 0 : (held >= K ? K - 1 : held));
        const uint32_t clamped = (held < 0 || held >= K) ? (1u << l) : 0u;
        const float *hrow = cbs + h * S;
        const float dh = nan_as_inf(code_distance<E, f32x4>(x, xx, hrow, ccs[h]));

        float best = __builtin_inff();
        int bk = 0, rank = 0;
        for (int k = 0; k < K; ++k) {
            const float d = nan_as_inf(code_distance<E, f32x4>(x, xx, cbs + k * S, ccs[k]));
            if (d < best) { best = d; bk = k; }
            rank += (d < dh || (d == dh && k < h)) ? 1 : 0;
        }
        const int64_t o = i * L + l;
        p.d_held[o] = dh;
        p.d_best[o] = best;
        p.rank[o] = rank;
        if (p.best) p.best[o] = (int64_t)bk;
        p.flags[i] = l == 0 ? clamped : (p.flags[i] | clamped);

        residual_behind<E>(x, hrow);
        if (p.r_out) store_row<E>(p.r_out + i * E, x);
        if (l == L - 1) p.err[i] = sq_chain<E>(x);
    }
}

// the residual between the levels; a one-level call needs none
static size_t audit_workspace_bytes(int64_t n, int e, int L) { return L > 1 && n > 0 ? align_up((size_t)n * e * sizeof(float), 256) : 0; }

size_t rq_audit_workspace(int64_t n, int e, const int *K, int L)
{
    if (!K || n < 0 || L < 1 || L > LCREC_MAX_LEVELS || !e_supported(e)) return 0;
    return audit_workspace_bytes(n, e, L);
}

int rq_audit(const float *z, int64_t n, int e, const float *codebooks, const int *K, int L, const int64_t *idx, int64_t idx_stride,
             float *d_held_out, float *d_best_out, int *rank_out, int64_t *best_out, float *err_out, float *resid_out,
             uint32_t *flags_out, void *workspace, size_t workspace_bytes, hipStream_t stream)
{
    const char *who = "rq_audit";
    if (!K) return fail(LCREC_EINVAL, "%s: K is NULL", who);
    if (L < 1 || L > LCREC_MAX_LEVELS) return fail(LCREC_EINVAL, "%s: L=%d (1 .. %d)", who, L, LCREC_MAX_LEVELS);
    if (n < 0) return fail(LCREC_EINVAL, "%s: n=%lld", who, (long long)n);
    if (!e_supported(e)) return fail(LCREC_EINVAL, "%s: e_dim=%d (supported: 16, 32, 64)", who, e);
    for (int l = 0; l < L; ++l)
        if (K[l] < 1) return fail(LCREC_EINVAL, "%s: K[%d]=%d", who, l, K[l]);
    if (idx_stride == 0) idx_stride = L;
    if (idx_stride < L) return fail(LCREC_EINVAL, "%s: idx_stride=%lld < L=%d", who, (long long)idx_stride, L);
    if (int rc = first_null(who, {{z, "z"}, {codebooks, "codebooks"}, {idx, "idx"}, {d_held_out, "d_held_out"},
                                  {d_best_out, "d_best_out"}, {rank_out, "rank_out"}, {err_out, "err_out"}, {flags_out, "flags_out"}}))
        return rc;
    if (((uintptr_t)z | (uintptr_t)codebooks | (uintptr_t)d_held_out | (uintptr_t)d_best_out | (uintptr_t)err_out |
         (uintptr_t)resid_out | (uintptr_t)workspace) & 15)
        return fail(LCREC_EINVAL, "%s: z, codebooks, d_held_out, d_best_out, err_out, resid_out and workspace must be 16-byte aligned", who);
    if (((uintptr_t)idx | (uintptr_t)best_out) & 7) return fail(LCREC_EINVAL, "%s: idx and best_out must be 8-byte aligned", who);
    if (((uintptr_t)rank_out | (uintptr_t)flags_out) & 3) return fail(LCREC_EINVAL, "%s: rank_out and flags_out must be 4-byte aligned", who);
    for (int l = 0; l < L; ++l)
        if (!rq_level_fits(K[l], e, L))
            return fail(LCREC_EUNSUPPORTED, "%s: level %d (K=%d, e=%d) does not fit in 160 KB of LDS (lcrec_rq_assign refuses it too)", who,
                        l, K[l], e);
    const size_t need = audit_workspace_bytes(n, e, L);
    if (need && (!workspace || workspace_bytes < need))
        return fail(LCREC_EWORKSPACE, "%s: workspace of %zu bytes, %zu needed (lcrec_rq_audit_workspace)", who,
                    workspace ? workspace_bytes : (size_t)0, need);
    if (n == 0) return LCREC_OK;

    TraceScope trace(K_RQ_AUDIT, stream);
    const int64_t blocks = (n + AUD_THREADS - 1) / AUD_THREADS;
    float *between = static_cast<float *>(workspace);
    int64_t cb_off = 0;
    for (int l = 0; l < L; ++l) {
        AuditParams p;
        p.r_in = l == 0 ? z : between;
        p.r_out = l == L - 1 ? resid_out : between;
        p.cb = codebooks + cb_off;
        p.idx = idx + l;
        p.idx_stride = idx_stride;
        p.n = n;
        p.K = K[l]; p.L = L; p.l = l;
        p.d_held = d_held_out; p.d_best = d_best_out; p.rank = rank_out; p.best = best_out;
        p.err = err_out; p.flags = flags_out;
        const size_t lds = level_lds_bytes(K[l], e);
        const int64_t resident = (int64_t)CUS * resident_per_cu(lds, AUD_MAX_PER_CU);   // LDS sets it for all but the smallest levels: 256 codes at e = 32: 4
        const unsigned grid = (unsigned)(blocks < resident ? blocks : resident);
        const int rc = with_e(e, [&](auto ec) {
            return launch_with_lds(rq_audit_level_kernel<decltype(ec)::value>, grid, AUD_THREADS, lds, stream, who, "rq_audit_level_kernel", p);
        });
        if (rc) return rc;
        cb_off += (int64_t)K[l] * e;
    }
    return LCREC_OK;
}

}  // namespace lcrec
