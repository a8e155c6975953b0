// Index audit: GIVEN tuples walked through the residual quantiser (lcrec_rq_audit; opt-in, audit_indices / generate --audit).
//
// The finishing, extending and spilling passes -- and the reference's own Sinkhorn rounds -- give some items a code that is not
// their nearest one.  This pass says what that cost, item by item and level by level: the distance of the held code, the best
// distance, and how many codes rank before the held one.  Beyond the reference, which only prints a collision rate.
//
// The rule (include/lcrec.h, lcrec_rq_audit, is the contract; tests/audit_ref.py restates it in numpy).  r_0 = z_i; per level l:
//   d_l(k)  = (xx + cc_k) - 2*dot_k, xx / cc / dot each one fp32 fma chain over the dimension ascending -- rq_assign.hip's and
//             finish.hip's bits, oracle/lcrec_oracle.c's lcrec_oracle_distances.  A NaN counts as +inf and is reported as +inf.
//   h       = the held code brought into [0, K_l) by lcrec_rq_apply_level's rule on the int64 value; clamped: flag bit l
//   d_held  = d_l(h);  best = first minimum of d_l in code order;  d_best = d_l(best)
//   rank    = #{k : d_l(k) < d_l(h)} + #{k < h : d_l(k) == d_l(h)}
//   r_{l+1} = the residual behind the HELD code, rq_assign's three operations: t = c - r; s = r + t; r' = r - s
// and err = the fma chain of r_L[j]^2.
//
// Shape: one launch per level, one item per lane.  The level's codebook (row stride E + 4 floats: rows stay 16-byte aligned for
// ds_read_b128 and consecutive rows start 4 banks apart) and its cc go to LDS once per workgroup; the lane holds its residual in E
// registers.  It first evaluates d(h) on its own held row -- one gathered row per item, the only read in which the lanes of a wave
// differ -- then sweeps k = 0 .. K-1 once: all 64 lanes read the same row at the same time, which LDS serves as a broadcast, and
// the lane keeps the first minimum and counts its rank.  Nothing crosses lanes: no shuffle, no atomic, no barrier after the
// staging.  The grid is the number of workgroups resident at once (256 CUs x what the level's LDS allows, at most 8); a grid-stride
// loop over blocks of 256 items does the rest, so a file of production size makes several trips.  Between the levels the residual
// lives in the workspace, each lane reading and rewriting its own row.
#include "common.h"

namespace lcrec {

constexpr int AUD_THREADS = 256;
constexpr int AUD_CUS = 256;          // the grid covers the workgroups that can be resident at once; the rest is the item loop
constexpr int AUD_MAX_PER_CU = 8;     // the register bound at e = 16 / 32 (63 / 62 VGPRs; 4 at e = 64, where a level
                                      // above 148 codes allows fewer anyway); the staged level's LDS usually allows fewer
constexpr size_t AUD_LDS_PER_CU = 160 * 1024;

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
__device__ __forceinline__ float audit_distance(const float (&x)[E], float xx, const float *crow, float cc)
{
    const f32x4 *c4 = reinterpret_cast<const f32x4 *>(crow);
    float dot = 0.f;
#pragma unroll
    for (int q = 0; q < E / 4; ++q) {
        const f32x4 c = c4[q];
        dot = __builtin_fmaf(x[4 * q], c[0], dot);
        dot = __builtin_fmaf(x[4 * q + 1], c[1], dot);
        dot = __builtin_fmaf(x[4 * q + 2], c[2], dot);
        dot = __builtin_fmaf(x[4 * q + 3], c[3], dot);
    }
    const float t = xx + cc;
    const float d = t - 2.0f * dot;
    return d == d ? d : __builtin_inff();   // a NaN counts as +inf
}

template <int E>
__global__ __launch_bounds__(AUD_THREADS) void rq_audit_level_kernel(AuditParams p)
{
    constexpr int S = E + 4;   // LDS row stride (floats)
    extern __shared__ __attribute__((aligned(16))) unsigned char aud_smem[];
    const int K = p.K;
    float *cbs = reinterpret_cast<float *>(aud_smem);   // [K][S]
    float *ccs = cbs + (size_t)K * S;                   // [K]
    const int tid = threadIdx.x;

    for (int q = tid; q < K * (E / 4); q += AUD_THREADS) {
        const int row = q / (E / 4), g = q % (E / 4);
        *reinterpret_cast<f32x4 *>(cbs + row * S + 4 * g) = *reinterpret_cast<const f32x4 *>(p.cb + (size_t)row * E + 4 * g);
    }
    __syncthreads();
    for (int k = tid; k < K; k += AUD_THREADS) {
        const float *cr = cbs + k * S;
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < E; ++j) a = __builtin_fmaf(cr[j], cr[j], a);
        ccs[k] = a;
    }
    __syncthreads();

    const int L = p.L, l = p.l;
    for (int64_t base = (int64_t)blockIdx.x * AUD_THREADS; base < p.n; base += (int64_t)gridDim.x * AUD_THREADS) {
        const int64_t i = base + tid;
        if (i >= p.n) continue;                          // tail lanes of the last block (no barrier follows)
        float x[E];
        {
            const f32x4 *s = reinterpret_cast<const f32x4 *>(p.r_in + i * E);
#pragma unroll
            for (int q = 0; q < E / 4; ++q) {
                const f32x4 v = s[q];
                x[4 * q] = v[0]; x[4 * q + 1] = v[1]; x[4 * q + 2] = v[2]; x[4 * q + 3] = v[3];
            }
        }
        float xx = 0.f;
#pragma unroll
        for (int j = 0; j < E; ++j) xx = __builtin_fmaf(x[j], x[j], xx);

        const int64_t held = p.idx[i * p.idx_stride];
        const int h = (int)(held < 0 ? 0 : (held >= K ? K - 1 : held));
        const uint32_t clamped = (held < 0 || held >= K) ? (1u << l) : 0u;
        const float *hrow = cbs + h * S;
        const float dh = audit_distance<E>(x, xx, hrow, ccs[h]);

        float best = __builtin_inff();
        int bk = 0, rank = 0;
        for (int k = 0; k < K; ++k) {
            const float d = audit_distance<E>(x, xx, cbs + k * S, ccs[k]);
            if (d < best) { best = d; bk = k; }
            rank += (d < dh || (d == dh && k < h)) ? 1 : 0;
        }
        const int64_t o = i * L + l;
        p.d_held[o] = dh;
        p.d_best[o] = best;
        p.rank[o] = rank;
        if (p.best) p.best[o] = (int64_t)bk;
        p.flags[i] = l == 0 ? clamped : (p.flags[i] | clamped);

        // the residual behind the held code: t = c - r; s = r + t; r' = r - s
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const float t = hrow[j] - x[j];
            const float s = x[j] + t;
            x[j] = x[j] - s;
        }
        if (p.r_out) {
            f32x4 *dst = reinterpret_cast<f32x4 *>(p.r_out + i * E);
#pragma unroll
            for (int q = 0; q < E / 4; ++q) {
                f32x4 v;
                v[0] = x[4 * q]; v[1] = x[4 * q + 1]; v[2] = x[4 * q + 2]; v[3] = x[4 * q + 3];
                dst[q] = v;
            }
        }
        if (l == L - 1) {
            float a = 0.f;
#pragma unroll
            for (int j = 0; j < E; ++j) a = __builtin_fmaf(x[j], x[j], a);
            p.err[i] = a;
        }
    }
}

// include/lcrec.h states this formula
static size_t audit_lds_bytes(int K, int e) { return (size_t)K * ((size_t)(e + 4) * 4 + 4); }

// workgroups of a level that one CU holds at a time: what its LDS allows, at most the register bound
static int audit_per_cu(size_t lds)
{
    const size_t fit = AUD_LDS_PER_CU / (lds ? lds : 1);
    return fit < 1 ? 1 : (fit > (size_t)AUD_MAX_PER_CU ? AUD_MAX_PER_CU : (int)fit);
}

// the residual between the levels; a one-level call needs none
static size_t audit_workspace_bytes(int64_t n, int e, int L) { return L > 1 && n > 0 ? align_up((size_t)n * e * sizeof(float), 256) : 0; }

size_t rq_audit_workspace(int64_t n, int e, const int *K, int L)
{
    if (!K || n < 0 || L < 1 || L > LCREC_MAX_LEVELS || (e != 16 && e != 32 && e != 64)) return 0;
    return audit_workspace_bytes(n, e, L);
}

template <int E>
static int audit_launch(const AuditParams &p, int grid, size_t lds, hipStream_t stream)
{
    auto kern = rq_audit_level_kernel<E>;
    hipError_t he = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (he != hipSuccess) return fail(LCREC_EHIP, "rq_audit: hipFuncSetAttribute(%zu B LDS): %s", lds, hipGetErrorString(he));
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(AUD_THREADS), lds, stream, p);
    return check_launch("rq_audit_level_kernel");
}

int rq_audit(const float *z, int64_t n, int e, const float *codebooks, const int *K, int L, const int64_t *idx, int64_t idx_stride,
             float *d_held_out, float *d_best_out, int *rank_out, int64_t *best_out, float *err_out, float *resid_out,
             uint32_t *flags_out, void *workspace, size_t workspace_bytes, hipStream_t stream)
{
    const char *who = "rq_audit";
    if (!K) return fail(LCREC_EINVAL, "%s: K is NULL", who);
    if (L < 1 || L > LCREC_MAX_LEVELS) return fail(LCREC_EINVAL, "%s: L=%d (1 .. %d)", who, L, LCREC_MAX_LEVELS);
    if (n < 0) return fail(LCREC_EINVAL, "%s: n=%lld", who, (long long)n);
    if (e != 16 && e != 32 && e != 64) return fail(LCREC_EINVAL, "%s: e_dim=%d (supported: 16, 32, 64)", who, e);
    for (int l = 0; l < L; ++l)
        if (K[l] < 1) return fail(LCREC_EINVAL, "%s: K[%d]=%d", who, l, K[l]);
    if (idx_stride == 0) idx_stride = L;
    if (idx_stride < L) return fail(LCREC_EINVAL, "%s: idx_stride=%lld < L=%d", who, (long long)idx_stride, L);
    const struct { const void *ptr; const char *name; } required[] = {
        {z, "z"}, {codebooks, "codebooks"}, {idx, "idx"}, {d_held_out, "d_held_out"}, {d_best_out, "d_best_out"},
        {rank_out, "rank_out"}, {err_out, "err_out"}, {flags_out, "flags_out"}};
    for (const auto &r : required)
        if (!r.ptr) return fail(LCREC_EINVAL, "%s: %s is NULL", who, r.name);
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
        const size_t lds = audit_lds_bytes(K[l], e);
        const int64_t resident = (int64_t)AUD_CUS * audit_per_cu(lds);   // LDS sets it for all but the smallest levels: 256 codes at e = 32: 4
        const int grid = (int)(blocks < resident ? blocks : resident);
        int rc;
        if (e == 16) rc = audit_launch<16>(p, grid, lds, stream);
        else if (e == 32) rc = audit_launch<32>(p, grid, lds, stream);
        else rc = audit_launch<64>(p, grid, lds, stream);
        if (rc) return rc;
        cb_off += (int64_t)K[l] * e;
    }
    return LCREC_OK;
}

}  // namespace lcrec
