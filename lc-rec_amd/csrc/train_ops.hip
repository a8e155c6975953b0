// The element-wise / column-reduction half of a training step, for gfx950 -- what the reference leaves to a dozen
// aten kernels per layer ("full training step on device"):
//
//   bn_relu_forward    training-mode BatchNorm1d (+ ReLU) after a Linear: index/models/layers.py:25-30
//   bn_relu_backward   its backward (autograd of the above under loss.backward(), index/trainer.py:117), incl. the
//                      gradient of the Linear's bias
//   relu_bias_backward ReLU mask + bias gradient of a Linear without BatchNorm (layers.py:23,28-30)
//   recon_loss_grad    mse / l1 reconstruction loss and its gradient (index/models/rqvae.py:74-85)
//   grad_norm_clip     global L2 norm of all gradients + clip coefficient (clip_grad_norm_(.., 1.0), trainer.py:118)
//   adamw_step         clipped AdamW / Adam update with the warm-up schedule evaluated on the device
//                      (trainer.py:49-92,119-120)
//   sgd_step, adagrad_step, rmsprop_step
//                      the same for the reference's other learners (trainer.py:49-81)
//
// All of it is HBM/L2-bound streaming over [batch][features] or over the flat parameter buffer; no MFMA.  Column
// reductions (BatchNorm statistics, bias gradients) are done by one 1024-thread workgroup per strip of 8-32 columns
// (see Strip below): deterministic, no atomics.  Batch-sized inputs only (a training batch is 1-8 k rows; the strip is
// re-read from L2 for the later passes).  First form (256 threads, one load in flight per lane): 64 us per call at
// 1024 x 2048 -- a third of the training step; 16 waves with 8 loads in flight each: see profiles/.
#include "common.h"

#include <stdlib.h>
#include <stdint.h>
#include <initializer_list>

namespace lcrec {

constexpr int CR_THREADS = 1024;  // 16 waves per strip: enough loads in flight to cover HBM/L2 latency from one CU
constexpr int CR_WAVES = CR_THREADS / 64;
#ifndef LCREC_CR_UNROLL
#define LCREC_CR_UNROLL 8
#endif
constexpr int CR_UNROLL = LCREC_CR_UNROLL;

// Strips are narrower than a 128-byte line (32 floats), so neighbours share lines -- and consecutive workgroups go to different
// XCDs (round-robin over 8), each with an L2 of its own that would fetch the shared line again.  When the grid is a multiple
// of 8, workgroup b takes strip (b % 8) * (grid / 8) + b / 8: the strips of one XCD are neighbours (measured on the float4
// form below: backward of 1024 x 2048 in 16-column strips 13.3 -> 8.0 us).  The dword and the float4 strips share it.
template <int COLS>
__device__ __forceinline__ int strip_of_block()
{
    const int b = blockIdx.x, g = gridDim.x;
    return (COLS < 32 && (g & 7) == 0) ? (b & 7) * (g >> 3) + (b >> 3) : b;
}

// Strip geometry: COLS columns x RGS = 1024 / COLS row groups; lane l of a wave holds column l % COLS, so a wave spans
// 64 / COLS consecutive row groups.  Row group g owns rows g, g + RGS, ... (each lane adds its rows in ascending order,
// CR_UNROLL loads in flight); the groups of a wave are added by xor-shuffles (a fixed tree), the 16 waves through LDS in
// wave order -- the same bits on every run.
template <int COLS>
struct Strip {
    static constexpr int RGS = CR_THREADS / COLS;
    int c, rg, col;
    bool live;
    __device__ Strip(int F) : c(threadIdx.x % COLS), rg(threadIdx.x / COLS), col(strip_of_block<COLS>() * COLS + threadIdx.x % COLS), live(col < F) {}

    // f(row) -> value; returns the sum over this lane's rows in ascending row order
    template <typename Fn>
    __device__ __forceinline__ float rows(int64_t n, Fn f) const
    {
        float s = 0.f;
        int64_t r = rg;
        for (; r + (int64_t)(CR_UNROLL - 1) * RGS < n; r += (int64_t)CR_UNROLL * RGS) {
            float v[CR_UNROLL];
#pragma unroll
            for (int u = 0; u < CR_UNROLL; ++u) v[u] = f(r + (int64_t)u * RGS);
#pragma unroll
            for (int u = 0; u < CR_UNROLL; ++u) s += v[u];
        }
        for (; r < n; r += RGS) s += f(r);
        return s;
    }

    // the same walk with two running sums: f(row, a, b) adds the row's contribution to both
    template <typename Fn>
    __device__ __forceinline__ void rows2(int64_t n, float &s0, float &s1, Fn f) const
    {
        s0 = 0.f;
        s1 = 0.f;
        int64_t r = rg;
        for (; r + (int64_t)(CR_UNROLL - 1) * RGS < n; r += (int64_t)CR_UNROLL * RGS) {
            float v0[CR_UNROLL], v1[CR_UNROLL];
#pragma unroll
            for (int u = 0; u < CR_UNROLL; ++u) f(r + (int64_t)u * RGS, v0[u], v1[u]);
#pragma unroll
            for (int u = 0; u < CR_UNROLL; ++u) { s0 += v0[u]; s1 += v1[u]; }
        }
        for (; r < n; r += RGS) {
            float a, b;
            f(r, a, b);
            s0 += a;
            s1 += b;
        }
    }

    // sum of one value per lane over all row groups of the lane's column; valid in every lane
    __device__ __forceinline__ float sum(float v, float (*sm)[COLS]) const
    {
#pragma unroll
        for (int o = COLS; o < 64; o <<= 1) v += __shfl_xor(v, o, 64);
        __syncthreads();                       // previous use of sm is over
        if ((threadIdx.x & 63) < COLS) sm[threadIdx.x >> 6][c] = v;
        __syncthreads();
        float s = sm[0][c];
#pragma unroll
        for (int w = 1; w < CR_WAVES; ++w) s += sm[w][c];
        return s;
    }
};

// Training-mode BatchNorm1d (+ReLU).  torch semantics: batch mean, biased variance for the normalisation,
// running_mean/var updated with `momentum` (running_var from the unbiased variance), eps inside the square root.
// STATS: only the local statistics of a rank's rows (lcrec_bn_stats: mean -> mean_out, M2 = sum (t - mean)^2 -> rstd_out, to be
// merged over ranks, Chan et al.), nothing applied.
// CACHED (n <= CR_MAXR rows per lane, not with STATS): the lane's rows stay in registers between the statistics pass and the
// apply pass -- t is read from memory once.  Same sums in the same order as the two-pass form, hence the same bits.
constexpr int CR_MAXR = 32;

template <int COLS, bool STATS = false, bool CACHED = false>
__global__ __launch_bounds__(CR_THREADS) void bn_relu_forward_kernel(const float *__restrict__ t, int64_t n, int F,
                                                                      const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                      float eps, float momentum, float *running_mean,
                                                                      float *running_var, float *__restrict__ y, float *mean_out,
                                                                      float *rstd_out, int relu)
{
    __shared__ float sm[CR_WAVES][COLS];
    constexpr int RGS = Strip<COLS>::RGS;
    const Strip<COLS> st(F);
    const int col = st.live ? st.col : 0;          // dead lanes read column 0 and write nothing
    const float inv_n = 1.0f / (float)n;
    const float *tc = t + col;
    // one statistics pass: sums of (t - pivot) and (t - pivot)^2 with pivot = the column's first row, a sample of the
    // column -- so |mean - pivot| is of the order of the standard deviation and m2 = s2 - s1^2/n loses a bit or two, not
    // the digits the textbook E[t^2] - mean^2 loses when |mean| >> std
    const float pivot = tc[0];
    float tv[CACHED ? CR_MAXR : 1];
    float s1 = 0.f, s2 = 0.f;
    if (CACHED) {
#pragma unroll
        for (int u = 0; u < CR_MAXR; ++u) {
            const int64_t r = st.rg + (int64_t)u * RGS;
            tv[u] = r < n ? tc[r * F] : pivot;
        }
#pragma unroll
        for (int u = 0; u < CR_MAXR; ++u) {
            const float d = tv[u] - pivot;
            if (st.rg + (int64_t)u * RGS < n) { s1 += d; s2 += d * d; }
        }
    } else {
        st.rows2(n, s1, s2, [&](int64_t r, float &a, float &b) { const float d = tc[r * F] - pivot; a = d; b = d * d; });
    }
    s1 = st.sum(s1, sm);
    s2 = st.sum(s2, sm);
    const float dmean = STATS ? s1 / (float)n : s1 * inv_n;        // (the statistics form divides; its bits are in the exchange rows)
    const float mean = pivot + dmean;
    float m2 = s2 - s1 * dmean;
    m2 = m2 > 0.f ? m2 : 0.f;
    if (STATS) {
        if (st.live && st.rg == 0) { mean_out[col] = mean; rstd_out[col] = m2; }
        return;
    }
    const float var = m2 * inv_n;
    const float rstd = 1.0f / __builtin_sqrtf(var + eps);
    if (!st.live) return;
    const float g = gamma ? gamma[col] : 1.0f, b = beta ? beta[col] : 0.0f;
    float *yc = y + col;
    if (CACHED) {
#pragma unroll
        for (int u = 0; u < CR_MAXR; ++u) {
            const int64_t r = st.rg + (int64_t)u * RGS;
            if (r < n) {
                float v = (tv[u] - mean) * rstd * g + b;
                if (relu) v = v > 0.f ? v : 0.f;
                yc[r * F] = v;
            }
        }
    } else {
#pragma unroll 4
        for (int64_t r = st.rg; r < n; r += RGS) {
            float v = (tc[r * F] - mean) * rstd * g + b;
            if (relu) v = v > 0.f ? v : 0.f;
            yc[r * F] = v;
        }
    }
    if (st.rg == 0) {
        mean_out[col] = mean;
        rstd_out[col] = rstd;
        if (running_mean) running_mean[col] = (1.0f - momentum) * running_mean[col] + momentum * mean;
        if (running_var) {
            const float unbiased = n > 1 ? m2 / (float)(n - 1) : var;
            running_var[col] = (1.0f - momentum) * running_var[col] + momentum * unbiased;
        }
    }
}

// Backward of y = [relu](bn(t)) for gy = dL/dy:
//   g = gy * [y > 0];  dbeta = sum g;  dgamma = sum g * xhat;  dt = gamma * rstd * (g - dbeta/n - xhat * dgamma/n)
// and the gradient of the Linear bias that produced t: dbias = sum dt (zero up to rounding, as in autograd).
struct BnBwd {
    const float *gy, *t, *y;
    int64_t n;
    int F;
    const float *gamma, *mean, *rstd;
    int relu;
    float *dt, *dgamma, *dbeta, *dbias;
    const float *fold_scale, *fold_shift;
    float *sum_g, *sum_gx;      // MODE 1: out, this rank's column sums of g and g * xhat; MODE 2: in, the sums over all ranks
    float n_total;              // MODE 2: rows of the global batch
};
// MODE 0: the whole backward of one process.  The data-parallel split (SyncBatchNorm semantics: the batch is the union of the
// ranks' rows, xhat from the GLOBAL statistics; lcrec_amd/layers.py all-reduces between the halves): MODE 1 =
// lcrec_bn_backward_reduce (the two column sums of this rank's rows, nothing written to dt), MODE 2 = lcrec_bn_backward_apply (dt
// and dbias from the global sums).  The halves take the ReLU mask from y alone (their host entries pass no fold).
// CACHED (MODE 0 only): the lane's masked gradients and xhat stay in registers, as in the forward.
template <int COLS, int MODE = 0, bool CACHED = false>
__global__ __launch_bounds__(CR_THREADS) void bn_relu_backward_kernel(BnBwd p)
{
    __shared__ float sm[CR_WAVES][COLS];
    constexpr int RGS = Strip<COLS>::RGS;
    const float *gy = p.gy, *__restrict__ t = p.t, *__restrict__ y = p.y;
    const int64_t n = p.n;
    const int F = p.F, relu = p.relu;
    const Strip<COLS> st(F);
    const int col = st.live ? st.col : 0;
    const float mu = p.mean[col], rs = p.rstd[col], gm = p.gamma ? p.gamma[col] : 1.0f;
    const float *gc = gy + col, *tc = t + col, *yc = (relu && y) ? y + col : nullptr;
    // the ReLU mask from the stored activation y, or -- when the forward never wrote one (lcrec_linear_bn_forward hands t to the
    // next layer, which applies max(t * scale + shift, 0) itself) -- from the same fused expression the consumer evaluated; or,
    // with fold_shift alone (= beta), from lcrec_bn_relu_forward's own expression (t - mean) * rstd * gamma + beta: the bits of
    // the y it wrote, without reading it
    const bool from_beta = relu && !y && !p.fold_scale;
    const float fs = (relu && !y && p.fold_scale) ? p.fold_scale[col] : 0.f, fh = (relu && !y) ? p.fold_shift[col] : 0.f;
    auto gval = [&](int64_t r) {
        float g = gc[r * F];
        if (relu) {
            const bool on = yc ? yc[r * F] > 0.f
                               : (from_beta ? (tc[r * F] - mu) * rs * gm + fh > 0.f : __builtin_fmaf(tc[r * F], fs, fh) > 0.f);
            if (!on) g = 0.f;
        }
        return g;
    };
    float gv[CACHED ? CR_MAXR : 1], xv[CACHED ? CR_MAXR : 1];
    float db = 0.f, dg = 0.f;
    if (MODE == 2) {
        db = p.sum_g[col];
        dg = p.sum_gx[col];
    } else if (CACHED) {
#pragma unroll
        for (int u = 0; u < CR_MAXR; ++u) {
            const int64_t r = st.rg + (int64_t)u * RGS;
            const bool in = r < n;
            gv[u] = in ? gval(r) : 0.f;
            xv[u] = in ? (tc[r * F] - mu) * rs : 0.f;
        }
#pragma unroll
        for (int u = 0; u < CR_MAXR; ++u)
            if (st.rg + (int64_t)u * RGS < n) { db += gv[u]; dg += gv[u] * xv[u]; }
        db = st.sum(db, sm);
        dg = st.sum(dg, sm);
    } else {
        st.rows2(n, db, dg, [&](int64_t r, float &a, float &b) { const float g = gval(r); a = g; b = g * ((tc[r * F] - mu) * rs); });
        db = st.sum(db, sm);
        dg = st.sum(dg, sm);
    }
    if (MODE == 1) {
        if (st.live && st.rg == 0) {
            p.sum_g[col] = db;
            p.sum_gx[col] = dg;
            if (p.dbeta) p.dbeta[col] = db;          // this rank's share of the parameter gradients (the gradient all-reduce sums them)
            if (p.dgamma) p.dgamma[col] = dg;
        }
        return;
    }
    const float inv_n = 1.0f / (MODE == 2 ? p.n_total : (float)n);
    const float k = gm * rs, mdb = db * inv_n, mdg = dg * inv_n;
    float *dc = p.dt + col;
    float sdt = 0.f;
    if (st.live && CACHED) {
#pragma unroll
        for (int u = 0; u < CR_MAXR; ++u) {
            const int64_t r = st.rg + (int64_t)u * RGS;
            if (r < n) {
                const float v = k * (gv[u] - mdb - xv[u] * mdg);
                dc[r * F] = v;
                sdt += v;
            }
        }
    } else if (st.live) {
#pragma unroll 4
        for (int64_t r = st.rg; r < n; r += RGS) {
            const float xh = (tc[r * F] - mu) * rs;
            const float v = k * (gval(r) - mdb - xh * mdg);
            dc[r * F] = v;
            sdt += v;
        }
    }
    const float dbs = st.sum(sdt, sm);
    if (st.live && st.rg == 0) {
        if (MODE == 0 && p.dgamma) p.dgamma[col] = dg;
        if (MODE == 0 && p.dbeta) p.dbeta[col] = db;
        if (p.dbias) p.dbias[col] = dbs;
    }
}

// ---- the two kernels again for the shapes a training step has: F a multiple of 4, rows 16-byte aligned, and few enough rows
// that a lane's share of the strip stays in registers (n <= RMAX * RGS).  Lanes read float4s: a strip of COLS columns is COLS / 4
// lanes wide and RGS = 1024 / (COLS / 4) row groups deep, so a 1024 x 16 strip is FOUR 16-byte loads per lane and array, all in
// flight at once, where the dword form above issues 16 per lane -- on one CU the dword form is bound by the texture-address
// rate (13 us for a 1024 x 16 backward strip however few strips the launch has; r03 kernel trace by grid size).
// Row order of the sums (fixed, so the same bits on every run): a lane's rows ascending; the row groups of a 16-lane row by DPP
// rotations; the workgroup's 64 such rows as four chains of 16 in row order, ((c0 + c1) + (c2 + c3)) -- see sum() below.
template <int COLS>
struct Strip4 {
    static constexpr int L4 = COLS / 4, RGS = CR_THREADS / L4;
    int c4, rg, col;
    bool live;
    __device__ Strip4(int F) : c4(threadIdx.x % L4), rg(threadIdx.x / L4), col(strip_of_block<COLS>() * COLS + 4 * (threadIdx.x % L4)), live(col < F) {}

    // v + (v rotated right by N lanes within its row of 16 lanes): one v_add_f32 with a DPP operand, no LDS crossbar
    template <int N>
    static __device__ __forceinline__ float add_ror(float v)
    {
        return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x120 + N, 0xf, 0xf, false));
    }

    // sums over all row groups of NV four-column values per lane; valid in every lane afterwards.
    //  1. inside a row of 16 lanes (16 / L4 row groups): DPP rotations, so lane c4 of the row ends with the row's sum of its
    //     columns (each lane adds in its own rotated order; only lanes c4 < L4 of each row are used, a fixed order);
    //  2. the 64 row partials of the workgroup (16 waves x 4 rows) through LDS, added by ONE lane per (value, column) as four
    //     chains of 16 in row order -- every lane reading all partials of its four columns would be 8x the LDS traffic;
    //  3. the totals back through LDS.
    template <int NV>
    __device__ __forceinline__ void sum(float (&v)[NV][4], float *sm) const
    {
        constexpr int PR = CR_WAVES * 4;                                          // partial rows
        float(*part)[NV * COLS] = reinterpret_cast<float(*)[NV * COLS]>(sm);     // [PR][NV * COLS]
        float *tot = sm + PR * NV * COLS;                                        // [NV * COLS]
#pragma unroll
        for (int q = 0; q < NV; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (L4 <= 1) v[q][e] = add_ror<1>(v[q][e]);
                if (L4 <= 2) v[q][e] = add_ror<2>(v[q][e]);
                if (L4 <= 4) v[q][e] = add_ror<4>(v[q][e]);
                if (L4 <= 8) v[q][e] = add_ror<8>(v[q][e]);
            }
        __syncthreads();                       // previous use of sm is over
        if ((threadIdx.x & 15) < L4)
#pragma unroll
            for (int q = 0; q < NV; ++q)
                *reinterpret_cast<float4 *>(&part[threadIdx.x >> 4][q * COLS + 4 * c4]) = make_float4(v[q][0], v[q][1], v[q][2], v[q][3]);
        __syncthreads();
        if (threadIdx.x < NV * COLS) {
            float a[4];
#pragma unroll
            for (int h = 0; h < 4; ++h) a[h] = part[h * (PR / 4)][threadIdx.x];
#pragma unroll 3                              // 12 reads in flight: fully unrolled, the 64 of them crowd out the cached rows
            for (int w = 1; w < PR / 4; ++w)
#pragma unroll
                for (int h = 0; h < 4; ++h) a[h] += part[h * (PR / 4) + w][threadIdx.x];
            tot[threadIdx.x] = (a[0] + a[1]) + (a[2] + a[3]);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const float4 a = *reinterpret_cast<const float4 *>(&tot[q * COLS + 4 * c4]);
            v[q][0] = a.x; v[q][1] = a.y; v[q][2] = a.z; v[q][3] = a.w;
        }
    }
    static constexpr int SM_FLOATS = (CR_WAVES * 4 + 1) * 2 * COLS;      // for NV <= 2
};

__device__ __forceinline__ void ld4(float (&d)[4], const float *p)
{
    const float4 q = *reinterpret_cast<const float4 *>(p);
    d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
}
__device__ __forceinline__ void st4(float *p, const float (&d)[4]) { *reinterpret_cast<float4 *>(p) = make_float4(d[0], d[1], d[2], d[3]); }

// STATS: only the local statistics of a rank's rows (lcrec_bn_stats: mean -> mean_out, M2 -> rstd_out), nothing applied
template <int COLS, int RMAX, bool STATS = false>
__global__ __launch_bounds__(CR_THREADS) void bn_relu_forward_v4_kernel(const float *__restrict__ t, int64_t n, int F,
                                                                         const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                         float eps, float momentum, float *running_mean,
                                                                         float *running_var, float *__restrict__ y, float *mean_out,
                                                                         float *rstd_out, int relu)
{
    using S = Strip4<COLS>;
    __shared__ __attribute__((aligned(16))) float sm[S::SM_FLOATS];
    const S st(F);
    const int col = st.live ? st.col : 0;          // dead lanes read columns 0..3 and write nothing
    const float inv_n = 1.0f / (float)n;
    const float *tc = t + col;
    float pivot[4];                                // the columns' first row, as in the dword form
    ld4(pivot, tc);
    float tv[RMAX][4];
#pragma unroll
    for (int u = 0; u < RMAX; ++u) {
        const int r = st.rg + u * S::RGS;         // 32-bit offsets from the uniform base (n * F < 2^29)
        ld4(tv[u], t + ((unsigned)(r < (int)n ? r : 0) * (unsigned)F + (unsigned)col));      // no branch between the loads; rows past n read the pivot row: exact zeros below
    }
    float s[2][4] = {};
#pragma unroll
    for (int u = 0; u < RMAX; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d = tv[u][e] - pivot[e];
            s[0][e] += d;
            s[1][e] += d * d;
        }
    float g[4] = {1.f, 1.f, 1.f, 1.f}, b[4] = {};          // in flight with the rows
    if (gamma) ld4(g, gamma + col);
    if (beta) ld4(b, beta + col);
    st.template sum<2>(s, sm);
    if (!st.live) return;
    float mean[4], rstd[4], m2[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float dmean = STATS ? s[0][e] / (float)n : s[0][e] * inv_n;        // (the dword statistics form divides; keep its expression)
        mean[e] = pivot[e] + dmean;
        const float m = s[1][e] - s[0][e] * dmean;
        m2[e] = m > 0.f ? m : 0.f;
        rstd[e] = 1.0f / __builtin_sqrtf(m2[e] * inv_n + eps);
    }
    if (STATS) {
        if (st.rg == 0) { st4(mean_out + col, mean); st4(rstd_out + col, m2); }
        return;
    }
#pragma unroll
    for (int u = 0; u < RMAX; ++u) {
        const int r = st.rg + u * S::RGS;
        if (r < (int)n) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = (tv[u][e] - mean[e]) * rstd[e] * g[e] + b[e];
                if (relu) v[e] = v[e] > 0.f ? v[e] : 0.f;
            }
            st4(y + ((unsigned)r * (unsigned)F + (unsigned)col), v);
        }
    }
    if (st.rg == 0) {
        st4(mean_out + col, mean);
        st4(rstd_out + col, rstd);
        if (running_mean) {
            float rm[4];
            ld4(rm, running_mean + col);
#pragma unroll
            for (int e = 0; e < 4; ++e) rm[e] = (1.0f - momentum) * rm[e] + momentum * mean[e];
            st4(running_mean + col, rm);
        }
        if (running_var) {
            float rv[4];
            ld4(rv, running_var + col);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float unbiased = n > 1 ? m2[e] / (float)(n - 1) : m2[e] * inv_n;
                rv[e] = (1.0f - momentum) * rv[e] + momentum * unbiased;
            }
            st4(running_var + col, rv);
        }
    }
}

// MODE 0: the whole backward of one process.  The data-parallel split (SyncBatchNorm semantics, lcrec_amd/layers.py all-reduces
// between the halves): MODE 1 = lcrec_bn_backward_reduce (the two column sums of this rank's rows, nothing written to dt),
// MODE 2 = lcrec_bn_backward_apply (dt and dbias from the global sums).
template <int COLS, int RMAX, int MODE = 0>
__global__ __launch_bounds__(CR_THREADS) void bn_relu_backward_v4_kernel(BnBwd p)
{
    using S = Strip4<COLS>;
    __shared__ __attribute__((aligned(16))) float sm[S::SM_FLOATS];
    const float *gy = p.gy, *__restrict__ t = p.t, *__restrict__ y = p.y;
    const int64_t n = p.n;
    const int F = p.F, relu = p.relu;
    const S st(F);
    const int col = st.live ? st.col : 0;
    float mu[4], rs[4], gm[4] = {1.f, 1.f, 1.f, 1.f}, fs[4] = {}, fh[4] = {};
    ld4(mu, p.mean + col);
    ld4(rs, p.rstd + col);
    if (MODE != 1 && p.gamma) ld4(gm, p.gamma + col);
    // the ReLU mask: the stored activation; or the consumer's fused expression fma(t, fold_scale, fold_shift); or, with fold_shift
    // alone (= beta), the forward's own expression -- the bits of the y it wrote, one array less to read (in the step: 2 us a call)
    const bool from_y = relu && y, from_fold = relu && !y && p.fold_scale, from_beta = relu && !y && !p.fold_scale;
    if (from_fold) ld4(fs, p.fold_scale + col);
    if (from_fold || from_beta) ld4(fh, p.fold_shift + col);
    float gv[RMAX][4], xv[RMAX][4];               // the lane's masked gradients and xhat, read once
#pragma unroll
    for (int u = 0; u < RMAX; ++u) {
        // Four rows per lane: every load issued unconditionally (rows past n read row 0 and are zeroed) -- no branch, nothing
        // waits between the 12 loads.  Eight rows per lane: a branch per row keeps the compiler from hoisting all 24 loads, which
        // do not fit the 128 registers a 1024-thread workgroup leaves each lane (measured with the spills: 8.8 -> 13.8 us at
        // 1024 x 2048 in 32-column strips).
        const int r = st.rg + u * S::RGS;
        const bool in = r < (int)n;
        const unsigned off = (unsigned)(in ? r : 0) * (unsigned)F + (unsigned)col;      // one 32-bit offset for the three arrays (n * F < 2^29)
        if (RMAX <= 4 || in) {
            float tt[4], yy[4] = {1.f, 1.f, 1.f, 1.f};
            ld4(gv[u], gy + off);
            ld4(tt, t + off);
            if (from_y) ld4(yy, y + off);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xh = (tt[e] - mu[e]) * rs[e];
                const bool on = from_fold ? __builtin_fmaf(tt[e], fs[e], fh[e]) > 0.f : (from_beta ? xh * gm[e] + fh[e] > 0.f : yy[e] > 0.f);
                gv[u][e] = (in && on) ? gv[u][e] : 0.f;
                xv[u][e] = in ? xh : 0.f;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) { gv[u][e] = 0.f; xv[u][e] = 0.f; }
        }
    }
    float s[2][4] = {};
#pragma unroll
    for (int u = 0; u < RMAX; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            s[0][e] += gv[u][e];
            s[1][e] += gv[u][e] * xv[u][e];
        }
    if (MODE == 2) {
        ld4(s[0], p.sum_g + col);
        ld4(s[1], p.sum_gx + col);
    } else {
        st.template sum<2>(s, sm);
    }
    if (MODE == 1) {
        if (st.live && st.rg == 0) {
            st4(p.sum_g + col, s[0]);
            st4(p.sum_gx + col, s[1]);
            if (p.dbeta) st4(p.dbeta + col, s[0]);           // this rank's share of the parameter gradients
            if (p.dgamma) st4(p.dgamma + col, s[1]);
        }
        return;
    }
    float *dt = p.dt, *dgamma = MODE == 0 ? p.dgamma : nullptr, *dbeta = MODE == 0 ? p.dbeta : nullptr, *dbias = p.dbias;
    const float inv_n = 1.0f / (MODE == 2 ? p.n_total : (float)n);
    float k[4], mdb[4], mdg[4], sdt[1][4] = {};
#pragma unroll
    for (int e = 0; e < 4; ++e) { k[e] = gm[e] * rs[e]; mdb[e] = s[0][e] * inv_n; mdg[e] = s[1][e] * inv_n; }
    if (st.live) {
#pragma unroll
        for (int u = 0; u < RMAX; ++u) {
            const int r = st.rg + u * S::RGS;
            if (r < (int)n) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] = k[e] * (gv[u][e] - mdb[e] - xv[u][e] * mdg[e]);
                    sdt[0][e] += v[e];
                }
                st4(dt + ((unsigned)r * (unsigned)F + (unsigned)col), v);
            }
        }
    }
    st.template sum<1>(sdt, sm);
    if (st.live && st.rg == 0) {
        if (dgamma) st4(dgamma + col, s[1]);
        if (dbeta) st4(dbeta + col, s[0]);
        if (dbias) st4(dbias + col, sdt[0]);
    }
}

// ---- the rest of the data-parallel split (the strip kernels above have the halves as modes)
//
// Statistics of the union of the ranks' rows from their (n_r, mean_r[F], M2_r[F]) rows (Chan et al., merged in rank order so
// every rank computes the same bits): mean = sum n_r mean_r / N, M2 = sum (M2_r + n_r (mean_r - mean)^2); rstd and the
// running statistics as nn.BatchNorm1d keeps them (biased variance normalises, unbiased goes into running_var).
__global__ __launch_bounds__(256) void bn_merge_stats_kernel(const float *__restrict__ rows, int world, int F, float eps, float momentum,
                                                             float *mean_out, float *rstd_out, float *running_mean, float *running_var)
{
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= F) return;
    const int64_t stride = 2 * (int64_t)F + 1;
    float total = 0.f, acc = 0.f;
    for (int r = 0; r < world; ++r) {
        const float nr = rows[r * stride];
        total += nr;
        acc += nr * rows[r * stride + 1 + col];
    }
    const float mean = acc / total;
    float m2 = 0.f;
    for (int r = 0; r < world; ++r) {
        const float nr = rows[r * stride];
        const float d = rows[r * stride + 1 + col] - mean;
        m2 += rows[r * stride + 1 + F + col] + nr * (d * d);
    }
    mean_out[col] = mean;
    rstd_out[col] = 1.0f / __builtin_sqrtf(m2 / total + eps);
    if (running_mean) running_mean[col] = (1.0f - momentum) * running_mean[col] + momentum * mean;
    if (running_var) running_var[col] = (1.0f - momentum) * running_var[col] + momentum * (m2 / (total > 1.f ? total - 1.f : 1.f));
}

// y = [relu]((t - mean) * rstd * gamma + beta) with given (global) statistics
__global__ __launch_bounds__(256) void bn_relu_apply_kernel(const float *__restrict__ t, int64_t n, int F, const float *__restrict__ gamma,
                                                            const float *__restrict__ beta, const float *__restrict__ mean,
                                                            const float *__restrict__ rstd, int relu, float *__restrict__ y)
{
    const int64_t total = n * F;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int col = (int)(i % F);
        float v = (t[i] - mean[col]) * rstd[col] * (gamma ? gamma[col] : 1.0f) + (beta ? beta[col] : 0.0f);
        if (relu) v = v > 0.f ? v : 0.f;
        y[i] = v;
    }
}

// g = gy * [y > 0] (in place allowed), dbias = column sums of g
template <int COLS>
__global__ __launch_bounds__(CR_THREADS) void relu_bias_backward_kernel(const float *gy, const float *__restrict__ y, int64_t n, int F,
                                                                         int relu, float *g_out, float *dbias)
{
    __shared__ float sm[CR_WAVES][COLS];
    const Strip<COLS> st(F);
    const int col = st.live ? st.col : 0;
    const float *gc = gy + col, *yc = relu ? y + col : nullptr;
    float *oc = (g_out && st.live) ? g_out + col : nullptr;
    const float s = st.rows(n, [&](int64_t r) {
        float g = gc[r * F];
        if (relu && !(yc[r * F] > 0.f)) g = 0.f;
        if (oc) oc[r * F] = g;
        return g;
    });
    const float db = st.sum(s, sm);
    if (st.live && st.rg == 0 && dbias) dbias[col] = db;
}

// ---- whole-tensor reductions: per-workgroup fp64 partials, then one finishing workgroup (fixed order)
// 1024-thread workgroups, at most 256 of them: as many loads in flight as 1024 x 256 threads, a quarter of the partials -- and
// of the ticket adds, which serialise on their one address (measured: 1024 arrivals cost the gradient-norm launch 8 us)
constexpr int RED_THREADS = 1024;
constexpr int RED_MAX_BLOCKS = TICKET_MAX_WORKGROUPS;

__device__ __forceinline__ double block_sum(double v, double *sm)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < RED_THREADS / 64; ++w) s += sm[w];
    return s;                              // valid in thread 0
}

// Sum of `blocks` per-workgroup partials in the finishing kernels' order (thread i adds partials i, i + 256, ...; then the
// workgroup tree) -- shared by the second-launch form and by the last-workgroup form, so both give the same bits.
template <bool HANDOFF>
__device__ __forceinline__ double sum_partials_ordered(const double *partial, int blocks, double *sm)
{
    double acc = 0.0;
    for (int i = threadIdx.x; i < blocks; i += RED_THREADS) acc += HANDOFF ? handoff_get(partial + i) : partial[i];
    return block_sum(acc, sm);            // valid in thread 0
}

// `ticket` form of a partial-sum kernel's tail: thread 0 publishes the workgroup's partial and takes a ticket; returns true
// (in every thread) in the workgroup that arrived last.
__device__ __forceinline__ bool publish_and_check_last(double *partial, double s, unsigned *ticket, int *last_sh)
{
    if (threadIdx.x == 0) {
        handoff_put(partial + blockIdx.x, s);
        *last_sh = ticket_is_last(ticket, gridDim.x) ? 1 : 0;
    }
    __syncthreads();
    return *last_sh != 0;
}

// mse: loss = mean (out - x)^2, g = 2 (out - x) / count;  l1: loss = mean |out - x|, g = sign(out - x) / count
__global__ __launch_bounds__(RED_THREADS) void recon_loss_grad_kernel(const float *__restrict__ out, const float *__restrict__ x,
                                                                       int64_t count, int64_t count_total, int l1,
                                                                       float *__restrict__ g, double *partial, unsigned *ticket,
                                                                       float *loss, int vec)
{
    __shared__ double sm[RED_THREADS / 64];
    __shared__ int last_sh;
    const float scale = (l1 ? 1.0f : 2.0f) / (float)count_total;
    double acc = 0.0;
    auto one = [&](float o, float t) {
        const float d = o - t;
        if (l1) { acc += (double)__builtin_fabsf(d); return d > 0.f ? scale : (d < 0.f ? -scale : 0.f); }
        acc += (double)d * (double)d;
        return d * scale;
    };
    // 16-byte accesses when the three arrays allow it (a lane's four elements in index order, so the workgroup's sum takes the
    // elements in a fixed order either way); the ragged end and unaligned callers by scalars.  vec: the launcher's
    // aligned16({out, x, g}), the bit its plan reports
    const int64_t quads = vec ? count / 4 : 0;
    for (int64_t q = (int64_t)blockIdx.x * RED_THREADS + threadIdx.x; q < quads; q += (int64_t)gridDim.x * RED_THREADS) {
        const float4 o = reinterpret_cast<const float4 *>(out)[q], t = reinterpret_cast<const float4 *>(x)[q];
        float4 r;
        r.x = one(o.x, t.x); r.y = one(o.y, t.y); r.z = one(o.z, t.z); r.w = one(o.w, t.w);
        if (g) reinterpret_cast<float4 *>(g)[q] = r;
    }
    for (int64_t i = quads * 4 + (int64_t)blockIdx.x * RED_THREADS + threadIdx.x; i < count; i += (int64_t)gridDim.x * RED_THREADS) {
        const float r = one(out[i], x[i]);
        if (g) g[i] = r;
    }
    const double s = block_sum(acc, sm);
    if (!ticket) {
        if (threadIdx.x == 0) partial[blockIdx.x] = s;
        return;
    }
    if (!publish_and_check_last(partial, s, ticket, &last_sh)) return;
    const double total = sum_partials_ordered<true>(partial, gridDim.x, sm);
    if (threadIdx.x == 0) *loss = (float)(total / (double)count_total);
}

__global__ __launch_bounds__(RED_THREADS) void recon_loss_finish_kernel(const double *partial, int blocks, int64_t count, float *loss)
{
    __shared__ double sm[RED_THREADS / 64];
    const double s = sum_partials_ordered<false>(partial, blocks, sm);
    if (threadIdx.x == 0) *loss = (float)(s / (double)count);
}

__device__ __forceinline__ void norm_and_coef(double sumsq, float max_norm, float *norm_out)
{
    const float norm = (float)__builtin_sqrt(sumsq);
    float coef = max_norm / (norm + 1e-6f);
    coef = coef > 1.0f ? 1.0f : coef;
    norm_out[0] = norm;
    norm_out[1] = coef;
}

// 16-byte loads (the flat gradient buffer is 256-byte aligned; a ragged tail is read by scalars): 35 MB at 768-d in ~7 us
__global__ __launch_bounds__(RED_THREADS) void sumsq_kernel(const float *__restrict__ g, int64_t count, double *partial, unsigned *ticket,
                                                             float max_norm, float *norm_out, int vec)
{
    __shared__ double sm[RED_THREADS / 64];
    __shared__ int last_sh;
    double acc = 0.0;
    const int64_t count4 = vec ? count / 4 : 0;                  // vec: g on 16 bytes (the launcher's plan)
    const f32x4 *g4 = reinterpret_cast<const f32x4 *>(g);
    for (int64_t i = (int64_t)blockIdx.x * RED_THREADS + threadIdx.x; i < count4; i += (int64_t)gridDim.x * RED_THREADS) {
        const f32x4 v = g4[i];
        acc += (double)v[0] * (double)v[0];
        acc += (double)v[1] * (double)v[1];
        acc += (double)v[2] * (double)v[2];
        acc += (double)v[3] * (double)v[3];
    }
    for (int64_t i = count4 * 4 + (int64_t)blockIdx.x * RED_THREADS + threadIdx.x; i < count; i += (int64_t)gridDim.x * RED_THREADS) {
        const double v = (double)g[i];
        acc += v * v;
    }
    const double s = block_sum(acc, sm);
    if (!ticket) {
        if (threadIdx.x == 0) partial[blockIdx.x] = s;
        return;
    }
    if (!publish_and_check_last(partial, s, ticket, &last_sh)) return;
    const double total = sum_partials_ordered<true>(partial, gridDim.x, sm);
    if (threadIdx.x == 0) norm_and_coef(total, max_norm, norm_out);
}

// norm_out[0] = ||g||_2, norm_out[1] = clip coefficient min(1, max_norm / (norm + 1e-6))   (torch.nn.utils.clip_grad_norm_)
__global__ __launch_bounds__(RED_THREADS) void grad_norm_finish_kernel(const double *partial, int blocks, float max_norm, float *norm_out)
{
    __shared__ double sm[RED_THREADS / 64];
    const double s = sum_partials_ordered<false>(partial, blocks, sm);
    if (threadIdx.x == 0) norm_and_coef(s, max_norm, norm_out);
}

enum OptimRule { RULE_SGD = 0, RULE_ADAGRAD = 1, RULE_RMSPROP = 2, RULE_ADAM = 3 };

struct OptimParams {
    float *p, *g;
    float *buf;              // momentum buffer: SGD / RMSprop with momentum != 0, else NULL; Adam: exp_avg
    float *sq;               // Adagrad: state_sum; RMSprop: square_avg; Adam: exp_avg_sq
    float *gavg;             // RMSprop centered: grad_avg, else NULL
    unsigned char *buf_ready;    // SGD with momentum: device byte, 0 until a step has set buf = g (torch's first step)
    int64_t count;
    const float *clip;       // [2]: norm, coefficient; or NULL (no clipping)
    int64_t *step;           // device step counter: optimiser steps taken so far (incremented by the kernel's last act)
    double base_lr, weight_decay, momentum, dampening, lr_decay, alpha, eps, beta1, beta2;
    int nesterov, centered;
    int decoupled;           // Adam: 1 = AdamW, 0 = Adam (L2 added to the gradient)
    int schedule;            // 0 = constant after warm-up, 1 = linear decay to 0 at total_steps, -1 = no schedule (lr = base_lr)
    int64_t warmup_steps, total_steps;
    float *lr_out;           // device float: the learning rate this step used (logging / tests), or NULL
    unsigned *ticket;        // with it the LAST workgroup to finish advances *step (no second launch)
    const unsigned char *skip;   // device flag (a sticky "loss was NaN"): when set, nothing is updated and *step stays
};

// learning rate of optimiser step `s` (0-based): base_lr * lambda(s), the python-double arithmetic of
// transformers' get_{linear,constant}_schedule_with_warmup (reference index/trainer.py:83-92)
__device__ __forceinline__ double lr_at(const OptimParams &a, int64_t s)
{
    if (a.schedule < 0) return a.base_lr;
    double f;
    if (s < a.warmup_steps) {
        f = (double)s / (double)(a.warmup_steps > 1 ? a.warmup_steps : 1);
    } else if (a.schedule == 1) {
        const int64_t den = a.total_steps - a.warmup_steps;
        f = (double)(a.total_steps - s) / (double)(den > 1 ? den : 1);
        f = f > 0.0 ? f : 0.0;
    } else {
        f = 1.0;
    }
    return a.base_lr * f;
}

// torch.optim.AdamW / Adam / SGD / Adagrad / RMSprop (the learners of reference index/trainer.py:49-81), single-tensor
// formulation, on the flat buffers: one kernel, the rule a template parameter.  Around the rule: the clip coefficient
// applied to the gradient on the way in (and stored back when it changed it, as clip_grad_norm_ leaves it), the learning
// rate from the device step counter, lr_out, the step advance (ticket) and the NaN skip.  State in fp32,
// hyper-parameters in double folded to float once.
// Adam's arithmetic is written out op by op in include/lcrec.h (the file is built with -ffp-contract=off): exp_avg by torch's
// lerp (below), the rest one rounding per op, none fused.  For the other three, element by element the arithmetic is that of
// torch's CPU kernels for each op of _single_tensor_{sgd,adagrad,rmsprop}:
//   x.add(y, alpha=a)          fma(a, y, x)
//   x.addcmul(y, z, value=a)   fma(a * y, z, x)
//   x.addcdiv(y, z, value=a)   x + (a * y) / z
//   x.lerp(y, w)               |w| < 0.5: fma(w, y - x, x), else fma(w - 1, y - x, y)
//   x.mul(a), sqrt, add        one rounding each (IEEE sqrt and division, no approximations)
constexpr int OPTIM_THREADS = 1024;
template <int RULE>
__global__ __launch_bounds__(OPTIM_THREADS) void optim_step_kernel(OptimParams a)
{
    const bool skip = a.skip && *a.skip;              // uniform over the launch
    const int64_t s = *a.step;                       // steps taken before this one
    const bool first = RULE == RULE_SGD && a.buf && !*a.buf_ready;
    const double lr = lr_at(a, s);
    const float coef = a.clip ? a.clip[1] : 1.0f;
    const bool decay = a.weight_decay != 0.0;
    const float wd = (float)a.weight_decay, epsf = (float)a.eps;
    // the rule's constants; each instantiation computes its own only (Adam alone has the pow and sqrt in double)
    float step_size = 0.f, bc2s = 0.f, b2 = 0.f, one_m_b1 = 0.f, one_m_b2 = 0.f, lr_wd = 0.f;
    float mom = 0.f, neg_lr = 0.f, one_m_damp = 0.f, neg_clr = 0.f, alphaf = 0.f, one_m_alpha = 0.f, lerp_w = 0.f;
    bool lerp_small = false;
    if constexpr (RULE == RULE_ADAM) {
        // bias corrections of step s + 1
        const double t = (double)(s + 1);
        const double bc1 = 1.0 - pow(a.beta1, t);
        const double bc2_sqrt = sqrt(1.0 - pow(a.beta2, t));
        step_size = (float)(lr / bc1);
        b2 = (float)a.beta2; one_m_b1 = (float)(1.0 - a.beta1); one_m_b2 = (float)(1.0 - a.beta2);
        bc2s = (float)bc2_sqrt;
        lr_wd = (float)(lr * a.weight_decay);
        lerp_small = __builtin_fabsf(one_m_b1) < 0.5f;
        lerp_w = lerp_small ? one_m_b1 : one_m_b1 - 1.0f;
    } else {
        // SGD: buf.mul_(momentum).add_(grad, alpha=1 - dampening).  Adagrad: clr = lr / (1 + (step - 1) * lr_decay), step the
        // post-increment count.  RMSprop: square_avg.mul_(alpha).addcmul_(grad, grad, value=1 - alpha), grad_avg.lerp_(grad, 1 - alpha).
        mom = (float)a.momentum;
        neg_lr = (float)(-lr);
        one_m_damp = (float)(1.0 - a.dampening);
        neg_clr = (float)(-(lr / (1.0 + (double)s * a.lr_decay)));
        alphaf = (float)a.alpha; one_m_alpha = (float)(1.0 - a.alpha);
        lerp_small = __builtin_fabsf(one_m_alpha) < 0.5f;
        lerp_w = lerp_small ? one_m_alpha : one_m_alpha - 1.0f;
    }
    // the buffers this rule reads and writes (the others are NULL and never touched); which ones is known at compile time,
    // except for the optional momentum buffer of SGD / RMSprop and RMSprop's grad_avg
    float *const B = a.buf, *const Q = RULE == RULE_SGD ? nullptr : a.sq, *const GA = RULE == RULE_RMSPROP ? a.gavg : nullptr;
    const bool has_b = RULE == RULE_ADAM || B, has_q = RULE != RULE_SGD, has_ga = GA != nullptr;
    if (!skip) {
        // one element: returns the clipped gradient (what clip_grad_norm_ leaves in .grad), updates p and the rule's state
        // (b: momentum buffer | exp_avg, q: sum of squares | exp_avg_sq, ga: RMSprop's grad_avg) in place
        auto one = [&](float &p, float g0, float &b, float &q, float &ga) {
            const float gc = g0 * coef;
            float g = gc;
            if (RULE == RULE_ADAM) {
                if (decay) {
                    if (a.decoupled) p -= lr_wd * p;
                    else g += p * wd;
                }
                b = __builtin_fmaf(lerp_w, g - b, lerp_small ? b : g);   // exp_avg.lerp_(g, 1 - beta1)
                q = b2 * q + one_m_b2 * g * g;
                const float denom = __builtin_sqrtf(q) / bc2s + epsf;
                p -= step_size * b / denom;
                return gc;
            }
            if (decay) g = __builtin_fmaf(wd, p, g);                      // grad.add(param, alpha=weight_decay)
            if (RULE == RULE_SGD) {
                if (has_b) {
                    b = first ? g : __builtin_fmaf(one_m_damp, g, b * mom);
                    g = a.nesterov ? __builtin_fmaf(mom, b, g) : b;      // grad.add(buf, alpha=momentum) | buf
                }
                p = __builtin_fmaf(neg_lr, g, p);                        // param.add_(grad, alpha=-lr)
            } else if (RULE == RULE_ADAGRAD) {
                q = __builtin_fmaf(g, g, q);                             // state_sum.addcmul_(grad, grad, value=1)
                const float std = __builtin_sqrtf(q) + epsf;
                p = p + (neg_clr * g) / std;                             // param.addcdiv_(grad, std, value=-clr)
            } else {
                q = __builtin_fmaf(one_m_alpha * g, g, q * alphaf);
                float avg;
                if (a.centered) {
                    ga = __builtin_fmaf(lerp_w, g - ga, lerp_small ? ga : g);
                    avg = __builtin_sqrtf(__builtin_fmaf(-ga, ga, q));   // square_avg.addcmul(grad_avg, grad_avg, value=-1).sqrt_()
                } else {
                    avg = __builtin_sqrtf(q);
                }
                avg = avg + epsf;
                if (has_b) {
                    b = b * mom + g / avg;                               // buf.mul_(momentum).addcdiv_(grad, avg)
                    p = __builtin_fmaf(neg_lr, b, p);                    // param.add_(buf, alpha=-lr)
                } else {
                    p = p + (neg_lr * g) / avg;                          // param.addcdiv_(grad, avg, value=-lr)
                }
            }
            return gc;
        };
        // 16-byte accesses (the engine's flat buffers are 256-byte aligned; a caller's unaligned or ragged end goes by
        // scalars): a quarter of the memory instructions of the dword form -- for Adam 8.9 M parameters x 8 streams were
        // 1.1 M wave-level instructions on the address path.  The clipped gradient is written back only when clipping
        // changed it (coef != 1).
        const bool vec = (((uintptr_t)a.p | (uintptr_t)a.g | (uintptr_t)B | (uintptr_t)Q | (uintptr_t)GA) & 15) == 0;
        const bool write_g = coef != 1.0f;
        const int64_t quads = vec ? a.count / 4 : 0;
        for (int64_t i = (int64_t)blockIdx.x * OPTIM_THREADS + threadIdx.x; i < quads; i += (int64_t)gridDim.x * OPTIM_THREADS) {
            float4 p = reinterpret_cast<float4 *>(a.p)[i];
            float4 b = has_b ? reinterpret_cast<float4 *>(B)[i] : float4{};
            float4 q = has_q ? reinterpret_cast<float4 *>(Q)[i] : float4{};
            float4 ga = has_ga ? reinterpret_cast<float4 *>(GA)[i] : float4{};
            const float4 g = reinterpret_cast<const float4 *>(a.g)[i];
            float4 gc;
            gc.x = one(p.x, g.x, b.x, q.x, ga.x); gc.y = one(p.y, g.y, b.y, q.y, ga.y);
            gc.z = one(p.z, g.z, b.z, q.z, ga.z); gc.w = one(p.w, g.w, b.w, q.w, ga.w);
            if (write_g) reinterpret_cast<float4 *>(a.g)[i] = gc;
            reinterpret_cast<float4 *>(a.p)[i] = p;
            if (has_b) reinterpret_cast<float4 *>(B)[i] = b;
            if (has_q) reinterpret_cast<float4 *>(Q)[i] = q;
            if (has_ga) reinterpret_cast<float4 *>(GA)[i] = ga;
        }
        for (int64_t i = quads * 4 + (int64_t)blockIdx.x * OPTIM_THREADS + threadIdx.x; i < a.count; i += (int64_t)gridDim.x * OPTIM_THREADS) {
            float p = a.p[i], b = has_b ? B[i] : 0.f, q = has_q ? Q[i] : 0.f, ga = has_ga ? GA[i] : 0.f;
            const float gc = one(p, a.g[i], b, q, ga);
            if (write_g) a.g[i] = gc;
            a.p[i] = p;
            if (has_b) B[i] = b;
            if (has_q) Q[i] = q;
            if (has_ga) GA[i] = ga;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0 && a.lr_out) *a.lr_out = (float)lr;
    }
    if (a.ticket) {
        // every workgroup read *step (and *buf_ready) on entry; the one that finishes last -- after all the others have
        // taken their tickets, i.e. are past those reads -- advances them
        __syncthreads();
        if (threadIdx.x == 0 && ticket_is_last(a.ticket, gridDim.x) && !skip) {
            *a.step = s + 1;
            if (first) *a.buf_ready = 1;
        }
    }
}

// the ticket-less form's second launch: step counter and (SGD momentum) the buffer-holds-a-value byte
__global__ void optim_advance_kernel(int64_t *step, unsigned char *buf_ready, const unsigned char *skip)
{
    if (skip && *skip) return;
    *step += 1;
    if (buf_ready) *buf_ready = 1;
}

// The scalar tail of a step, one thread: level losses and their mean (vq.py:90-92, rq.py:53), total loss (rqvae.py:83),
// the trainer's running sums (trainer.py:122-123) and its NaN check (trainer.py:116) as a sticky device flag.
__global__ void step_losses_kernel(const double *sse, int L, double count, float beta, float qlw, const float *recon,
                                   float *out3, double *sums2, unsigned char *nan_flag, const int64_t *probe,
                                   unsigned char *probe_flag)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (probe && probe_flag && *probe < 0) *probe_flag = 1;     // a poisoned (-1) Sinkhorn assignment: the solver gave up
    float acc = 0.f;
    for (int l = 0; l < L; ++l) {
        const float mse = (float)(sse[l] / count);
        acc += mse + beta * mse;
    }
    const float rq_loss = acc / (float)L;
    const float rec = *recon;
    const float loss = rec + qlw * rq_loss;
    out3[0] = loss; out3[1] = rec; out3[2] = rq_loss;
    if (sums2) { sums2[0] += (double)loss; sums2[1] += (double)rec; }
    if (nan_flag && loss != loss) *nan_flag = 1;
}

// d loss / d z of the quantiser (quantize.py): (coef * (z - C0[idx0])) * weight + g_xq, coef = beta * 2/(L n e)
__global__ __launch_bounds__(256) void quantizer_input_grad_kernel(const float *__restrict__ z, const float *__restrict__ cb0,
                                                                   const int64_t *__restrict__ idx, int64_t idx_stride, int64_t n,
                                                                   int e, float coef, float weight, const float *__restrict__ g_xq,
                                                                   float *__restrict__ out)
{
    const int64_t total = n * e;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / e;
        const int k = (int)(i - row * e);
        const float t = z[i] - cb0[idx[row * idx_stride] * e + k];
        const float u = coef * t;
        const float v = u * weight;
        out[i] = v + g_xq[i];
    }
}

// The same with the column sums of `out` beside it (dbias of the encoder's last Linear, which has neither BatchNorm nor an
// activation behind it: its bias gradient is the column sum of the gradient reaching z): ONE workgroup, thread (row group, column),
// rows ascending per lane, row groups added in order through LDS.  For batch-sized n (n * e <= 64 K elements).
constexpr int QGB_THREADS = 1024;
__global__ __launch_bounds__(QGB_THREADS) void quantizer_input_grad_bias_kernel(const float *__restrict__ z, const float *__restrict__ cb0,
                                                                                const int64_t *__restrict__ idx, int64_t idx_stride, int n,
                                                                                int e, float coef, float weight,
                                                                                const float *__restrict__ g_xq, float *__restrict__ out,
                                                                                float *__restrict__ dbias)
{
    __shared__ float part[QGB_THREADS];
    const int c = threadIdx.x % e, rg = threadIdx.x / e, rgs = QGB_THREADS / e;      // e divides 1024 (16, 32, 64)
    float acc = 0.f;
    for (int r0 = rg; r0 < n; r0 += 4 * rgs) {                // four rows' loads in flight
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = r0 + u * rgs;
            const int rr = r < n ? r : rg;                    // (a valid row: rg < n whenever this loop runs)
            const int64_t i = (int64_t)rr * e + c;
            const float t = z[i] - cb0[idx[(int64_t)rr * idx_stride] * e + c];
            const float uu = coef * t;
            const float w = uu * weight;
            v[u] = w + g_xq[i];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int r = r0 + u * rgs;
            if (r < n) {
                out[(int64_t)r * e + c] = v[u];
                acc += v[u];
            }
        }
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x < e) {
        float s = part[threadIdx.x];
        for (int g = 1; g < rgs; ++g) s += part[g * e + threadIdx.x];
        dbias[threadIdx.x] = s;
    }
}

// dL/dC[k][:] = (scale * (count[k] * C[k][:] - sum[k][:])) * weight -- the closed form autograd derives from vq.py:90-92
// (SURVEY.md a9), in the order quantize.py evaluates it
__global__ __launch_bounds__(256) void codebook_grad_kernel(const float *__restrict__ count, const float *__restrict__ sum,
                                                            const float *__restrict__ cb, int K, int e, float scale, float weight,
                                                            float *__restrict__ grad)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= K * e) return;
    const float t = count[i / e] * cb[i] - sum[i];
    grad[i] = (scale * t) * weight;
}

// ---------------------------------------------------------------- dropout (include/lcrec.h, "Dropout masks")
// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants).  One call yields the four words of elements 4q .. 4q+3.
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t out[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

constexpr int DROP_THREADS = 256;
constexpr int DROP_BLOCKS_PER_CU = 4;   // 16 waves per CU: loads enough in flight for a stream whose ALU work (40 multiplies) is hidden

// MASK_ONLY: keep_out[4q .. 4q+3] = [word >= T]; else out = keep ? in * s : +0 (out may be in).  quads = n * features / 4,
// q0 = row_offset * features / 4: the launch's first counter.  seed and step are read here, from device memory, so a replayed
// graph sees the values of the step it runs in.
template <bool MASK_ONLY>
__global__ __launch_bounds__(DROP_THREADS) void dropout_kernel(const float *in, float *out, unsigned char *keep_out, int64_t quads,
                                                               uint64_t q0, uint32_t T, float s, const int64_t *__restrict__ seed,
                                                               const int64_t *__restrict__ step, uint32_t position)
{
    const uint64_t key = (uint64_t)*seed;
    const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32), c3 = (uint32_t)(uint64_t)*step;
    const int64_t stride = (int64_t)gridDim.x * DROP_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * DROP_THREADS + threadIdx.x; i < quads; i += stride) {
        const uint64_t q = q0 + (uint64_t)i;
        uint32_t w[4];
        philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), position, c3, k0, k1, w);
        if (MASK_ONLY) {
            uchar4 m;
            m.x = w[0] >= T; m.y = w[1] >= T; m.z = w[2] >= T; m.w = w[3] >= T;
            reinterpret_cast<uchar4 *>(keep_out)[i] = m;
        } else {
            const f32x4 x = reinterpret_cast<const f32x4 *>(in)[i];
            f32x4 y;
            y.x = w[0] >= T ? x.x * s : 0.0f;
            y.y = w[1] >= T ? x.y * s : 0.0f;
            y.z = w[2] >= T ? x.z * s : 0.0f;
            y.w = w[3] >= T ? x.w * s : 0.0f;
            reinterpret_cast<f32x4 *>(out)[i] = y;
        }
    }
}

// ---------------------------------------------------------------- fp16 / fp64 -> fp32 (include/lcrec.h, lcrec_cast_rows)
// An embedding file that is not fp32 is copied to HBM as it is and widened / narrowed here: dst[i] = (float)src[i], the
// hardware's own conversions (v_cvt_f32_f16 is exact, v_cvt_f32_f64 rounds to nearest even; fp32 subnormal results are
// kept -- the library is built without denormal flushing).  HBM-bound: 2 + 4 or 8 + 4 bytes per element, no LDS.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int CAST_THREADS = 256;

template <typename SRC> struct CastVec;
template <> struct CastVec<_Float16> { static constexpr int N = 8; };   // one 16-byte load, two 16-byte stores
template <> struct CastVec<double> { static constexpr int N = 4; };     // two 16-byte loads, one 16-byte store

__device__ __forceinline__ void cast_vec(const _Float16 *src, float *dst)
{
    const f16x8 h = *reinterpret_cast<const f16x8 *>(src);
    f32x4 lo, hi;
    lo.x = (float)h[0]; lo.y = (float)h[1]; lo.z = (float)h[2]; lo.w = (float)h[3];
    hi.x = (float)h[4]; hi.y = (float)h[5]; hi.z = (float)h[6]; hi.w = (float)h[7];
    reinterpret_cast<f32x4 *>(dst)[0] = lo;
    reinterpret_cast<f32x4 *>(dst)[1] = hi;
}
__device__ __forceinline__ void cast_vec(const double *src, float *dst)
{
    const f64x2 a = reinterpret_cast<const f64x2 *>(src)[0], b = reinterpret_cast<const f64x2 *>(src)[1];
    f32x4 y;
    y.x = (float)a.x; y.y = (float)a.y; y.z = (float)b.x; y.w = (float)b.y;
    *reinterpret_cast<f32x4 *>(dst) = y;
}

// Elements [head, head + nvec * N) go N at a time through 16-byte accesses: the launcher chose `head` so that src + head and
// dst + head are both 16-byte aligned.  The head and the tail behind the vectors (at most N - 1 elements each) go one element
// per thread in the same launch.  nvec == 0 and head == 0 is the scalar path: every element is an "end".
template <typename SRC>
__global__ __launch_bounds__(CAST_THREADS) void cast_rows_kernel(const SRC *__restrict__ src, float *__restrict__ dst, int64_t count,
                                                                 int head, int64_t nvec)
{
    constexpr int N = CastVec<SRC>::N;
    const int64_t stride = (int64_t)gridDim.x * CAST_THREADS;
    const int64_t first = (int64_t)blockIdx.x * CAST_THREADS + threadIdx.x;
    for (int64_t i = first; i < nvec; i += stride) cast_vec(src + head + i * N, dst + head + i * N);
    const int64_t body = nvec * N, ends = count - body;
    for (int64_t i = first; i < ends; i += stride) {
        const int64_t j = i < head ? i : i + body;
        dst[j] = (float)src[j];
    }
}

// ---------------------------------------------------------------- host side

// dword strip width by feature count: wide layers read 128-byte row segments; narrow ones take narrower strips so that more
// than a handful of CUs work (their whole input is a few hundred KB)
static int strip_cols(int F)
{
    static const int forced = [] { const char *e = getenv("LCREC_STRIP_COLS"); return e ? atoi(e) : 0; }();   // tuning only
    if (forced == 8 || forced == 16 || forced == 32) return forced;
    if (forced == -1) return F >= 4096 ? 32 : (F >= 2048 ? 16 : 8);
    // measured again after the step had become GPU-bound (batch 1024, ms per step at 768-d / 4096-d): this table's
    // predecessor (32 from 1024 columns, 16 from 256, else 8) 1.259 / 1.848, 8 everywhere 1.293 / 1.920, 32 everywhere
    // 1.354 / 1.929, 16 everywhere 1.241 / 1.839
    return 16;
}

// ---- the plan of a BatchNorm strip launch: which kernel family, strip width, rows per lane and grid a call gets for its shape.
// The five host entries below launch by it and lcrec_debug_bn_plan() reports it; neither restates the other.
//
// float4 strips (F a multiple of 4, every pointer on 16 bytes, n * F < 2^29 for the kernels' 32-bit offsets): 16 columns
// (64-byte row segments) where that makes at least 32 strips; narrower strips for narrower layers, whose whole input is a few
// hundred KB that a handful of CUs would pull from memory one after the other (in the step the operands are cold: written by a
// GEMM on other XCDs, or a whole forward pass ago).  32-column strips: measured no better than 16 once the strips of an XCD are
// neighbours (tools/bn_probe.py).  Narrowed while n exceeds 8 rows per lane; beyond that at 4 columns the shape is not theirs.
// dword strips (everything else): strip_cols(F); the whole forward and backward narrow it towards 8 columns while n exceeds
// CR_MAXR rows per lane, so that the register-cached form fits (the halves of the data-parallel split have none and do not
// narrow): the width sets the number of row groups, hence the order of the sums and the bits.  Cached from 1025 rows -- measured
// (768-d recipe): at 1024 rows the second pass hits L2 anyway and the cached form is ~1 % slower; at 2048 rows the narrower
// strips + cached rows are ~3 % of the step faster.
constexpr int V4_MAX_ROWS = 8;
static lcrec_bn_plan bn_plan(int call, int64_t n, int F, bool aligned)
{
    static const int v4 = [] { const char *e = getenv("LCREC_BN_V4"); return e ? atoi(e) : 1; }();   // 0 off; 4 / 8 / 16 force a strip width (tuning)
    lcrec_bn_plan p = {};
    if (v4 && !(F & 3) && aligned && n * F < ((int64_t)1 << 29)) {
        int cols = v4 == 4 || v4 == 8 || v4 == 16 ? v4 : (F >= 512 ? 16 : (F >= 256 ? 8 : 4));
        while (cols > 4 && n > (int64_t)V4_MAX_ROWS * (CR_THREADS / (cols / 4))) cols /= 2;
        const int64_t rgs = CR_THREADS / (cols / 4);
        if (n <= V4_MAX_ROWS * rgs) {
            p.float4 = 1;
            p.cols = cols;
            p.rows_per_lane = n <= rgs ? 1 : (n <= 2 * rgs ? 2 : (n <= 4 * rgs ? 4 : 8));
        }
    }
    if (!p.float4) {
        p.cols = strip_cols(F);
        if (call == LCREC_BN_FORWARD || call == LCREC_BN_BACKWARD) {
            static const int cached_min = [] { const char *e = getenv("LCREC_BN_CACHED_MIN"); return e ? atoi(e) : 1025; }();   // tuning
            while (p.cols > 8 && n > (int64_t)CR_MAXR * (CR_THREADS / p.cols)) p.cols /= 2;
            p.cached = n >= cached_min && n <= (int64_t)CR_MAXR * (CR_THREADS / p.cols);
        }
    }
    p.grid = (F + p.cols - 1) / p.cols;
    p.xcd_order = p.cols < 32 && (p.grid & 7) == 0;          // strip_of_block()
    return p;
}

static bool aligned16(std::initializer_list<const void *> ptrs)
{
    for (const void *p : ptrs)
        if ((uintptr_t)p & 15) return false;
    return true;
}

// the one place a strip width (and the float4 rows per lane) becomes template arguments: f(IntC<COLS>{}) / f(IntC<COLS>{}, IntC<RMAX>{})
template <class Fn>
static void with_strip(int cols, Fn &&f) { cols == 32 ? f(IntC<32>{}) : cols == 16 ? f(IntC<16>{}) : f(IntC<8>{}); }
template <class Fn>
static void with_strip4(const lcrec_bn_plan &p, Fn &&f)
{
    auto rows = [&](auto cols) {
        const int r = p.rows_per_lane;
        r == 1 ? f(cols, IntC<1>{}) : r == 2 ? f(cols, IntC<2>{}) : r == 4 ? f(cols, IntC<4>{}) : f(cols, IntC<8>{});
    };
    p.cols == 16 ? rows(IntC<16>{}) : p.cols == 8 ? rows(IntC<8>{}) : rows(IntC<4>{});
}

template <bool STATS>
static void launch_bn_forward(const lcrec_bn_plan &p, hipStream_t stream, const float *t, int64_t n, int F, const float *gamma,
                              const float *beta, float eps, float momentum, float *running_mean, float *running_var, float *y,
                              float *mean_out, float *rstd_out, int relu)
{
    const dim3 grid((unsigned)p.grid), block(CR_THREADS);
    if (p.float4)
        with_strip4(p, [&](auto cols, auto rmax) {
            hipLaunchKernelGGL((bn_relu_forward_v4_kernel<decltype(cols)::value, decltype(rmax)::value, STATS>), grid, block, 0, stream, t, n, F,
                               gamma, beta, eps, momentum, running_mean, running_var, y, mean_out, rstd_out, relu);
        });
    else
        with_strip(p.cols, [&](auto cols) {
            auto go = [&](auto cached) {
                hipLaunchKernelGGL((bn_relu_forward_kernel<decltype(cols)::value, STATS, decltype(cached)::value != 0>), grid, block, 0, stream, t, n,
                                   F, gamma, beta, eps, momentum, running_mean, running_var, y, mean_out, rstd_out, relu);
            };
            if constexpr (!STATS)
                if (p.cached) return go(IntC<1>{});
            go(IntC<0>{});
        });
}

template <int MODE>
static void launch_bn_backward(const lcrec_bn_plan &p, hipStream_t stream, const BnBwd &a)
{
    const dim3 grid((unsigned)p.grid), block(CR_THREADS);
    if (p.float4)
        with_strip4(p, [&](auto cols, auto rmax) {
            hipLaunchKernelGGL((bn_relu_backward_v4_kernel<decltype(cols)::value, decltype(rmax)::value, MODE>), grid, block, 0, stream, a);
        });
    else
        with_strip(p.cols, [&](auto cols) {
            auto go = [&](auto cached) {
                hipLaunchKernelGGL((bn_relu_backward_kernel<decltype(cols)::value, MODE, decltype(cached)::value != 0>), grid, block, 0, stream, a);
            };
            if constexpr (MODE == 0)
                if (p.cached) return go(IntC<1>{});
            go(IntC<0>{});
        });
}

static int red_blocks(int64_t count, int per_thread = 16)
{
    int64_t b = (count + (int64_t)RED_THREADS * per_thread - 1) / ((int64_t)RED_THREADS * per_thread);
    return (int)(b < 1 ? 1 : (b > RED_MAX_BLOCKS ? RED_MAX_BLOCKS : b));
}

// workgroups of quantizer_input_grad_kernel (four elements per thread, at most 2048)
static int qg_grid(int64_t n, int e)
{
    const int64_t blocks = (n * e + 256 * 4 - 1) / (256 * 4);
    return (int)(blocks > 2048 ? 2048 : blocks);
}

// ---- the plan of a step-tail launch of this file (include/lcrec.h, lcrec_step_tail_plan): relu_bias_backward, the two flat
// reductions and quantizer_input_grad_bias launch by it and lcrec_debug_step_tail_plan() reports it; neither restates the other.
// (rq_apply_level and the code_stats calls: vq_tail_plan, vq_train.hip.)
static lcrec_step_tail_plan step_tail_plan(int call, int64_t n, int width, bool aligned)
{
    lcrec_step_tail_plan p = {};
    if (call == LCREC_TAIL_RELU_BIAS_BACKWARD) {
        p.family = LCREC_TAILK_STRIP;
        p.cols = strip_cols(width);
        p.grid = (width + p.cols - 1) / p.cols;
        p.xcd_order = p.cols < 32 && (p.grid & 7) == 0;          // strip_of_block()
        p.tail = n % ((int64_t)CR_UNROLL * (CR_THREADS / p.cols));
    } else if (call == LCREC_TAIL_RECON_LOSS_GRAD || call == LCREC_TAIL_GRAD_NORM_CLIP) {
        p.family = LCREC_TAILK_REDUCE;
        // the loss: one 16-byte access per lane and array: a batch's 786 k elements on 192 CUs, not 48
        p.grid = red_blocks(n, call == LCREC_TAIL_RECON_LOSS_GRAD ? 4 : 16);
        p.vec16 = aligned;
        p.tail = aligned ? n % 4 : n;
        p.second_launch = 1;
    } else {
        if ((width == 16 || width == 32 || width == 64) && n * width <= 65536) {
            p.family = LCREC_TAILK_QGB_ONE;
            p.grid = 1;
            p.tail = n % (4 * (QGB_THREADS / width));
        } else {                                                  // other shapes: the two launches this call stands for
            p.family = LCREC_TAILK_QG_TWO;
            p.grid = qg_grid(n, width);
            p.second_launch = 1;
        }
    }
    return p;
}

int debug_step_tail_plan(int call, int64_t n, int width, int aligned, lcrec_step_tail_plan *out)
{
    if (!out) return fail(LCREC_EINVAL, "debug_step_tail_plan: NULL pointer");
    if (call < LCREC_TAIL_RELU_BIAS_BACKWARD || call > LCREC_TAIL_CODE_STATS_LEVELS) return fail(LCREC_EINVAL, "debug_step_tail_plan: no such call (%d)", call);
    if (n < 1) return fail(LCREC_EINVAL, "debug_step_tail_plan: n_or_count=%lld", (long long)n);
    const bool flat = call == LCREC_TAIL_RECON_LOSS_GRAD || call == LCREC_TAIL_GRAD_NORM_CLIP;
    if (!flat && width < 1) return fail(LCREC_EINVAL, "debug_step_tail_plan: width=%d", width);
    if (call == LCREC_TAIL_RELU_BIAS_BACKWARD && n > (1 << 20)) return fail(LCREC_EUNSUPPORTED, "debug_step_tail_plan: relu_bias_backward is sized for training batches (n=%lld)", (long long)n);
    if (call >= LCREC_TAIL_RQ_APPLY_LEVEL) {
        const int K = out->K;
        if (call == LCREC_TAIL_RQ_APPLY_LEVEL ? (width % 4 != 0) : K < 1) return fail(LCREC_EINVAL, "debug_step_tail_plan: bad e=%d or out->K=%d", width, K);
        if (!vq_tail_plan(call, n, width, K, out)) return fail(LCREC_EUNSUPPORTED, "debug_step_tail_plan: code_stats: e_dim=%d (supported: 16, 32, 64)", width);
        return LCREC_OK;
    }
    *out = step_tail_plan(call, n, width, aligned != 0);
    return LCREC_OK;
}

int debug_bn_plan(int call, int64_t n, int F, int aligned, lcrec_bn_plan *out)
{
    if (!out) return fail(LCREC_EINVAL, "debug_bn_plan: NULL pointer");
    if (call < LCREC_BN_FORWARD || call > LCREC_BN_BACKWARD_APPLY) return fail(LCREC_EINVAL, "debug_bn_plan: no such call (%d)", call);
    if (n < 1 || n > (1 << 20) || F < 1) return fail(LCREC_EUNSUPPORTED, "debug_bn_plan: sized for training batches (n=%lld)", (long long)n);
    *out = bn_plan(call, n, F, aligned != 0);
    return LCREC_OK;
}

int bn_relu_forward(const float *t, int64_t n, int F, const float *gamma, const float *beta, float eps, float momentum,
                    float *running_mean, float *running_var, float *y, float *mean_out, float *rstd_out, int relu,
                    hipStream_t stream)
{
    if (n == 0 || F == 0) return LCREC_OK;
    if (!t || !y || !mean_out || !rstd_out) return fail(LCREC_EINVAL, "bn_relu_forward: NULL pointer");
    if (n < 2) return fail(LCREC_EINVAL, "bn_relu_forward: training-mode BatchNorm needs more than 1 row (n=%lld)", (long long)n);
    if (n > (1 << 20) || F < 1) return fail(LCREC_EUNSUPPORTED, "bn_relu_forward: sized for training batches (n=%lld)", (long long)n);
    TraceScope trace(K_BN_FWD, stream);
    const lcrec_bn_plan p = bn_plan(LCREC_BN_FORWARD, n, F, aligned16({t, y, gamma, beta, running_mean, running_var, mean_out, rstd_out}));
    launch_bn_forward<false>(p, stream, t, n, F, gamma, beta, eps, momentum, running_mean, running_var, y, mean_out, rstd_out, relu);
    return check_launch(p.float4 ? "bn_relu_forward_v4_kernel" : "bn_relu_forward_kernel");
}

int bn_relu_backward(const float *gy, const float *t, const float *y, int64_t n, int F, const float *gamma, const float *mean,
                     const float *rstd, int relu, float *dt, float *dgamma, float *dbeta, float *dbias, const float *fold_scale,
                     const float *fold_shift, hipStream_t stream)
{
    if (n == 0 || F == 0) return LCREC_OK;
    if (!gy || !t || !mean || !rstd || !dt || (relu && !y && !fold_shift))
        return fail(LCREC_EINVAL, "bn_relu_backward: NULL pointer (with relu: y, or fold_scale and fold_shift, or fold_shift = beta alone)");
    if (n > (1 << 20) || F < 1) return fail(LCREC_EUNSUPPORTED, "bn_relu_backward: sized for training batches (n=%lld)", (long long)n);
    TraceScope trace(K_BN_BWD, stream);
    const lcrec_bn_plan p = bn_plan(LCREC_BN_BACKWARD, n, F, aligned16({gy, t, y, gamma, mean, rstd, dt, dgamma, dbeta, dbias, fold_scale, fold_shift}));
    launch_bn_backward<0>(p, stream, BnBwd{gy, t, y, n, F, gamma, mean, rstd, relu, dt, dgamma, dbeta, dbias, fold_scale, fold_shift, nullptr, nullptr, 0.f});
    return check_launch(p.float4 ? "bn_relu_backward_v4_kernel" : "bn_relu_backward_kernel");
}

int bn_stats(const float *t, int64_t n, int F, float *mean_out, float *m2_out, hipStream_t stream)
{
    if (!t || !mean_out || !m2_out) return fail(LCREC_EINVAL, "bn_stats: NULL pointer");
    if (n < 1 || n > (1 << 20) || F < 1) return fail(LCREC_EUNSUPPORTED, "bn_stats: sized for training batches (n=%lld)", (long long)n);
    TraceScope trace(K_BN_FWD, stream);
    const lcrec_bn_plan p = bn_plan(LCREC_BN_STATS, n, F, aligned16({t, mean_out, m2_out}));
    launch_bn_forward<true>(p, stream, t, n, F, nullptr, nullptr, 0.f, 0.f, nullptr, nullptr, nullptr, mean_out, m2_out, 0);
    return check_launch(p.float4 ? "bn_relu_forward_v4_kernel<stats>" : "bn_relu_forward_kernel<stats>");
}

int bn_merge_stats(const float *rows, int world, int F, float eps, float momentum, float *mean_out, float *rstd_out,
                   float *running_mean, float *running_var, hipStream_t stream)
{
    if (!rows || !mean_out || !rstd_out) return fail(LCREC_EINVAL, "bn_merge_stats: NULL pointer");
    if (world < 1 || world > 4096 || F < 1) return fail(LCREC_EINVAL, "bn_merge_stats: bad shape (world=%d, features=%d)", world, F);
    TraceScope trace(K_BN_FWD, stream);
    hipLaunchKernelGGL(bn_merge_stats_kernel, dim3((F + 255) / 256), dim3(256), 0, stream, rows, world, F, eps, momentum, mean_out,
                       rstd_out, running_mean, running_var);
    return check_launch("bn_merge_stats_kernel");
}

int bn_relu_apply(const float *t, int64_t n, int F, const float *gamma, const float *beta, const float *mean, const float *rstd,
                  int relu, float *y, hipStream_t stream)
{
    if (n == 0 || F == 0) return LCREC_OK;
    if (!t || !mean || !rstd || !y) return fail(LCREC_EINVAL, "bn_relu_apply: NULL pointer");
    int64_t blocks = (n * F + 256 * 8 - 1) / (256 * 8);
    if (blocks > 4096) blocks = 4096;
    TraceScope trace(K_BN_FWD, stream);
    hipLaunchKernelGGL(bn_relu_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, t, n, F, gamma, beta, mean, rstd, relu, y);
    return check_launch("bn_relu_apply_kernel");
}

int bn_backward_reduce(const float *gy, const float *t, const float *y, int64_t n, int F, const float *mean, const float *rstd,
                       int relu, float *sum_g, float *sum_gx, float *dbeta, float *dgamma, hipStream_t stream)
{
    if (!gy || !t || !mean || !rstd || !sum_g || !sum_gx || (relu && !y)) return fail(LCREC_EINVAL, "bn_backward_reduce: NULL pointer");
    if (n < 1 || n > (1 << 20) || F < 1) return fail(LCREC_EUNSUPPORTED, "bn_backward_reduce: sized for training batches");
    TraceScope trace(K_BN_BWD, stream);
    const lcrec_bn_plan p = bn_plan(LCREC_BN_BACKWARD_REDUCE, n, F, aligned16({gy, t, y, mean, rstd, sum_g, sum_gx, dbeta, dgamma}));
    launch_bn_backward<1>(p, stream, BnBwd{gy, t, y, n, F, nullptr, mean, rstd, relu, nullptr, dgamma, dbeta, nullptr, nullptr, nullptr, sum_g, sum_gx, 0.f});
    return check_launch(p.float4 ? "bn_relu_backward_v4_kernel<reduce>" : "bn_relu_backward_kernel<reduce>");
}

int bn_backward_apply(const float *gy, const float *t, const float *y, int64_t n, int F, const float *gamma, const float *mean,
                      const float *rstd, int relu, const float *sum_g, const float *sum_gx, float n_total, float *dt, float *dbias,
                      hipStream_t stream)
{
    if (!gy || !t || !mean || !rstd || !sum_g || !sum_gx || !dt || (relu && !y)) return fail(LCREC_EINVAL, "bn_backward_apply: NULL pointer");
    if (n < 1 || n > (1 << 20) || F < 1 || !(n_total >= 1.0f)) return fail(LCREC_EUNSUPPORTED, "bn_backward_apply: sized for training batches");
    TraceScope trace(K_BN_BWD, stream);
    const lcrec_bn_plan p = bn_plan(LCREC_BN_BACKWARD_APPLY, n, F, aligned16({gy, t, y, gamma, mean, rstd, sum_g, sum_gx, dt, dbias}));
    launch_bn_backward<2>(p, stream, BnBwd{gy, t, y, n, F, gamma, mean, rstd, relu, dt, nullptr, nullptr, dbias, nullptr, nullptr,
                                           const_cast<float *>(sum_g), const_cast<float *>(sum_gx), n_total});
    return check_launch(p.float4 ? "bn_relu_backward_v4_kernel<apply>" : "bn_relu_backward_kernel<apply>");
}

int relu_bias_backward(const float *gy, const float *y, int64_t n, int F, int relu, float *g_out, float *dbias, hipStream_t stream)
{
    if (n == 0 || F == 0) return LCREC_OK;
    if (!gy || (relu && !y)) return fail(LCREC_EINVAL, "relu_bias_backward: NULL pointer");
    if (n > (1 << 20) || F < 1) return fail(LCREC_EUNSUPPORTED, "relu_bias_backward: sized for training batches (n=%lld)", (long long)n);
    TraceScope trace(K_RELU_BIAS_BWD, stream);
    const lcrec_step_tail_plan p = step_tail_plan(LCREC_TAIL_RELU_BIAS_BACKWARD, n, F, true);
    with_strip(p.cols, [&](auto c) {
        hipLaunchKernelGGL(relu_bias_backward_kernel<decltype(c)::value>, dim3((unsigned)p.grid), dim3(CR_THREADS), 0, stream, gy, y,
                           n, F, relu, g_out, dbias);
    });
    return check_launch("relu_bias_backward_kernel");
}

size_t train_reduce_workspace() { return RED_MAX_BLOCKS * sizeof(double); }

int recon_loss_grad(const float *out, const float *x, int64_t count, int64_t count_total, int l1, float *g, float *loss,
                    void *workspace, size_t workspace_bytes, unsigned *ticket, hipStream_t stream)
{
    if (count_total == 0) count_total = count;
    if (count_total < count) return fail(LCREC_EINVAL, "recon_loss_grad: count_total < count");
    if (!out || !x || !loss) return fail(LCREC_EINVAL, "recon_loss_grad: NULL pointer");
    if (count < 1) return fail(LCREC_EINVAL, "recon_loss_grad: empty input");
    if (!workspace || workspace_bytes < train_reduce_workspace()) return fail(LCREC_EWORKSPACE, "recon_loss_grad: workspace too small");
    const lcrec_step_tail_plan p = step_tail_plan(LCREC_TAIL_RECON_LOSS_GRAD, count, 0, aligned16({out, x, g}));
    const int blocks = p.grid;
    TraceScope trace(K_LOSS, stream);
    hipLaunchKernelGGL(recon_loss_grad_kernel, dim3(blocks), dim3(RED_THREADS), 0, stream, out, x, count, count_total, l1, g, (double *)workspace,
                       ticket, loss, p.vec16);
    if (!ticket)
        hipLaunchKernelGGL(recon_loss_finish_kernel, dim3(1), dim3(RED_THREADS), 0, stream, (const double *)workspace, blocks, count_total, loss);
    return check_launch("recon_loss_grad_kernel");
}

int grad_norm_clip(const float *g, int64_t count, float max_norm, float *norm_out, void *workspace, size_t workspace_bytes,
                   unsigned *ticket, hipStream_t stream)
{
    if (!g || !norm_out) return fail(LCREC_EINVAL, "grad_norm_clip: NULL pointer");
    if (count < 1) return fail(LCREC_EINVAL, "grad_norm_clip: empty input");
    if (!workspace || workspace_bytes < train_reduce_workspace()) return fail(LCREC_EWORKSPACE, "grad_norm_clip: workspace too small");
    const lcrec_step_tail_plan p = step_tail_plan(LCREC_TAIL_GRAD_NORM_CLIP, count, 0, aligned16({g}));
    const int blocks = p.grid;
    TraceScope trace(K_GRAD_NORM, stream);
    hipLaunchKernelGGL(sumsq_kernel, dim3(blocks), dim3(RED_THREADS), 0, stream, g, count, (double *)workspace, ticket, max_norm, norm_out,
                       p.vec16);
    if (!ticket)
        hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(RED_THREADS), 0, stream, (const double *)workspace, blocks, max_norm, norm_out);
    return check_launch("grad_norm kernels");
}

int step_losses(const double *sse, int L, int64_t n, int e, float beta, float qlw, const float *recon, float *out3, double *sums2,
                unsigned char *nan_flag, const int64_t *probe, unsigned char *probe_flag, hipStream_t stream)
{
    if (!sse || !recon || !out3) return fail(LCREC_EINVAL, "step_losses: NULL pointer");
    if (L < 1 || L > LCREC_MAX_LEVELS || n < 1 || e < 1) return fail(LCREC_EINVAL, "step_losses: bad shape");
    TraceScope trace(K_LOSS, stream);
    hipLaunchKernelGGL(step_losses_kernel, dim3(1), dim3(64), 0, stream, sse, L, (double)n * (double)e, beta, qlw, recon, out3, sums2, nan_flag,
                       probe, probe_flag);
    return check_launch("step_losses_kernel");
}

int quantizer_input_grad(const float *z, const float *cb0, const int64_t *idx, int64_t idx_stride, int64_t n, int e, float coef,
                         float weight, const float *g_xq, float *out, hipStream_t stream)
{
    if (n == 0) return LCREC_OK;
    if (!z || !cb0 || !idx || !g_xq || !out) return fail(LCREC_EINVAL, "quantizer_input_grad: NULL pointer");
    if (n < 0 || e < 1) return fail(LCREC_EINVAL, "quantizer_input_grad: bad shape");
    const int blocks = qg_grid(n, e);
    TraceScope trace(K_APPLY_LEVEL, stream);
    hipLaunchKernelGGL(quantizer_input_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, z, cb0, idx, idx_stride, n, e, coef, weight,
                       g_xq, out);
    return check_launch("quantizer_input_grad_kernel");
}

int quantizer_input_grad_bias(const float *z, const float *cb0, const int64_t *idx, int64_t idx_stride, int64_t n, int e, float coef,
                              float weight, const float *g_xq, float *out, float *dbias, hipStream_t stream)
{
    if (!dbias) return quantizer_input_grad(z, cb0, idx, idx_stride, n, e, coef, weight, g_xq, out, stream);
    if (n == 0) return LCREC_OK;
    if (!z || !cb0 || !idx || !g_xq || !out) return fail(LCREC_EINVAL, "quantizer_input_grad_bias: NULL pointer");
    if (n < 0 || e < 1) return fail(LCREC_EINVAL, "quantizer_input_grad_bias: bad shape");
    if (step_tail_plan(LCREC_TAIL_QUANTIZER_INPUT_GRAD_BIAS, n, e, true).family == LCREC_TAILK_QGB_ONE) {
        TraceScope trace(K_APPLY_LEVEL, stream);
        hipLaunchKernelGGL(quantizer_input_grad_bias_kernel, dim3(1), dim3(QGB_THREADS), 0, stream, z, cb0, idx, idx_stride, (int)n, e, coef,
                           weight, g_xq, out, dbias);
        return check_launch("quantizer_input_grad_bias_kernel");
    }
    // other shapes: the two launches this call stands for
    if (int rc = quantizer_input_grad(z, cb0, idx, idx_stride, n, e, coef, weight, g_xq, out, stream)) return rc;
    return relu_bias_backward(out, nullptr, n, e, 0, nullptr, dbias, stream);
}

int codebook_grad(const float *count, const float *sum, const float *cb, int K, int e, float scale, float weight, float *grad,
                  hipStream_t stream)
{
    if (!count || !sum || !cb || !grad) return fail(LCREC_EINVAL, "codebook_grad: NULL pointer");
    if (K < 1 || e < 1) return fail(LCREC_EINVAL, "codebook_grad: bad shape");
    TraceScope trace(K_CODE_STATS, stream);
    hipLaunchKernelGGL(codebook_grad_kernel, dim3((K * e + 255) / 256), dim3(256), 0, stream, count, sum, cb, K, e, scale, weight, grad);
    return check_launch("codebook_grad_kernel");
}

// The arguments every rule's entry point has, as launch parameters; the entry point adds its rule's own.
static OptimParams optim_params(float *p, float *g, int64_t count, const float *clip, int64_t *step, double base_lr, double weight_decay,
                                int schedule, int64_t warmup_steps, int64_t total_steps, float *lr_out, unsigned *ticket,
                                const unsigned char *skip)
{
    OptimParams a = {};
    a.p = p; a.g = g; a.count = count; a.clip = clip; a.step = step; a.base_lr = base_lr; a.weight_decay = weight_decay;
    a.schedule = schedule; a.warmup_steps = warmup_steps; a.total_steps = total_steps; a.lr_out = lr_out; a.ticket = ticket; a.skip = skip;
    return a;
}

// The launch of optim_step_kernel (include/lcrec.h, lcrec_optim_plan): launch_optim_step launches by it and
// lcrec_debug_optim_plan() reports it.  The kernel's two loops stride by the whole grid's lanes.
static lcrec_optim_plan optim_plan(int64_t count, bool aligned, bool has_ticket)
{
    lcrec_optim_plan p = {};
    int64_t blocks = (count + OPTIM_THREADS * 8 - 1) / (OPTIM_THREADS * 8);
    if (blocks > TICKET_MAX_WORKGROUPS) blocks = TICKET_MAX_WORKGROUPS;
    p.workgroups = (int)blocks;
    p.second_launch = !has_ticket;
    p.quads = aligned ? count / 4 : 0;
    p.scalars = count - 4 * p.quads;
    const int64_t lanes = blocks * OPTIM_THREADS;
    p.quad_trips_max = (p.quads + lanes - 1) / lanes;
    p.quad_trips_min = p.quads / lanes;
    p.scalar_trips_max = (p.scalars + lanes - 1) / lanes;
    p.scalar_trips_min = p.scalars / lanes;
    return p;
}

int debug_optim_plan(int64_t count, int aligned, int has_ticket, lcrec_optim_plan *out)
{
    if (!out) return fail(LCREC_EINVAL, "debug_optim_plan: NULL pointer");
    if (count < 1) return fail(LCREC_EINVAL, "debug_optim_plan: count=%lld", (long long)count);
    *out = optim_plan(count, aligned != 0, has_ticket != 0);
    return LCREC_OK;
}

// `what`: the entry point, for error texts; `label`: its trace label (K_ADAMW | K_OPTIM_STEP)
template <int RULE>
static int launch_optim_step(const OptimParams &a, const char *what, int label, hipStream_t stream)
{
    if (!a.p || !a.g || !a.step) return fail(LCREC_EINVAL, "%s: NULL pointer", what);
    if (a.count < 1) return fail(LCREC_EINVAL, "%s: empty parameter buffer", what);
    if (a.schedule < -1 || a.schedule > 1) return fail(LCREC_EINVAL, "%s: schedule %d (supported: -1 none, 0 constant, 1 linear)", what, a.schedule);
    if (!(a.base_lr >= 0.0) || !(a.weight_decay >= 0.0)) return fail(LCREC_EINVAL, "%s: lr and weight_decay must be >= 0", what);
    const lcrec_optim_plan plan = optim_plan(a.count, aligned16({a.p, a.g, a.buf, a.sq, a.gavg}), a.ticket != nullptr);
    TraceScope trace(label, stream);
    hipLaunchKernelGGL(optim_step_kernel<RULE>, dim3((unsigned)plan.workgroups), dim3(OPTIM_THREADS), 0, stream, a);
    if (plan.second_launch) hipLaunchKernelGGL(optim_advance_kernel, dim3(1), dim3(1), 0, stream, a.step, a.buf_ready, a.skip);
    return check_launch(what);
}

int adamw_step(float *p, float *g, float *m, float *v, int64_t count, const float *clip, int64_t *step, double base_lr,
               double beta1, double beta2, double eps, double weight_decay, int decoupled, int schedule, int64_t warmup_steps,
               int64_t total_steps, float *lr_out, unsigned *ticket, const unsigned char *skip, hipStream_t stream)
{
    if (!m || !v) return fail(LCREC_EINVAL, "adamw_step: NULL pointer");
    OptimParams a = optim_params(p, g, count, clip, step, base_lr, weight_decay, schedule, warmup_steps, total_steps, lr_out, ticket, skip);
    a.buf = m; a.sq = v; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.decoupled = decoupled;
    return launch_optim_step<RULE_ADAM>(a, "adamw_step", K_ADAMW, stream);
}

int sgd_step(float *p, float *g, float *buf, unsigned char *buf_ready, int64_t count, const float *clip, int64_t *step, double base_lr,
             double momentum, double dampening, int nesterov, double weight_decay, int schedule, int64_t warmup_steps,
             int64_t total_steps, float *lr_out, unsigned *ticket, const unsigned char *skip, hipStream_t stream)
{
    if (!(momentum >= 0.0)) return fail(LCREC_EINVAL, "sgd_step: momentum %g (must be >= 0)", momentum);
    if (momentum != 0.0 && (!buf || !buf_ready))
        return fail(LCREC_EINVAL, "sgd_step: momentum != 0 needs momentum_buffer and momentum_ready");
    if (momentum == 0.0 && (buf || buf_ready)) return fail(LCREC_EINVAL, "sgd_step: momentum_buffer given with momentum 0");
    if (nesterov && (momentum <= 0.0 || dampening != 0.0))
        return fail(LCREC_EINVAL, "sgd_step: nesterov momentum requires a momentum and zero dampening");
    OptimParams a = optim_params(p, g, count, clip, step, base_lr, weight_decay, schedule, warmup_steps, total_steps, lr_out, ticket, skip);
    a.buf = buf; a.buf_ready = buf_ready; a.momentum = momentum; a.dampening = dampening; a.nesterov = nesterov != 0;
    return launch_optim_step<RULE_SGD>(a, "sgd_step", K_OPTIM_STEP, stream);
}

int adagrad_step(float *p, float *g, float *state_sum, int64_t count, const float *clip, int64_t *step, double base_lr, double lr_decay,
                 double eps, double weight_decay, int schedule, int64_t warmup_steps, int64_t total_steps, float *lr_out,
                 unsigned *ticket, const unsigned char *skip, hipStream_t stream)
{
    if (!state_sum) return fail(LCREC_EINVAL, "adagrad_step: NULL pointer");
    if (!(lr_decay >= 0.0) || !(eps >= 0.0)) return fail(LCREC_EINVAL, "adagrad_step: lr_decay and eps must be >= 0");
    OptimParams a = optim_params(p, g, count, clip, step, base_lr, weight_decay, schedule, warmup_steps, total_steps, lr_out, ticket, skip);
    a.sq = state_sum; a.lr_decay = lr_decay; a.eps = eps;
    return launch_optim_step<RULE_ADAGRAD>(a, "adagrad_step", K_OPTIM_STEP, stream);
}

int rmsprop_step(float *p, float *g, float *square_avg, float *buf, float *grad_avg, int64_t count, const float *clip, int64_t *step,
                 double base_lr, double alpha, double eps, double weight_decay, double momentum, int centered, int schedule,
                 int64_t warmup_steps, int64_t total_steps, float *lr_out, unsigned *ticket, const unsigned char *skip, hipStream_t stream)
{
    if (!square_avg) return fail(LCREC_EINVAL, "rmsprop_step: NULL pointer");
    if (!(alpha >= 0.0) || !(eps >= 0.0) || !(momentum >= 0.0)) return fail(LCREC_EINVAL, "rmsprop_step: alpha, eps and momentum must be >= 0");
    if ((momentum > 0.0) != (buf != nullptr))
        return fail(LCREC_EINVAL, "rmsprop_step: momentum_buffer must be given exactly when momentum > 0");
    if ((centered != 0) != (grad_avg != nullptr))
        return fail(LCREC_EINVAL, "rmsprop_step: grad_avg must be given exactly when centered");
    OptimParams a = optim_params(p, g, count, clip, step, base_lr, weight_decay, schedule, warmup_steps, total_steps, lr_out, ticket, skip);
    a.sq = square_avg; a.buf = buf; a.gavg = grad_avg; a.alpha = alpha; a.eps = eps; a.momentum = momentum; a.centered = centered != 0;
    return launch_optim_step<RULE_RMSPROP>(a, "rmsprop_step", K_OPTIM_STEP, stream);
}

// grid of the dropout and cast kernels (one item = one thread's access per trip): from the device's CU count (a batch's widest activation is 2 M elements = 2 k workgroups of
// one access each; 4 per CU make the same passes with fewer workgroups to dispatch), never more than the work
static int dropout_grid(int64_t quads)
{
    static const int cus = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 1) v = 256;
        return v;
    }();
    const int64_t need = (quads + DROP_THREADS - 1) / DROP_THREADS;
    const int64_t cap = (int64_t)cus * DROP_BLOCKS_PER_CU;
    return (int)(need < cap ? need : cap);
}

static int dropout_check(const char *what, int64_t n, int F, const int64_t *seed, const int64_t *step, int position, int64_t row_offset)
{
    if (!seed || !step) return fail(LCREC_EINVAL, "%s: NULL pointer", what);
    if (n < 0 || F < 4 || F % 4) return fail(LCREC_EINVAL, "%s: features %d (a positive multiple of 4) and n %lld (>= 0)", what, F, (long long)n);
    if (position < 0 || row_offset < 0) return fail(LCREC_EINVAL, "%s: position and row_offset must be >= 0", what);
    if (n > INT64_MAX / F - row_offset) return fail(LCREC_EINVAL, "%s: (row_offset + n) * features overflows", what);
    return LCREC_OK;
}

int dropout_apply(const float *in, float *out, int64_t n, int F, uint32_t T, float s, const int64_t *seed, const int64_t *step,
                  int position, int64_t row_offset, hipStream_t stream)
{
    if (int rc = dropout_check("dropout_apply", n, F, seed, step, position, row_offset)) return rc;
    // s = 1 / (1 - p) with 0 <= p < 1: finite and >= 1 (p >= 1 gives inf or a negative value, p < 0 a value below 1, NaN neither)
    if (!(s >= 1.0f) || s > 3.4028234e38f) return fail(LCREC_EINVAL, "dropout_apply: scale %g is not 1 / (1 - p) of a p in [0, 1)", (double)s);
    if (n == 0) return LCREC_OK;
    if (!in || !out) return fail(LCREC_EINVAL, "dropout_apply: NULL pointer");
    if (((uintptr_t)in | (uintptr_t)out) & 15) return fail(LCREC_EINVAL, "dropout_apply: in and out must be 16-byte aligned");
    const int64_t quads = n * F / 4;
    TraceScope trace(K_DROPOUT, stream);
    hipLaunchKernelGGL(dropout_kernel<false>, dim3((unsigned)dropout_grid(quads)), dim3(DROP_THREADS), 0, stream, in, out,
                       (unsigned char *)nullptr, quads, (uint64_t)row_offset * (uint64_t)(F / 4), T, s, seed, step, (uint32_t)position);
    return check_launch("dropout_apply kernel");
}

int dropout_mask(unsigned char *keep_out, int64_t n, int F, uint32_t T, const int64_t *seed, const int64_t *step, int position,
                 int64_t row_offset, hipStream_t stream)
{
    if (int rc = dropout_check("dropout_mask", n, F, seed, step, position, row_offset)) return rc;
    if (n == 0) return LCREC_OK;
    if (!keep_out) return fail(LCREC_EINVAL, "dropout_mask: NULL pointer");
    if ((uintptr_t)keep_out & 3) return fail(LCREC_EINVAL, "dropout_mask: keep_out must be 4-byte aligned");
    const int64_t quads = n * F / 4;
    TraceScope trace(K_DROPOUT, stream);
    hipLaunchKernelGGL(dropout_kernel<true>, dim3((unsigned)dropout_grid(quads)), dim3(DROP_THREADS), 0, stream, (const float *)nullptr,
                       (float *)nullptr, keep_out, quads, (uint64_t)row_offset * (uint64_t)(F / 4), T, 1.0f, seed, step, (uint32_t)position);
    return check_launch("dropout_mask kernel");
}

// The 16-byte path needs src + h and dst + h aligned together for one head h < count.  dst + h is aligned for h = h0, h0 + 4, ...
// (h0 <= 3) and src + h every 8 halves / 2 doubles, so h0 and h0 + 4 are the only candidates worth a look (fp64: h0 alone).
template <typename SRC>
static int launch_cast(const SRC *src, int64_t count, float *dst, hipStream_t stream)
{
    constexpr int N = CastVec<SRC>::N;
    int head = (int)(((16 - ((uintptr_t)dst & 15)) & 15) / 4);
    if (((uintptr_t)(src + head) & 15) && N == 8) head += 4;
    const bool fast = !((uintptr_t)(src + head) & 15) && head + N <= count;
    if (!fast) head = 0;
    const int64_t nvec = fast ? (count - head) / N : 0;
    const int64_t ends = count - nvec * N;
    TraceScope trace(K_CAST, stream);
    hipLaunchKernelGGL(cast_rows_kernel<SRC>, dim3((unsigned)dropout_grid(nvec > ends ? nvec : ends)), dim3(CAST_THREADS), 0, stream, src,
                       dst, count, head, nvec);
    return check_launch("cast_rows kernel");
}

int cast_rows(const void *src, int src_dtype, int64_t count, float *dst, hipStream_t stream)
{
    if (src_dtype != LCREC_DTYPE_F16 && src_dtype != LCREC_DTYPE_F64)
        return fail(LCREC_EINVAL, "cast_rows: src_dtype %d is neither LCREC_DTYPE_F16 (1) nor LCREC_DTYPE_F64 (2)", src_dtype);
    if (count < 0) return fail(LCREC_EINVAL, "cast_rows: count %lld must be >= 0", (long long)count);
    if (count == 0) return LCREC_OK;
    if (!src) return fail(LCREC_EINVAL, "cast_rows: src is NULL");
    if (!dst) return fail(LCREC_EINVAL, "cast_rows: dst is NULL");
    const uintptr_t src_mask = src_dtype == LCREC_DTYPE_F16 ? 1 : 7;
    if ((uintptr_t)src & src_mask) return fail(LCREC_EINVAL, "cast_rows: src must be aligned to its element size (%d bytes)", (int)src_mask + 1);
    if ((uintptr_t)dst & 3) return fail(LCREC_EINVAL, "cast_rows: dst must be 4-byte aligned");
    if (src_dtype == LCREC_DTYPE_F16) return launch_cast(static_cast<const _Float16 *>(src), count, dst, stream);
    return launch_cast(static_cast<const double *>(src), count, dst, stream);
}

}  // namespace lcrec
