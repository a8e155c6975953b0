// The residual quantiser's walk, as the index-side passes take it: finish.hip, audit.hip and beam.hip build on these pieces and
// on nothing else, so the bits they promise are stated -- and written -- once, here.  (rq_assign.hip keeps its own MFMA-shaped
// form of the same rule, pinned by its own table.)
//
// The rule (oracle/lcrec_oracle.c's lcrec_oracle_distances; tests/finish_ref.py, spill_ref.py, audit_ref.py and beam_ref.py
// restate it in numpy):
//   d(r, c)  = (xx + cc) - 2*dot, with xx = sum r[j]^2, cc = sum c[j]^2 and dot = sum r[j]*c[j] each ONE fp32 fma chain over the
//              dimension ascending from 0.f (sq_chain, code_distance); no contraction, no reassociation
//   compare  : wherever distances are compared or reported a NaN counts as +inf, so it never beats anything (nan_as_inf; ordered_bits
//              for the unsigned form, which also folds -0 into +0)
//   argmin   : smallest distance, lowest code on a tie (wg_argmin across a workgroup)
//   residual : behind code c, three operations in this order and no other: t = c - r; s = r + t; r' = r - s (residual_behind)
// Rows are moved between memory and registers in 16-byte pieces (load_row, store_row); a level's codebook and its cc go to LDS
// once per workgroup (stage_rows, stage_cc, stage_level), at a row stride the caller chooses: E + 4 floats keeps rows 16-byte
// aligned for ds_read_b128 under a broadcast sweep, E + 1 puts 32 consecutive rows on 32 banks for ds_read_b32 when every lane
// reads a row of its own.
#pragma once
#include "common.h"

#include <type_traits>

namespace lcrec {

constexpr int NO_CODE = 0x7fffffff;   // "no candidate" in an argmin: behind every code on a tie

template <int E>
__device__ __forceinline__ void load_row(const float *__restrict__ src, float (&x)[E])
{
    const f32x4 *s = reinterpret_cast<const f32x4 *>(src);
#pragma unroll
    for (int q = 0; q < E / 4; ++q) {
        const f32x4 v = s[q];
        x[4 * q] = v[0]; x[4 * q + 1] = v[1]; x[4 * q + 2] = v[2]; x[4 * q + 3] = v[3];
    }
}

template <int E>
__device__ __forceinline__ void store_row(float *__restrict__ dst, const float (&x)[E])
{
    f32x4 *d = reinterpret_cast<f32x4 *>(dst);
#pragma unroll
    for (int q = 0; q < E / 4; ++q) {
        f32x4 v;
        v[0] = x[4 * q]; v[1] = x[4 * q + 1]; v[2] = x[4 * q + 2]; v[3] = x[4 * q + 3];
        d[q] = v;
    }
}

// xx, cc and err: the fma chain of squares
template <int E>
__device__ __forceinline__ float sq_chain(const float *v)
{
    float a = 0.f;
#pragma unroll
    for (int j = 0; j < E; ++j) a = __builtin_fmaf(v[j], v[j], a);
    return a;
}

// The raw d.  ROW is the width at which the code's row is read: f32x4 for a 16-byte aligned row (stride E + 4), float otherwise.
template <int E, class ROW>
__device__ __forceinline__ float code_distance(const float (&x)[E], float xx, const float *crow, float cc)
{
    float dot = 0.f;
    if constexpr (std::is_same_v<ROW, f32x4>) {
        const f32x4 *c4 = reinterpret_cast<const f32x4 *>(crow);
#pragma unroll
        for (int q = 0; q < E / 4; ++q) {
            const f32x4 c = c4[q];
            dot = __builtin_fmaf(x[4 * q], c[0], dot);
            dot = __builtin_fmaf(x[4 * q + 1], c[1], dot);
            dot = __builtin_fmaf(x[4 * q + 2], c[2], dot);
            dot = __builtin_fmaf(x[4 * q + 3], c[3], dot);
        }
    } else {
        static_assert(std::is_same_v<ROW, float>, "a row is read by 16 bytes or by single floats");
#pragma unroll
        for (int k = 0; k < E; ++k) dot = __builtin_fmaf(x[k], crow[k], dot);
    }
    const float t = xx + cc;
    return t - 2.0f * dot;
}

__device__ __forceinline__ float nan_as_inf(float d) { return d == d ? d : __builtin_inff(); }

// unsigned order of the result == float order of d; NaN -> +inf, -0 -> +0
__device__ __forceinline__ uint32_t ordered_bits(float d)
{
    d = nan_as_inf(d);
    if (d == 0.f) d = 0.f;
    const uint32_t u = __float_as_uint(d);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// x becomes the residual behind the code whose row is crow
template <int E>
__device__ __forceinline__ void residual_behind(float (&x)[E], const float *crow)
{
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const float t = crow[j] - x[j];
        const float s = x[j] + t;
        x[j] = x[j] - s;
    }
}

// K rows of E floats to LDS at a row stride of STRIDE floats.  No barrier.
template <int E, int STRIDE, int THREADS>
__device__ __forceinline__ void stage_rows(const float *cb, int K, float *cbs)
{
    for (int q = threadIdx.x; q < K * (E / 4); q += THREADS) {
        const int row = q / (E / 4), g = q % (E / 4);
        const f32x4 v = *reinterpret_cast<const f32x4 *>(cb + (size_t)row * E + 4 * g);
        float *dst = cbs + row * STRIDE + 4 * g;
        if constexpr (STRIDE % 4 == 0) *reinterpret_cast<f32x4 *>(dst) = v;
        else { dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3]; }
    }
}

// cc of K staged rows (behind the barrier that follows stage_rows).  No barrier.
template <int E, int STRIDE, int THREADS>
__device__ __forceinline__ void stage_cc(const float *cbs, int K, float *ccs)
{
    for (int k = threadIdx.x; k < K; k += THREADS) ccs[k] = sq_chain<E>(cbs + k * STRIDE);
}

// One level: rows, barrier, cc, barrier.  `between` runs before the first barrier, for what a caller wants published by it.
template <int E, int STRIDE, int THREADS, class Between>
__device__ __forceinline__ void stage_level(const float *cb, int K, float *cbs, float *ccs, Between between)
{
    stage_rows<E, STRIDE, THREADS>(cb, K, cbs);
    between();
    __syncthreads();
    stage_cc<E, STRIDE, THREADS>(cbs, K, ccs);
    __syncthreads();
}
template <int E, int STRIDE, int THREADS>
__device__ __forceinline__ void stage_level(const float *cb, int K, float *cbs, float *ccs)
{
    stage_level<E, STRIDE, THREADS>(cb, K, cbs, ccs, [] {});
}

// (best, bk) of the whole workgroup, the same in every thread: smallest distance, lowest code on a tie; NO_CODE: no candidate.
// A wave64 shuffle reduction, then one LDS step over the waves.  Every thread calls it, with the same `step`.
template <int WAVES>
__device__ __forceinline__ int wg_argmin(float best, int bk, float (*red_d)[WAVES], int (*red_k)[WAVES], unsigned &step, int lane,
                                         int wave)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float od = __shfl_xor(best, o, 64);
        const int ok = __shfl_xor(bk, o, 64);
        if (od < best || (od == best && ok < bk)) { best = od; bk = ok; }
    }
    const int par = step & 1;   // two hand-over buffers: a wave can be one reduction ahead of another, never two
    ++step;
    if (lane == 0) { red_d[par][wave] = best; red_k[par][wave] = bk; }
    __syncthreads();
    best = red_d[par][0]; bk = red_k[par][0];
#pragma unroll
    for (int v = 1; v < WAVES; ++v) {
        const float od = red_d[par][v];
        const int ok = red_k[par][v];
        if (od < best || (od == best && ok < bk)) { best = od; bk = ok; }
    }
    return __builtin_amdgcn_readfirstlane(bk);
}

// The nearest of the staged codes k with is_free(k), for the whole workgroup: thread t evaluates k = t, t + THREADS, ...
template <int E, int STRIDE, int THREADS, class Free>
__device__ __forceinline__ int wg_nearest_free(const float (&x)[E], float xx, const float *cbs, const float *ccs, int K, Free is_free,
                                               float (*red_d)[THREADS / 64], int (*red_k)[THREADS / 64], unsigned &step, int lane,
                                               int wave)
{
    float best = __builtin_inff();
    int bk = NO_CODE;
    for (int k = threadIdx.x; k < K; k += THREADS) {
        if (!is_free(k)) continue;
        const float d = nan_as_inf(code_distance<E, float>(x, xx, cbs + k * STRIDE, ccs[k]));
        if (bk == NO_CODE || d < best) { best = d; bk = k; }
    }
    return wg_argmin(best, bk, red_d, red_k, step, lane, wave);
}

// The movers walk of one workgroup over a bucket of m positions (= ids ascending), a chunk of THREADS positions at a time:
// is_mover(pos) says which take part, serve(pos) -- called by every thread, movers in ascending position -- gives one a place, and
// each serve uses up one of the free_left places.  When none is left this mover and all later ones stay: those met inside a
// chunk are counted one by one (late), those of whole later chunks in parallel (my_late).  counters[0] += served,
// counters[1] += left behind.  free_left, moved and late are the same in every thread.  sum_sh: THREADS / 64 ints of LDS that
// nobody else uses from here on.
template <int THREADS, class Count, class IsMover, class Serve>
__device__ __forceinline__ void movers_walk(int64_t m, Count free_left, IsMover is_mover, Serve serve, int *sum_sh,
                                            unsigned long long *counters)
{
    constexpr int WAVES = THREADS / 64;
    __shared__ unsigned long long wmask[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long moved = 0, late = 0;
    unsigned my_late = 0;
    for (int64_t base = 0; base < m; base += THREADS) {
        const int64_t pos = base + tid;
        const bool mover = pos < m && is_mover(pos);
        if (free_left == 0) { my_late += mover; continue; }
        const unsigned long long mine = __ballot(mover);
        if (lane == 0) wmask[wave] = mine;
        __syncthreads();
        unsigned long long masks[WAVES];
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const unsigned long long v = wmask[w];
            masks[w] = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(v >> 32)) << 32) |
                       (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)v);   // (it returns int)
        }
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            unsigned long long mask = masks[w];
            while (mask) {
                if (free_left == 0) { late += __builtin_popcountll(mask); break; }
                const int bit = __builtin_ctzll(mask);
                mask &= mask - 1;
                serve(base + w * 64 + bit);
                ++moved;
                --free_left;
            }
        }
        __syncthreads();   // wmask is rewritten by the next chunk
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) my_late += __shfl_xor(my_late, o, 64);
    __syncthreads();
    if (lane == 0) sum_sh[wave] = (int)my_late;
    __syncthreads();
    if (tid == 0) {
        for (int w = 0; w < WAVES; ++w) late += (unsigned)sum_sh[w];
        if (moved) atomicAdd(&counters[0], moved);
        if (late) atomicAdd(&counters[1], late);
    }
}

}  // namespace lcrec
