// Decode pass: index tuples back to embeddings, and the reconstruction error of every item (lcrec_decode_tuples; opt-in,
// decode_indices / audit_indices --recon).  Beyond the reference, whose decoder runs only inside RQVAE.forward
// (index/models/rqvae.py:57-66) and whose index/ stage never goes back from a tuple to a vector.
//
// The rule (include/lcrec.h, lcrec_decode_tuples, is the contract; tests/decode_ref.py restates it in numpy).  For item i:
//   h_l  = the held code of level l brought into [0, K_l) by lcrec_rq_apply_level's rule on the int64 value; clamped: flag bit l
//   q    = C_0[h_0], then q = q + C_l[h_l] for l = 1 .. L-1: one fp32 add per element, levels ascending -- the sum of the CODES, not
//          the straight-through sum r + (c - r) that rq_assign writes to xq_out
//   y    = the decoder on q, every layer lcrec_linear_forward (gemm_f32.hip; launched from abi.hip, not from here)
//   err  = per row one chain over the columns ascending, d = y - x: fmaf(d, d, err), or err + |d| for the L1 loss
// Two kernels live here.
//
// rq_decode_gather: rules 1-2.  e / 4 lanes per item, each lane one 16-byte piece of the row: it reads the item's L codes (the lanes
// of an item read the same words: one request), gathers its piece of each held row with a 16-byte load and adds them in level
// order, and stores 16 bytes -- consecutive lanes write consecutive pieces, so a wave stores 1 KB in a row.  The code rows come
// from L2 (a production quantiser is 4 x 256 rows of 128 B); there is no LDS, so any K_l >= 1 is admitted.  A grid-stride loop over
// blocks of 256 / (e / 4) items bounds the grid.
//
// recon_row_error: rule 4.  The chain over a row's columns is sequential, so a lane owns a row: 128 rows per workgroup, one per
// lane.  Read that way from HBM the lanes of a wave would touch 64 different rows at a time, so the workgroup stages tiles of 32
// columns through LDS instead: for the tile, lanes read 16-byte pieces side by side along the rows of y and of x (eight lanes
// cover a row's 128 B, a wave eight rows), write them to LDS with a row stride of 33 floats, and after the barrier every lane walks
// its own row of the tile -- lanes r and r + 1 then sit one bank apart and the 32 lanes of a half wave on 32 different banks, for the
// writes as well (bank = row + column mod 32 in both directions).  The lane carries err from tile to tile, so the result does not
// depend on the tiling.  Rows past n and columns past w are neither loaded nor used.  A grid-stride loop over blocks of 128 rows
// bounds the grid.  y and x are read once and nothing else moves: the kernel is bound by HBM.
// Widths that are no multiple of 4 (rows then start off 16 bytes) stage by single floats, a lane per column: the same tile, the
// same chain.
#include "common.h"

namespace lcrec {

constexpr int DG_THREADS = 256;
constexpr int DG_MAX_GRID = 1024;      // workgroups; the item loop does the rest (include/lcrec.h and tests/decode_cases.py state this)
constexpr int RE_ROWS = 128;           // rows per workgroup = threads: a lane owns a row
constexpr int RE_COLS = 32;            // columns per tile
constexpr int RE_STRIDE = RE_COLS + 1; // LDS row stride (floats)
constexpr int RE_MAX_GRID = 1024;      // 4 workgroups of 33 KB LDS on each of 256 CUs

struct GatherParams {
    const int64_t *idx;
    int64_t idx_stride;
    int64_t n;
    const float *cb[LCREC_MAX_LEVELS];   // level l's rows
    int K[LCREC_MAX_LEVELS];
    int L;
    float *q;                            // [n][E]
    uint32_t *flags;                     // [n] or NULL
};

template <int E>
__global__ __launch_bounds__(DG_THREADS) void rq_decode_gather_kernel(GatherParams p)
{
    constexpr int LANES = E / 4;                      // lanes per item
    constexpr int ITEMS = DG_THREADS / LANES;         // items per workgroup and trip
    const int g = threadIdx.x % LANES, slot = threadIdx.x / LANES;
    for (int64_t base = (int64_t)blockIdx.x * ITEMS; base < p.n; base += (int64_t)gridDim.x * ITEMS) {
        const int64_t i = base + slot;
        if (i >= p.n) continue;                       // tail of the last block (no barrier anywhere)
        const int64_t *held = p.idx + i * p.idx_stride;
        f32x4 q;
        uint32_t flags = 0;
        for (int l = 0; l < p.L; ++l) {
            const int64_t v = held[l];
            const int K = p.K[l];
            const int64_t h = v < 0 ? 0 : (v >= K ? K - 1 : v);
            flags |= (v < 0 || v >= K) ? (1u << l) : 0u;
            const f32x4 c = *reinterpret_cast<const f32x4 *>(p.cb[l] + h * E + 4 * g);
            if (l == 0) q = c;
            else { q[0] = q[0] + c[0]; q[1] = q[1] + c[1]; q[2] = q[2] + c[2]; q[3] = q[3] + c[3]; }
        }
        *reinterpret_cast<f32x4 *>(p.q + i * E + 4 * g) = q;
        if (p.flags && g == 0) p.flags[i] = flags;
    }
}

template <int E>
static int gather_launch(const GatherParams &p, hipStream_t stream)
{
    constexpr int ITEMS = DG_THREADS / (E / 4);
    const int64_t blocks = (p.n + ITEMS - 1) / ITEMS;
    const int grid = (int)(blocks < DG_MAX_GRID ? blocks : DG_MAX_GRID);
    hipLaunchKernelGGL(rq_decode_gather_kernel<E>, dim3((unsigned)grid), dim3(DG_THREADS), 0, stream, p);
    return check_launch("rq_decode_gather_kernel");
}

// Arguments are checked by the caller (abi.hip, decode_tuples): e in {16, 32, 64}, 1 <= L <= LCREC_MAX_LEVELS, K[l] >= 1, n > 0.
int rq_decode_gather(const int64_t *idx, int64_t idx_stride, int64_t n, int e, const float *codebooks, const int *K, int L,
                     float *q_out, uint32_t *flags_out, hipStream_t stream)
{
    GatherParams p;
    p.idx = idx; p.idx_stride = idx_stride; p.n = n; p.L = L; p.q = q_out; p.flags = flags_out;
    int64_t off = 0;
    for (int l = 0; l < LCREC_MAX_LEVELS; ++l) {
        p.cb[l] = l < L ? codebooks + off : nullptr;
        p.K[l] = l < L ? K[l] : 0;
        if (l < L) off += (int64_t)K[l] * e;
    }
    TraceScope trace(K_RQ_DECODE_GATHER, stream);
    return with_e(e, [&](auto ec) { return gather_launch<decltype(ec)::value>(p, stream); });
}

// VEC: w % 4 == 0 and both arrays on 16 bytes: every row starts on 16 bytes
template <bool VEC, bool L1>
__global__ __launch_bounds__(RE_ROWS) void recon_row_error_kernel(const float *__restrict__ y, const float *__restrict__ x, int64_t n,
                                                                    int w, float *__restrict__ err_out)
{
    __shared__ float ys[RE_ROWS * RE_STRIDE];
    __shared__ float xs[RE_ROWS * RE_STRIDE];
    const int tid = threadIdx.x;
    for (int64_t row0 = (int64_t)blockIdx.x * RE_ROWS; row0 < n; row0 += (int64_t)gridDim.x * RE_ROWS) {
        const int64_t left = n - row0;
        const int rows = left < RE_ROWS ? (int)left : RE_ROWS;
        float err = 0.f;
        for (int c0 = 0; c0 < w; c0 += RE_COLS) {
            const int cols = w - c0 < RE_COLS ? w - c0 : RE_COLS;
            if (VEC) {
                constexpr int PER_ROW = RE_COLS / 4;                       // 16-byte pieces per tile row
                constexpr int TRIPS = RE_ROWS * PER_ROW / RE_ROWS;         // pieces per lane: 8
                f32x4 vy[TRIPS], vx[TRIPS];
#pragma unroll
                for (int k = 0; k < TRIPS; ++k) {
                    const int q = tid + RE_ROWS * k, r = q / PER_ROW, c = 4 * (q % PER_ROW);
                    if (r < rows && c < cols) {                            // (w % 4 == 0: a piece is inside the row or outside it)
                        const int64_t at = (row0 + r) * w + c0 + c;
                        vy[k] = *reinterpret_cast<const f32x4 *>(y + at);
                        vx[k] = *reinterpret_cast<const f32x4 *>(x + at);
                    } else {
                        vy[k] = f32x4{0.f, 0.f, 0.f, 0.f};
                        vx[k] = f32x4{0.f, 0.f, 0.f, 0.f};
                    }
                }
                __syncthreads();                                           // the previous tile has been read
#pragma unroll
                for (int k = 0; k < TRIPS; ++k) {
                    const int q = tid + RE_ROWS * k, r = q / PER_ROW, c = 4 * (q % PER_ROW);
                    float *dy = ys + r * RE_STRIDE + c, *dx = xs + r * RE_STRIDE + c;
                    dy[0] = vy[k][0]; dy[1] = vy[k][1]; dy[2] = vy[k][2]; dy[3] = vy[k][3];
                    dx[0] = vx[k][0]; dx[1] = vx[k][1]; dx[2] = vx[k][2]; dx[3] = vx[k][3];
                }
            } else {
                constexpr int TRIPS = RE_ROWS * RE_COLS / RE_ROWS;         // floats per lane: 32
                __syncthreads();
                const int c = tid % RE_COLS;
                for (int k = 0; k < TRIPS; ++k) {
                    const int r = (tid + RE_ROWS * k) / RE_COLS;
                    const bool in = r < rows && c < cols;
                    const int64_t at = (row0 + r) * w + c0 + c;
                    ys[r * RE_STRIDE + c] = in ? y[at] : 0.f;
                    xs[r * RE_STRIDE + c] = in ? x[at] : 0.f;
                }
            }
            __syncthreads();
            if (tid < rows) {
                const float *ry = ys + tid * RE_STRIDE, *rx = xs + tid * RE_STRIDE;
                if (cols == RE_COLS) {
#pragma unroll
                    for (int j = 0; j < RE_COLS; ++j) {
                        const float d = ry[j] - rx[j];
                        err = L1 ? err + __builtin_fabsf(d) : __builtin_fmaf(d, d, err);
                    }
                } else {
                    for (int j = 0; j < cols; ++j) {
                        const float d = ry[j] - rx[j];
                        err = L1 ? err + __builtin_fabsf(d) : __builtin_fmaf(d, d, err);
                    }
                }
            }
        }
        if (tid < rows) err_out[row0 + tid] = err;
        __syncthreads();                                                   // (the next trip's first tile is staged behind a barrier anyway; w == 0 never gets here)
    }
}

// Arguments are checked by the caller: n > 0, w >= 1, y / x / err_out given.
int recon_row_error(const float *y, const float *x, int64_t n, int w, int l1, float *err_out, hipStream_t stream)
{
    const int64_t blocks = (n + RE_ROWS - 1) / RE_ROWS;
    const int grid = (int)(blocks < RE_MAX_GRID ? blocks : RE_MAX_GRID);
    const bool vec = w % 4 == 0 && (((uintptr_t)y | (uintptr_t)x) & 15) == 0;
    TraceScope trace(K_RECON_ROW_ERROR, stream);
    auto kern = vec ? (l1 ? recon_row_error_kernel<true, true> : recon_row_error_kernel<true, false>)
                    : (l1 ? recon_row_error_kernel<false, true> : recon_row_error_kernel<false, false>);
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(RE_ROWS), 0, stream, y, x, n, w, err_out);
    return check_launch("recon_row_error_kernel");
}

}  // namespace lcrec
