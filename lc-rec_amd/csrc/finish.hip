// Nearest-free-code finishing pass over the tuples the conflict rounds leave colliding (opt-in, --finish nearest_free).
//
// The reference stops after its 20 Sinkhorn rounds (index/generate_indices.py:107-128) and writes whatever still collides
// (:131-136 only print the rate).  This pass follows on from there and goes BEYOND the reference: every item that still shares
// its tuple with another is given a free code of the LAST level, chosen by the quantiser's own distance.  Nothing above the last
// level moves, and no item that collides with nobody moves.
//
// The rule: rq_walk.h states the quantiser's arithmetic (the distance d, a NaN as +inf, ties); include/lcrec.h,
// lcrec_finish_nearest_free, is this pass's contract and tests/finish_ref.py restates it in numpy:
//   bucket   = the items sharing idx[:, :L-1]; the caller lists the buckets as (members, offsets), ids ascending in a bucket
//   keepers  : for every last code held by >= 2 items of the bucket the holder with the smallest d keeps it (tie: lowest id);
//              the other holders are movers
//   movers   : in ascending id each takes the free code with the smallest d (tie: lowest code), which is occupied from then on;
//              when no code is free this mover and all later ones of the bucket stay where they are: `unresolved`
//
// Shape: one 256-thread workgroup per bucket.
//   1. histogram of the bucket's last codes in LDS; a bucket without a doubly held code ends here, before anything is staged;
//   2. the codebook goes to LDS once (row stride E + 1 floats: 32 consecutive rows on 32 banks for ds_read_b32), then cc;
//   3. keepers, parallel over members: one chain d(i, own code) each, ds_min_u64 per code on {ordered distance bits, position in
//      the bucket} -- positions ascend with the item id, so the lowest id wins a tie in the same operation;
//   4. movers, sequential: thread t evaluates the full chain of the free codes t, t+256, ...; a wave64 shuffle reduction and one
//      LDS step across the four waves pick (distance, lowest code); the code's owner thread marks it occupied.
// The mover loop stops evaluating when the free count reaches zero -- the rest is counted -- so no bucket takes more than K
// sequential steps whatever its size.  Nothing crosses workgroups: no flag, no spin; the only global atomics are the two counters.
#include "rq_walk.h"

namespace lcrec {

constexpr int FIN_THREADS = 256;
constexpr int FIN_WAVES = FIN_THREADS / 64;

struct FinishParams {
    int64_t *idx;            // [n][L]
    int64_t n;
    int L, K;                // K of the last level
    const float *resid;      // [n][E]
    const float *cb;         // [K][E]
    const int64_t *members, *offsets;
    unsigned long long *counters;   // {moved, unresolved}
};

// lcrec_extend_nearest_free: items with id < n_frozen never move, and resid holds the rows of the new items only
struct ExtendParams : FinishParams {
    int64_t n_frozen;
};

// FROZEN = false is lcrec_finish_nearest_free (every `if constexpr (FROZEN)` drops out); FROZEN = true adds the frozen holders of
// lcrec_extend_nearest_free: fro[k] counts them per code, a code with one has no keeper, and no row of a frozen id is ever read.
template <int E, bool FROZEN>
__global__ __launch_bounds__(FIN_THREADS) void finish_nearest_free_kernel(std::conditional_t<FROZEN, ExtendParams, FinishParams> p)
{
    constexpr int S = E + 1;   // LDS row stride (floats)
    extern __shared__ __attribute__((aligned(16))) unsigned char fin_smem[];
    const int K = p.K;
    unsigned long long *key = reinterpret_cast<unsigned long long *>(fin_smem);   // [K] {ordered distance, position}: the keeper
    float *cbs = reinterpret_cast<float *>(key + K);                              // [K][S]
    float *ccs = cbs + (size_t)K * S;                                             // [K]
    int *cnt = reinterpret_cast<int *>(ccs + K);                                  // [K] holders, then 1 for a code a mover took
    int *fro = cnt + K;                                                           // [K] frozen holders (FROZEN only: not allocated otherwise)
    __shared__ float red_d[2][FIN_WAVES];
    __shared__ int red_k[2][FIN_WAVES];
    __shared__ int sum_sh[FIN_WAVES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t lo = p.offsets[blockIdx.x], hi = p.offsets[blockIdx.x + 1];
    const int64_t m = hi > lo ? hi - lo : 0;
    const int64_t *mem = p.members + lo;
    const int L = p.L;
    int64_t nf = 0;                                                               // ids below it are frozen
    if constexpr (FROZEN) {
        nf = p.n_frozen;
        // ids ascend inside a bucket: a frozen last member means no new item, and such a bucket is never touched
        if (m == 0 || mem[m - 1] < nf) return;
    }

    // a member takes part when its id and its code are in range; any other is left alone (nothing is read or written for it)
    auto code_of = [&](int64_t pos, int64_t &id) -> int {
        id = mem[pos];
        if (id < 0 || id >= p.n) return -1;
        const int64_t c = p.idx[id * L + (L - 1)];
        return (c < 0 || c >= K) ? -1 : (int)c;
    };

    // ---- 1. holders per code
    for (int k = tid; k < K; k += FIN_THREADS) {
        cnt[k] = 0; key[k] = ~0ull;
        if constexpr (FROZEN) fro[k] = 0;
    }
    __syncthreads();
    for (int64_t pos = tid; pos < m; pos += FIN_THREADS) {
        int64_t id;
        const int c = code_of(pos, id);
        if (c >= 0) {
            atomicAdd(&cnt[c], 1);
            if constexpr (FROZEN) { if (id < nf) atomicAdd(&fro[c], 1); }
        }
    }
    __syncthreads();
    int twice = 0, used = 0;
    for (int k = tid; k < K; k += FIN_THREADS) {
        if constexpr (FROZEN) twice |= cnt[k] >= 2 && cnt[k] > fro[k];           // ... with a new item among its holders
        else twice |= cnt[k] >= 2;
        used += cnt[k] > 0;
    }
    if (!__syncthreads_or(twice)) return;                                         // untouched bucket (the whole workgroup leaves)

    // ---- 2. codebook and cc; the count of the free codes rides on the staging's first barrier
    stage_level<E, S, FIN_THREADS>(p.cb, K, cbs, ccs, [&] {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) used += __shfl_xor(used, o, 64);
        if (lane == 0) sum_sh[wave] = used;
    });
    int free_codes = K;
#pragma unroll
    for (int w = 0; w < FIN_WAVES; ++w) free_codes -= sum_sh[w];
    free_codes = __builtin_amdgcn_readfirstlane(free_codes);                      // (the same in every lane: say so, for scalar branches)

    // ---- 3. keepers
    for (int64_t pos = tid; pos < m; pos += FIN_THREADS) {
        int64_t id;
        const int c = code_of(pos, id);
        if (c < 0 || cnt[c] < 2) continue;
        if constexpr (FROZEN) { if (fro[c] > 0 || id < nf) continue; }           // a frozen holder keeps the code: no keeper among the new
        float x[E];
        load_row<E>(p.resid + (id - nf) * E, x);
        const float d = code_distance<E, float>(x, sq_chain<E>(x), cbs + c * S, ccs[c]);
        atomicMin(&key[c], ((unsigned long long)ordered_bits(d) << 32) | (unsigned long long)(uint32_t)pos);
    }
    __syncthreads();

    // ---- 4. movers, in position (= id) order: thread t evaluates the free codes t, t + 256, ...; the code's owner marks it occupied
    unsigned step = 0;
    movers_walk<FIN_THREADS>(
        m, free_codes,
        [&](int64_t pos) -> bool {
            int64_t id;
            const int c = code_of(pos, id);
            if constexpr (FROZEN) return c >= 0 && id >= nf && cnt[c] >= 2 && (fro[c] > 0 || (uint32_t)key[c] != (uint32_t)pos);
            else return c >= 0 && cnt[c] >= 2 && (uint32_t)key[c] != (uint32_t)pos;
        },
        [&](int64_t pos) {
            const int64_t id = mem[pos];                                          // in range: it was found a mover
            float x[E];
            load_row<E>(p.resid + (id - nf) * E, x);                              // a mover is never frozen: id >= nf
            const int bk = wg_nearest_free<E, S, FIN_THREADS>(x, sq_chain<E>(x), cbs, ccs, K, [&](int k) { return cnt[k] == 0; }, red_d,
                                                              red_k, step, lane, wave);
            // a code was free, so bk is one; its owner is the only thread that reads cnt[bk] in this walk
            if (tid == (bk & (FIN_THREADS - 1))) {
                cnt[bk] = 1;
                p.idx[id * L + (L - 1)] = (int64_t)bk;
            }
        },
        sum_sh, p.counters);
}

static size_t finish_lds_bytes(int K, int e, bool frozen)
{
    return (size_t)K * (8 + (size_t)(e + 1) * 4 + 4 + 4 + (frozen ? 4 : 0));   // key, codebook row, cc, cnt, (fro)
}

// Both entries: `frozen` selects lcrec_extend_nearest_free's checks, texts, LDS need and kernel.
static int nearest_free(bool frozen, int64_t *idx, int64_t n, int64_t n_frozen, int L, const int *K, const float *resid_last, int e,
                        const float *codebook_last, const int64_t *bucket_members, const int64_t *bucket_offsets, int64_t n_buckets,
                        int64_t *counters_out, hipStream_t stream)
{
    const char *who = frozen ? "extend_nearest_free" : "finish_nearest_free";
    if (!counters_out) return fail(LCREC_EINVAL, "%s: counters_out is NULL", who);
    if (!K) return fail(LCREC_EINVAL, "%s: K is NULL", who);
    if (L < 1 || L > LCREC_MAX_LEVELS) return fail(LCREC_EINVAL, "%s: L=%d (1 .. %d)", who, L, LCREC_MAX_LEVELS);
    if (n < 0 || n > 0xffffffffLL) return fail(LCREC_EINVAL, "%s: n=%lld (0 .. 2^32 - 1)", who, (long long)n);
    if (n_frozen < 0 || n_frozen > n)
        return fail(LCREC_EINVAL, "%s: n_frozen=%lld (0 .. n=%lld)", who, (long long)n_frozen, (long long)n);
    if (n_buckets < 0 || n_buckets > 0x7fffffffLL)
        return fail(LCREC_EINVAL, "%s: n_buckets=%lld (0 .. 2^31 - 1)", who, (long long)n_buckets);
    if (!e_supported(e)) return fail(LCREC_EUNSUPPORTED, "%s: e_dim=%d (supported: 16, 32, 64)", who, e);
    const int Kl = K[L - 1];
    if (Kl <= 0) return fail(LCREC_EINVAL, "%s: K[%d]=%d", who, L - 1, Kl);
    const size_t lds = finish_lds_bytes(Kl, e, frozen);
    if (!rq_level_fits(Kl, e, L) || lds + 512 > LDS_PER_CU) {
        if (frozen)
            return fail(LCREC_EUNSUPPORTED, "%s: level %d (K=%d, e=%d) does not fit in 160 KB of LDS with the frozen-holder counts "
                        "(%zu B: 4 more per code than finish_nearest_free)", who, L - 1, Kl, e, lds);
        return fail(LCREC_EUNSUPPORTED, "%s: level %d (K=%d, e=%d) does not fit in 160 KB of LDS", who, L - 1, Kl, e);
    }
    if (((uintptr_t)resid_last | (uintptr_t)codebook_last) & 15)
        return fail(LCREC_EINVAL, "%s: resid_last and codebook_last must be 16-byte aligned", who);
    if (((uintptr_t)idx | (uintptr_t)bucket_members | (uintptr_t)bucket_offsets | (uintptr_t)counters_out) & 7)
        return fail(LCREC_EINVAL, "%s: idx, bucket_members, bucket_offsets and counters_out must be 8-byte aligned", who);
    if (n_buckets > 0 && (!idx || !codebook_last || !bucket_members || !bucket_offsets || (!frozen && !resid_last)))
        return fail(LCREC_EINVAL, "%s: NULL pointer", who);
    if (frozen && n_buckets > 0 && !resid_last && n_frozen < n)   // (no new item: there is no row, and NULL is fine)
        return fail(LCREC_EINVAL, "%s: NULL pointer (resid_last, with %lld new items)", who, (long long)(n - n_frozen));
    hipError_t he = hipMemsetAsync(counters_out, 0, 2 * sizeof(int64_t), stream);
    if (he != hipSuccess) return fail(LCREC_EHIP, "%s: %s", who, hipGetErrorString(he));
    if (n_buckets == 0 || n == 0 || n_frozen == n) return LCREC_OK;   // (no new item: nothing can move)

    ExtendParams p;
    p.idx = idx; p.n = n; p.L = L; p.K = Kl;
    p.resid = resid_last; p.cb = codebook_last;
    p.members = bucket_members; p.offsets = bucket_offsets;
    p.counters = reinterpret_cast<unsigned long long *>(counters_out);
    p.n_frozen = n_frozen;
    return with_e(e, [&](auto ec) {
        constexpr int E = decltype(ec)::value;
        auto launch = [&](auto kernel, int trace_id, const char *kernel_name) {
            if (int rc = allow_lds(kernel, lds, who)) return rc;
            TraceScope trace(trace_id, stream);                                   // (the launch alone)
            hipLaunchKernelGGL(kernel, dim3((unsigned)n_buckets), dim3(FIN_THREADS), lds, stream, p);
            return check_launch(kernel_name);
        };
        if (frozen) return launch(finish_nearest_free_kernel<E, true>, K_EXTEND, "extend_nearest_free_kernel");
        return launch(finish_nearest_free_kernel<E, false>, K_FINISH, "finish_nearest_free_kernel");   // (p sliced to FinishParams)
    });
}

int finish_nearest_free(int64_t *idx, int64_t n, int L, const int *K, const float *resid_last, int e, const float *codebook_last,
                        const int64_t *bucket_members, const int64_t *bucket_offsets, int64_t n_buckets, int64_t *counters_out,
                        hipStream_t stream)
{
    return nearest_free(false, idx, n, 0, L, K, resid_last, e, codebook_last, bucket_members, bucket_offsets, n_buckets, counters_out,
                        stream);
}

int extend_nearest_free(int64_t *idx, int64_t n, int64_t n_frozen, int L, const int *K, const float *resid_last, int e,
                        const float *codebook_last, const int64_t *bucket_members, const int64_t *bucket_offsets, int64_t n_buckets,
                        int64_t *counters_out, hipStream_t stream)
{
    return nearest_free(true, idx, n, n_frozen, L, K, resid_last, e, codebook_last, bucket_members, bucket_offsets, n_buckets,
                        counters_out, stream);
}

// ---- lcrec_spill_nearest_free: what the two passes above leave unresolved moves to a sibling bucket (opt-in, --spill) ----------
//
// A bucket that holds more items than the last level has codes cannot be separated by last codes alone.  Such an item takes
// another code one level up -- the nearest one whose row still has a free cell -- and the nearest free last code there, both by the
// quantiser's own distance.  include/lcrec.h, lcrec_spill_nearest_free, is the contract; tests/spill_ref.py restates it in numpy.
//   a = level L-2 (K2 codes, codebook C2, residual r2 entering it); the last level L-1 has K1 codes, C1, r1
//   movers       : of every full tuple held by >= 2 items -- a frozen holder: every new holder; else all new holders but the one
//                  nearest to the shared last code (tie: lowest id)
//   super-bucket : the items sharing idx[:, :L-2]; cell (a, k) is occupied when any of them holds it
//   serving      : movers in ascending id; a' = nearest code (r2, C2) among the rows with a free cell, r' = the residual of r2
//                  behind C2[a'], k = nearest free cell of row a' (r', C1); no free cell anywhere: unresolved
//
// Two kernels.
//   1. spill_keepers_kernel: one wave per shared tuple (a handful of items): the holders are counted, the keeper is a wave
//      reduction on {ordered distance bits, item id}, and the movers' flags are set in the workspace.
//   2. spill_movers_kernel: one 256-thread workgroup per super-bucket, shaped like finish_nearest_free_kernel.  A super-bucket
//      without a flagged member ends before anything is staged.  LDS: both codebooks (row stride E + 1), both cc vectors, one
//      occupancy bit per cell (K2 rows of ceil(K1 / 32) words, the bits past K1 of a row's last word set for good) and the free
//      cells per row.  Per mover two rounds of "every thread evaluates its share, wave64 shuffle reduction, one LDS step across the
//      four waves": rows a = t, t + 256, ... with a free cell, then the free cells k = t, t + 256, ... of the row that won.
//      fre[a] is read and written only by thread a & 255, so no barrier is needed between one mover's update and the next mover's
//      first round; an occupancy bit is read in the second round, a barrier after the update.
// Nothing crosses workgroups; the only global atomics are the two counters.
struct SpillParams {
    int64_t *idx;             // [n][L]
    int64_t n, n_frozen;
    int L, K2, K1;
    const float *r2, *r1;     // [n - n_frozen][E]: the residuals entering levels L-2 and L-1
    const float *cb2, *cb1;
    const int64_t *tmem, *toff;   // the shared tuples
    const int64_t *smem, *soff;   // the super-buckets
    unsigned char *flag;      // [n] (workspace): 1 = mover
    unsigned long long *counters;
};

template <int E>
__global__ __launch_bounds__(FIN_THREADS) void spill_keepers_kernel(SpillParams p, int64_t n_groups)
{
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * FIN_WAVES + (threadIdx.x >> 6);
    if (g >= n_groups) return;                                                    // (the whole wave)
    const int64_t lo = p.toff[g], hi = p.toff[g + 1];
    const int64_t m = hi > lo ? hi - lo : 0;
    const int64_t *mem = p.tmem + lo;
    const int L = p.L;
    const int64_t nf = p.n_frozen;

    // a member is a holder when its id and both its codes are in range; any other takes no part
    auto holder = [&](int64_t pos, int64_t &id) -> int {
        id = mem[pos];
        if (id < 0 || id >= p.n) return -1;
        const int64_t a = p.idx[id * L + (L - 2)], c = p.idx[id * L + (L - 1)];
        return (a < 0 || a >= p.K2 || c < 0 || c >= p.K1) ? -1 : (int)c;
    };

    int holders = 0, frozen = 0;
    for (int64_t pos = lane; pos < m; pos += 64) {
        int64_t id;
        if (holder(pos, id) >= 0) { ++holders; frozen += id < nf; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { holders += __shfl_xor(holders, o, 64); frozen += __shfl_xor(frozen, o, 64); }
    if (holders < 2 || holders == frozen) return;                                 // not shared, or no new holder: no mover

    uint32_t kd = ~0u, ki = ~0u;                                                  // the keeper: {ordered distance, item id}
    if (frozen == 0) {
        for (int64_t pos = lane; pos < m; pos += 64) {
            int64_t id;
            const int c = holder(pos, id);
            if (c < 0) continue;
            const float *cr = p.cb1 + (size_t)c * E;
            float x[E];
            load_row<E>(p.r1 + (id - nf) * E, x);
            // sq_chain's two chains in one loop: taken one after the other they cost the e = 32 form two more VGPRs
            float xx = 0.f, cc = 0.f;
#pragma unroll
            for (int j = 0; j < E; ++j) { xx = __builtin_fmaf(x[j], x[j], xx); cc = __builtin_fmaf(cr[j], cr[j], cc); }
            const uint32_t d = ordered_bits(code_distance<E, float>(x, xx, cr, cc));
            if (d < kd || (d == kd && (uint32_t)id < ki)) { kd = d; ki = (uint32_t)id; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t od = __shfl_xor(kd, o, 64), oi = __shfl_xor(ki, o, 64);
            if (od < kd || (od == kd && oi < ki)) { kd = od; ki = oi; }
        }
    }
    for (int64_t pos = lane; pos < m; pos += 64) {
        int64_t id;
        if (holder(pos, id) < 0 || id < nf) continue;
        if (frozen > 0 || (uint32_t)id != ki) p.flag[id] = 1;
    }
}

template <int E>
__global__ __launch_bounds__(FIN_THREADS) void spill_movers_kernel(SpillParams p)
{
    constexpr int S = E + 1;   // LDS row stride (floats)
    extern __shared__ __attribute__((aligned(16))) unsigned char spill_smem[];
    const int K2 = p.K2, K1 = p.K1, W = (K1 + 31) >> 5;
    float *cb2s = reinterpret_cast<float *>(spill_smem);                          // [K2][S]
    float *cb1s = cb2s + (size_t)K2 * S;                                          // [K1][S]
    float *cc2s = cb1s + (size_t)K1 * S;                                          // [K2]
    float *cc1s = cc2s + K2;                                                      // [K1]
    uint32_t *occ = reinterpret_cast<uint32_t *>(cc1s + K1);                      // [K2][W] bit k & 31 of word k >> 5: cell (a, k)
    int *fre = reinterpret_cast<int *>(occ + (size_t)K2 * W);                     // [K2] free cells of the row
    __shared__ float red_d[2][FIN_WAVES];
    __shared__ int red_k[2][FIN_WAVES];
    __shared__ int sum_sh[FIN_WAVES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t lo = p.soff[blockIdx.x], hi = p.soff[blockIdx.x + 1];
    const int64_t m = hi > lo ? hi - lo : 0;
    const int64_t *mem = p.smem + lo;
    const int L = p.L;
    const int64_t nf = p.n_frozen;

    // a mover is a member the keepers flagged: a new item (id >= nf, so it has rows) whose id and codes were in range
    auto is_mover = [&](int64_t pos) -> bool {
        const int64_t id = mem[pos];
        return id >= nf && id < p.n && p.flag[id] != 0;
    };

    // ---- 1. a super-bucket without a mover is not touched (the whole workgroup leaves)
    int any = 0;
    for (int64_t pos = tid; pos < m; pos += FIN_THREADS) any |= is_mover(pos);
    if (!__syncthreads_or(any)) return;

    // ---- 2. codebooks, cc, and the occupied cells
    stage_rows<E, S, FIN_THREADS>(p.cb2, K2, cb2s);
    stage_rows<E, S, FIN_THREADS>(p.cb1, K1, cb1s);
    for (int q = tid; q < K2 * W; q += FIN_THREADS)
        occ[q] = ((q % W) == W - 1 && (K1 & 31)) ? ~0u << (K1 & 31) : 0u;        // cells past K1 never become free
    __syncthreads();
    stage_cc<E, S, FIN_THREADS>(cb2s, K2 + K1, cc2s);                             // (cb1s follows cb2s, cc1s follows cc2s)
    for (int64_t pos = tid; pos < m; pos += FIN_THREADS) {
        const int64_t id = mem[pos];
        if (id < 0 || id >= p.n) continue;
        const int64_t a = p.idx[id * L + (L - 2)], c = p.idx[id * L + (L - 1)];
        if (a < 0 || a >= K2 || c < 0 || c >= K1) continue;
        atomicOr(&occ[(int)a * W + ((int)c >> 5)], 1u << ((int)c & 31));
    }
    __syncthreads();
    int mine = 0;
    for (int a = tid; a < K2; a += FIN_THREADS) {
        int f = 32 * W;
        for (int w = 0; w < W; ++w) f -= __builtin_popcount(occ[a * W + w]);
        fre[a] = f;
        mine += f;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if (lane == 0) sum_sh[wave] = mine;
    __syncthreads();
    long long free_cells = 0;                                                     // K2 * K1 < 2^62
#pragma unroll
    for (int w = 0; w < FIN_WAVES; ++w) free_cells += sum_sh[w];

    // ---- 3. movers, in position (= id) order
    unsigned step = 0;
    movers_walk<FIN_THREADS>(
        m, free_cells, is_mover,
        [&](int64_t pos) {
            const int64_t id = mem[pos];                                          // in range and new: it was found a mover
            float x[E];
            load_row<E>(p.r2 + (id - nf) * E, x);
            // round 1: the nearest code of level L-2 among the rows with a free cell (there is a free cell, so ba is a row)
            const int ba = wg_nearest_free<E, S, FIN_THREADS>(x, sq_chain<E>(x), cb2s, cc2s, K2, [&](int a) { return fre[a] > 0; }, red_d,
                                                              red_k, step, lane, wave);
            residual_behind<E>(x, cb2s + ba * S);
            // round 2: the nearest free cell of that row (fre[ba] > 0, so bk is a cell)
            const uint32_t *row = occ + ba * W;
            const int bk = wg_nearest_free<E, S, FIN_THREADS>(x, sq_chain<E>(x), cb1s, cc1s, K1,
                                                              [&](int k) { return !((row[k >> 5] >> (k & 31)) & 1u); }, red_d, red_k, step,
                                                              lane, wave);
            if (tid == (bk & (FIN_THREADS - 1))) {
                atomicOr(&occ[ba * W + (bk >> 5)], 1u << (bk & 31));
                p.idx[id * L + (L - 2)] = (int64_t)ba;
                p.idx[id * L + (L - 1)] = (int64_t)bk;
            }
            if (tid == (ba & (FIN_THREADS - 1))) fre[ba] -= 1;                    // its owner: the only thread that reads it
        },
        sum_sh, p.counters);
}

// include/lcrec.h states this formula
static size_t spill_lds_bytes(int K2, int K1, int e)
{
    const size_t words = (size_t)(K1 + 31) / 32;
    return ((size_t)K2 + K1) * ((size_t)(e + 1) * 4 + 4) + (size_t)K2 * (words * 4 + 4);   // codebook rows + cc, bitmap + free count
}

size_t spill_workspace(int64_t n) { return align_up((size_t)(n > 0 ? n : 1), 256); }

int spill_nearest_free(int64_t *idx, int64_t n, int64_t n_frozen, int L, const int *K, const float *resid_prev, const float *resid_last,
                       int e, const float *codebook_prev, const float *codebook_last, const int64_t *tuple_members,
                       const int64_t *tuple_offsets, int64_t n_tuples, const int64_t *super_members, const int64_t *super_offsets,
                       int64_t n_supers, int64_t *counters_out, void *workspace, size_t workspace_bytes, hipStream_t stream)
{
    const char *who = "spill_nearest_free";
    if (!counters_out) return fail(LCREC_EINVAL, "%s: counters_out is NULL", who);
    if (!K) return fail(LCREC_EINVAL, "%s: K is NULL", who);
    if (L < 2 || L > LCREC_MAX_LEVELS)
        return fail(LCREC_EINVAL, "%s: L=%d (2 .. %d: the pass moves an item one level above the last)", who, L, LCREC_MAX_LEVELS);
    if (n < 0 || n > 0xffffffffLL) return fail(LCREC_EINVAL, "%s: n=%lld (0 .. 2^32 - 1)", who, (long long)n);
    if (n_frozen < 0 || n_frozen > n)
        return fail(LCREC_EINVAL, "%s: n_frozen=%lld (0 .. n=%lld)", who, (long long)n_frozen, (long long)n);
    if (n_tuples < 0 || n_tuples > 0x7fffffffLL)
        return fail(LCREC_EINVAL, "%s: n_tuple_groups=%lld (0 .. 2^31 - 1)", who, (long long)n_tuples);
    if (n_supers < 0 || n_supers > 0x7fffffffLL)
        return fail(LCREC_EINVAL, "%s: n_super_buckets=%lld (0 .. 2^31 - 1)", who, (long long)n_supers);
    if (!e_supported(e)) return fail(LCREC_EUNSUPPORTED, "%s: e_dim=%d (supported: 16, 32, 64)", who, e);
    const int K2 = K[L - 2], K1 = K[L - 1];
    if (K2 <= 0) return fail(LCREC_EINVAL, "%s: K[%d]=%d", who, L - 2, K2);
    if (K1 <= 0) return fail(LCREC_EINVAL, "%s: K[%d]=%d", who, L - 1, K1);
    const size_t lds = spill_lds_bytes(K2, K1, e);
    if (lds + 512 > LDS_PER_CU)
        return fail(LCREC_EUNSUPPORTED, "%s: levels %d and %d (K=%d and K=%d, e=%d) need %zu B of LDS together: more than 160 KB", who,
                    L - 2, L - 1, K2, K1, e, lds + 512);
    if (((uintptr_t)resid_prev | (uintptr_t)resid_last | (uintptr_t)codebook_prev | (uintptr_t)codebook_last) & 15)
        return fail(LCREC_EINVAL, "%s: resid_prev, resid_last, codebook_prev and codebook_last must be 16-byte aligned", who);
    if (((uintptr_t)idx | (uintptr_t)tuple_members | (uintptr_t)tuple_offsets | (uintptr_t)super_members | (uintptr_t)super_offsets |
         (uintptr_t)counters_out) & 7)
        return fail(LCREC_EINVAL, "%s: idx, the group tables and counters_out must be 8-byte aligned", who);
    const bool work = n_tuples > 0 && n_supers > 0 && n_frozen < n;
    if (work && (!idx || !resid_prev || !resid_last || !codebook_prev || !codebook_last || !tuple_members || !tuple_offsets ||
                 !super_members || !super_offsets))
        return fail(LCREC_EINVAL, "%s: NULL pointer", who);
    const size_t need = spill_workspace(n);
    if (work && (!workspace || workspace_bytes < need))
        return fail(LCREC_EWORKSPACE, "%s: workspace of %zu bytes, %zu needed (lcrec_spill_nearest_free_workspace)", who,
                    workspace ? workspace_bytes : (size_t)0, need);
    hipError_t he = hipMemsetAsync(counters_out, 0, 2 * sizeof(int64_t), stream);
    if (he != hipSuccess) return fail(LCREC_EHIP, "%s: %s", who, hipGetErrorString(he));
    if (!work) return LCREC_OK;   // (no shared tuple, or no new item: nothing can move)

    SpillParams p;
    p.idx = idx; p.n = n; p.n_frozen = n_frozen; p.L = L; p.K2 = K2; p.K1 = K1;
    p.r2 = resid_prev; p.r1 = resid_last; p.cb2 = codebook_prev; p.cb1 = codebook_last;
    p.tmem = tuple_members; p.toff = tuple_offsets; p.smem = super_members; p.soff = super_offsets;
    p.flag = static_cast<unsigned char *>(workspace);
    p.counters = reinterpret_cast<unsigned long long *>(counters_out);
    return with_e(e, [&](auto ec) {
        constexpr int E = decltype(ec)::value;
        if (int rc = allow_lds(spill_movers_kernel<E>, lds, who)) return rc;
        const hipError_t hm = hipMemsetAsync(p.flag, 0, (size_t)n, stream);
        if (hm != hipSuccess) return fail(LCREC_EHIP, "%s: %s", who, hipGetErrorString(hm));
        {
            TraceScope trace(K_SPILL_KEEPERS, stream);
            const int64_t blocks = (n_tuples + FIN_WAVES - 1) / FIN_WAVES;
            hipLaunchKernelGGL(spill_keepers_kernel<E>, dim3((unsigned)blocks), dim3(FIN_THREADS), 0, stream, p, n_tuples);
            const int rc = check_launch("spill_keepers_kernel");
            if (rc != LCREC_OK) return rc;
        }
        TraceScope trace(K_SPILL, stream);
        hipLaunchKernelGGL(spill_movers_kernel<E>, dim3((unsigned)n_supers), dim3(FIN_THREADS), lds, stream, p);
        return check_launch("spill_movers_kernel");
    });
}

}  // namespace lcrec
