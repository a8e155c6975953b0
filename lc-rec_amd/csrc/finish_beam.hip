// Beam finishing pass: colliding items move to their next-best WHOLE tuple nobody holds (lcrec_finish_beam; opt-in, generate
// --finish beam), and its frozen-aware form for a catalogue that grows (lcrec_extend_finish_beam; generate --extend --extend_finish
// beam): one body, lcrec_finish_beam is n_frozen = 0.
//
// lcrec_finish_nearest_free changes a last code and lcrec_spill_nearest_free the last two; lcrec_rq_beam lists the W best whole
// tuples of an item with their exact errors.  This pass brings the two together and goes BEYOND the reference: of every shared tuple
// the member with the smallest error keeps it, and the others walk down their own candidate lists, in synchronous rounds, to the
// first tuple that no item holds and no other mover has taken.  Purely combinatorial: tuples and the errors it is given are
// compared, no distance is computed.  include/lcrec.h, lcrec_finish_beam, is the contract; tests/beam_finish_ref.py restates it.
//
// Shape (every launch on the caller's stream, nothing read back):
//   1. the n held tuples and the M * W candidates are packed into the keys of tuple_key.h (a dead candidate gets key 0: it is never
//      looked up); both key sets are sorted once with rocPRIM, low word then high word (stable, so the pair is ordered);
//   2. mark: every candidate looks itself up in the sorted held keys (in O from the start: never proposed) and in the sorted
//      candidate keys: the lower bound there is its SLOT, which equal candidate tuples share;
//   3. keepers: one wave per shared tuple, a wave reduction on {ordered error bits, item id}; the others become movers;
//   4. W rounds of two launches.  propose: an unplaced mover advances past the candidates that are dead, held or in a claimed slot
//      and does an atomicMin of {ordered error bits, item id} on its slot.  resolve: the mover whose word the slot holds writes its
//      row, claims the slot and is placed; the others step on.  `claimed` is written by resolve and read by propose only, so a
//      round sees the occupied set as it stood when the round began;
//   5. unresolved = movers - moved.
// The only atomics are min (the slots), max (the round count) and integer add (the counters): the result does not depend on the
// order in which anything arrives.
//
// lcrec_extend_finish_beam: items with id < n_frozen never move and nothing of theirs is read from err_held, cand or cand_err.  Their
// held tuples are packed and sorted with the others (O is every tuple held); their candidates are packed as dead without a look at
// the row; in keepers a frozen holder is counted, takes no part in the reduction, and a group with one has no keeper.
#include "rq_walk.h"
#include "tuple_key.h"

#include <rocprim/device/device_radix_sort.hpp>

namespace lcrec {

constexpr int FB_THREADS = 256;
constexpr int FB_WAVES = FB_THREADS / 64;

// a mover's state in ptr[]: its pointer 0 .. W-1, W = its list is exhausted; the two below are no pointers
constexpr int FB_NO_MOVER = -1;
constexpr int FB_PLACED = 0x7fffffff;

struct BeamFinishParams {
    int64_t *idx;                  // [n][L]
    int64_t n, M, MW;              // items, members, members * width
    int W;
    int wide;                      // the key has a high word
    const int64_t *members, *offsets;
    const float *err_held;         // [M]
    const int64_t *cand;           // [M][W][L]
    const float *cand_err;         // [M][W]
    int *choice;                   // [M]
    unsigned long long *counters;  // {movers, moved, unresolved, rounds}
    const uint64_t *hlo, *hhi;     // [n] sorted held keys
    const uint64_t *clo, *chi;     // [MW] candidate keys, as packed
    const uint64_t *slo, *shi;     // [MW] sorted candidate keys
    int64_t *cslot;                // [MW] the candidate's slot, -1: dead or held from the start
    unsigned long long *best;      // [MW] per slot: the smallest {ordered error bits, item id} proposed
    unsigned char *claimed;        // [MW] per slot
    int *ptr;                      // [M]
};

__global__ void fb_pack_held_kernel(const int64_t *__restrict__ idx, int64_t n, PackDesc d, uint64_t *klo, uint64_t *khi)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned __int128 key = pack_tuple_key(idx + i * d.L, d);
    klo[i] = (uint64_t)key;
    khi[i] = (uint64_t)(key >> 64);
}

// a candidate with a code outside its level is dead
__device__ __forceinline__ bool fb_live(const int64_t *__restrict__ row, const PackDesc &d)
{
    bool live = true;
    for (int l = 0; l < d.L; ++l) live = live && row[l] >= 0 && row[l] < d.K[l];
    return live;
}

// The three kernels that know of frozen items are compiled twice: FROZEN = false is the code for n_frozen == 0, without a trace of
// them, and n_frozen is an argument of these three alone -- the 2 * width launches of the rounds take the arguments they took before
// there was a frozen form, and lcrec_finish_beam costs what it cost.
// the candidates of a frozen member are dead, whatever their rows hold: the row is not read.  W is 1, 2, 4 or 8: candidate c belongs
// to member c >> log2(W)
template <bool FROZEN>
__device__ __forceinline__ bool fb_owner_frozen(const int64_t *__restrict__ members, int64_t c, int W, int64_t n_frozen)
{
    if constexpr (!FROZEN) return false;
    else return members[c >> (__ffs(W) - 1)] < n_frozen;
}

// candidates: a dead one gets key 0 (any key will do: it is never looked up, and the sort only has to stay within the key's bits)
template <bool FROZEN>
__global__ void fb_pack_cand_kernel(const int64_t *__restrict__ cand, const int64_t *__restrict__ members, int64_t count, int W,
                                    int64_t n_frozen, PackDesc d, uint64_t *klo, uint64_t *khi)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= count) return;
    const int64_t *row = cand + c * d.L;
    const bool live = !fb_owner_frozen<FROZEN>(members, c, W, n_frozen) && fb_live(row, d);
    const unsigned __int128 key = live ? pack_tuple_key(row, d) : (unsigned __int128)0;
    klo[c] = (uint64_t)key;
    khi[c] = (uint64_t)(key >> 64);
}

// first position in the sorted keys (hi, lo) that is not below (khi, klo)
__device__ __forceinline__ int64_t fb_lower_bound(const uint64_t *lo, const uint64_t *hi, int wide, int64_t count, uint64_t klo, uint64_t khi)
{
    int64_t a = 0, b = count;
    while (a < b) {
        const int64_t m = a + ((b - a) >> 1);
        const bool below = wide ? (hi[m] < khi || (hi[m] == khi && lo[m] < klo)) : lo[m] < klo;
        if (below) a = m + 1; else b = m;
    }
    return a;
}

template <bool FROZEN>
__global__ void fb_mark_kernel(BeamFinishParams p, PackDesc d, int64_t n_frozen)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= p.MW) return;
    if (fb_owner_frozen<FROZEN>(p.members, c, p.W, n_frozen) || !fb_live(p.cand + c * d.L, d)) { p.cslot[c] = -1; return; }
    const uint64_t klo = p.clo[c], khi = p.wide ? p.chi[c] : 0;
    const int64_t h = fb_lower_bound(p.hlo, p.hhi, p.wide, p.n, klo, khi);
    if (h < p.n && p.hlo[h] == klo && (!p.wide || p.hhi[h] == khi)) { p.cslot[c] = -1; return; }   // some item holds it
    p.cslot[c] = fb_lower_bound(p.slo, p.shi, p.wide, p.MW, klo, khi);
}

__global__ void fb_init_kernel(BeamFinishParams p)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= p.M) return;
    p.ptr[j] = FB_NO_MOVER;
    p.choice[j] = -1;
}

// one wave per group, as spill_keepers_kernel: the keeper is a wave reduction on {ordered error bits, item id} over the NEW holders;
// frozen holders are counted only, and one of them leaves the group without a keeper (ki stays ~0u, which is no item id: n < 2^32)
template <bool FROZEN>
__global__ __launch_bounds__(FB_THREADS) void fb_keepers_kernel(BeamFinishParams p, int64_t n_groups, int64_t n_frozen)
{
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * FB_WAVES + (threadIdx.x >> 6);
    if (g >= n_groups) return;                                                    // (the whole wave)
    int64_t lo = p.offsets[g], hi = p.offsets[g + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > p.M ? p.M : hi;                                                     // nothing past the member table is touched

    uint32_t kd = ~0u, ki = ~0u;
    int holders = 0, frozen = 0;
    for (int64_t pos = lo + lane; pos < hi; pos += 64) {
        const int64_t id = p.members[pos];
        if (id < 0 || id >= p.n) continue;
        ++holders;
        if (FROZEN && id < n_frozen) { ++frozen; continue; }                      // (err_held[pos] is not read)
        const uint32_t d = ordered_bits(p.err_held[pos]);
        if (d < kd || (d == kd && (uint32_t)id < ki)) { kd = d; ki = (uint32_t)id; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t od = __shfl_xor(kd, o, 64), oi = __shfl_xor(ki, o, 64);
        if (od < kd || (od == kd && oi < ki)) { kd = od; ki = oi; }
        holders += __shfl_xor(holders, o, 64);
        if (FROZEN) frozen += __shfl_xor(frozen, o, 64);
    }
    if (holders < 2 || frozen == holders) return;                                 // (no new holder: no mover)
    if (frozen > 0) ki = ~0u;
    for (int64_t pos = lo + lane; pos < hi; pos += 64) {
        const int64_t id = p.members[pos];
        if ((FROZEN && id < n_frozen) || id < 0 || id >= p.n || (uint32_t)id == ki) continue;
        p.ptr[pos] = 0;
        p.choice[pos] = -2;
    }
    if (lane == 0) atomicAdd(&p.counters[0], (unsigned long long)(holders - frozen - (frozen > 0 ? 0 : 1)));
}

__device__ __forceinline__ unsigned long long fb_word(float err, int64_t id)
{
    return ((unsigned long long)ordered_bits(err) << 32) | (unsigned long long)(uint32_t)id;
}

__global__ void fb_propose_kernel(BeamFinishParams p)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= p.M) return;
    int q = p.ptr[j];
    if (q < 0 || q >= p.W) return;                                                // no mover, exhausted or placed
    const int64_t *slot = p.cslot + j * p.W;
    while (q < p.W && (slot[q] < 0 || p.claimed[slot[q]])) ++q;
    p.ptr[j] = q;
    if (q < p.W) atomicMin(&p.best[slot[q]], fb_word(p.cand_err[j * p.W + q], p.members[j]));
}

__global__ void fb_resolve_kernel(BeamFinishParams p, int L, int round)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= p.M) return;
    const int q = p.ptr[j];
    if (q < 0 || q >= p.W) return;
    const int64_t s = p.cslot[j * p.W + q], id = p.members[j];
    if (p.best[s] != fb_word(p.cand_err[j * p.W + q], id)) { p.ptr[j] = q + 1; return; }
    const int64_t *row = p.cand + (j * p.W + q) * L;
    for (int l = 0; l < L; ++l) p.idx[id * L + l] = row[l];
    p.claimed[s] = 1;
    p.choice[j] = q;
    p.ptr[j] = FB_PLACED;
    atomicAdd(&p.counters[1], 1ULL);
    atomicMax(&p.counters[3], (unsigned long long)(round + 1));
}

__global__ void fb_finalize_kernel(unsigned long long *counters) { counters[2] = counters[0] - counters[1]; }

static size_t fb_sort_temp_bytes(int64_t count)
{
    size_t a = 0;
    (void)rocprim::radix_sort_pairs(nullptr, a, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t *)nullptr,
                                    (size_t)count, 0, 64, (hipStream_t)0, false);
    // the size query needs a device; without one (build host) fall back to a generous bound
    if (a < 256) a = (size_t)count * 32 + (1u << 20);
    return align_up(a, 256) + 256;
}

// include/lcrec.h states this layout
struct BeamFinishPlan {
    int bits[LCREC_MAX_LEVELS];
    int total_bits, lo_bits, hi_bits;
    int64_t mw;
    size_t stride_n, stride_c, claimed_bytes, ptr_bytes, temp_bytes, workspace_bytes;
};

static int finish_beam_plan(const char *who, int64_t n, int64_t n_members, int L, const int *K, int width, BeamFinishPlan *p)
{
    *p = BeamFinishPlan{};
    if (L < 1 || L > LCREC_MAX_LEVELS) return fail(LCREC_EINVAL, "%s: L=%d (1 .. %d)", who, L, LCREC_MAX_LEVELS);
    if (n < 0 || n > 0xffffffffLL) return fail(LCREC_EINVAL, "%s: n=%lld (0 .. 2^32 - 1)", who, (long long)n);
    if (n_members < 0 || n_members > 0xffffffffLL)
        return fail(LCREC_EINVAL, "%s: n_members=%lld (0 .. 2^32 - 1)", who, (long long)n_members);
    if (width != 1 && width != 2 && width != 4 && width != 8) return fail(LCREC_EINVAL, "%s: width=%d (supported: 1, 2, 4, 8)", who, width);
    if (K) {
        for (int l = 0; l < L; ++l)
            if (K[l] < 1) return fail(LCREC_EINVAL, "%s: K[%d]=%d", who, l, K[l]);
        p->total_bits = key_bits(K, L, p->bits);
        if (p->total_bits > 128) return fail(LCREC_EUNSUPPORTED, "%s: tuples need %d bits (> 128)", who, p->total_bits);
    }
    p->lo_bits = p->total_bits > 64 ? 64 : (p->total_bits > 0 ? p->total_bits : 1);
    p->hi_bits = p->total_bits > 64 ? p->total_bits - 64 : 0;
    p->mw = n_members * width;
    const int64_t items = n > 0 ? n : 1, cands = p->mw > 0 ? p->mw : 1;
    p->stride_n = align_up((size_t)items * 8, 256);
    p->stride_c = align_up((size_t)cands * 8, 256);
    p->claimed_bytes = align_up((size_t)cands, 256);
    p->ptr_bytes = align_up((size_t)(n_members > 0 ? n_members : 1) * 4, 256);
    p->temp_bytes = fb_sort_temp_bytes(items > cands ? items : cands);
    p->workspace_bytes = 6 * p->stride_n + 6 * p->stride_c + p->claimed_bytes + p->ptr_bytes + p->temp_bytes;
    return LCREC_OK;
}

static const char *fb_who(bool frozen) { return frozen ? "extend_finish_beam" : "finish_beam"; }

size_t finish_beam_workspace(bool frozen, int64_t n, int64_t n_members, int L, int width)
{
    BeamFinishPlan p;   // (the sizes do not depend on the key)
    return finish_beam_plan(fb_who(frozen), n, n_members, L, nullptr, width, &p) == LCREC_OK ? p.workspace_bytes : 0;
}

// (lo, hi) -> (out_lo, out_hi) ordered by the pair: a stable sort by the low word, then (a key wider than 64 bits) by the high word
static hipError_t fb_sort_keys(const BeamFinishPlan &plan, uint64_t *lo, uint64_t *hi, uint64_t *tmp_lo, uint64_t *tmp_hi, uint64_t *out_lo,
                               uint64_t *out_hi, int64_t count, void *temp, hipStream_t stream)
{
    size_t tb = plan.temp_bytes;
    if (plan.hi_bits == 0) return rocprim::radix_sort_keys(temp, tb, lo, out_lo, (size_t)count, 0, plan.lo_bits, stream, false);
    hipError_t he = rocprim::radix_sort_pairs(temp, tb, lo, tmp_lo, hi, tmp_hi, (size_t)count, 0, plan.lo_bits, stream, false);
    if (he != hipSuccess) return he;
    tb = plan.temp_bytes;
    return rocprim::radix_sort_pairs(temp, tb, tmp_hi, out_hi, tmp_lo, out_lo, (size_t)count, 0, plan.hi_bits, stream, false);
}

// Both entries: `frozen` selects lcrec_extend_finish_beam's checks, texts and trace name.
int finish_beam(bool frozen, int64_t *idx, int64_t n, int64_t n_frozen, int L, const int *K, const int64_t *tuple_members,
                const int64_t *tuple_offsets, int64_t n_groups, int64_t n_members, const float *err_held, const int64_t *cand,
                const float *cand_err, int width, int *choice_out, int64_t *counters_out, void *workspace, size_t workspace_bytes,
                hipStream_t stream)
{
    const char *who = fb_who(frozen);
    if (int rc = first_null(who, {{counters_out, "counters_out"}, {K, "K"}})) return rc;
    if (n_groups < 0 || n_groups > 0x7fffffffLL)
        return fail(LCREC_EINVAL, "%s: n_tuple_groups=%lld (0 .. 2^31 - 1)", who, (long long)n_groups);
    BeamFinishPlan plan;
    if (int rc = finish_beam_plan(who, n, n_members, L, K, width, &plan)) return rc;
    if (n_frozen < 0 || n_frozen > n) return fail(LCREC_EINVAL, "%s: n_frozen=%lld (0 .. n=%lld)", who, (long long)n_frozen, (long long)n);
    if (((uintptr_t)idx | (uintptr_t)tuple_members | (uintptr_t)tuple_offsets | (uintptr_t)cand | (uintptr_t)counters_out |
         (uintptr_t)workspace) & 7)
        return fail(LCREC_EINVAL, "%s: idx, tuple_members, tuple_offsets, cand, counters_out and workspace must be 8-byte aligned", who);
    if (((uintptr_t)err_held | (uintptr_t)cand_err | (uintptr_t)choice_out) & 3)
        return fail(LCREC_EINVAL, "%s: err_held, cand_err and choice_out must be 4-byte aligned", who);
    const bool work = n_groups > 0 && n_members > 0 && n > 0 && n_frozen < n;
    if (work) {
        if (int rc = first_null(who, {{idx, "idx"}, {tuple_members, "tuple_members"}, {tuple_offsets, "tuple_offsets"},
                                      {err_held, "err_held"}, {cand, "cand"}, {cand_err, "cand_err"}, {choice_out, "choice_out"}}))
            return rc;
        if (!workspace || workspace_bytes < plan.workspace_bytes)
            return fail(LCREC_EWORKSPACE, "%s: workspace of %zu bytes, %zu needed (lcrec_%s_workspace)", who,
                        workspace ? workspace_bytes : (size_t)0, plan.workspace_bytes, who);
    }
    hipError_t he = hipMemsetAsync(counters_out, 0, 4 * sizeof(int64_t), stream);
    if (he != hipSuccess) return fail(LCREC_EHIP, "%s: %s", who, hipGetErrorString(he));
    if (!work) return LCREC_OK;   // (no shared tuple, or no new item: nothing can move)

    PackDesc d;
    d.L = L;
    for (int l = 0; l < L; ++l) {
        d.bits[l] = plan.bits[l];
        d.K[l] = K[l];
    }
    char *ws = reinterpret_cast<char *>(workspace);
    auto take = [&](size_t bytes) { char *q = ws; ws += bytes; return q; };
    uint64_t *h[6], *c[6];   // {packed lo, packed hi, between the sorts lo, hi, sorted lo, sorted hi}
    for (auto &a : h) a = (uint64_t *)take(plan.stride_n);
    for (auto &a : c) a = (uint64_t *)take(plan.stride_c);
    unsigned char *claimed = (unsigned char *)take(plan.claimed_bytes);
    int *ptr = (int *)take(plan.ptr_bytes);
    void *temp = ws;

    BeamFinishParams p;
    p.idx = idx; p.n = n; p.M = n_members; p.MW = plan.mw; p.W = width; p.wide = plan.hi_bits > 0;
    p.members = tuple_members; p.offsets = tuple_offsets;
    p.err_held = err_held; p.cand = cand; p.cand_err = cand_err;
    p.choice = choice_out;
    p.counters = reinterpret_cast<unsigned long long *>(counters_out);
    p.hlo = h[4]; p.hhi = h[5];
    p.clo = c[0]; p.chi = c[1];
    p.slo = c[4]; p.shi = c[5];
    // the two arrays between the sorts are free once the keys are sorted: the slots and their words live there
    p.cslot = reinterpret_cast<int64_t *>(c[2]);
    p.best = reinterpret_cast<unsigned long long *>(c[3]);
    p.claimed = claimed;
    p.ptr = ptr;

    const unsigned grid_n = (unsigned)((n + FB_THREADS - 1) / FB_THREADS);
    const unsigned grid_c = (unsigned)((plan.mw + FB_THREADS - 1) / FB_THREADS);
    const unsigned grid_m = (unsigned)((n_members + FB_THREADS - 1) / FB_THREADS);
    const unsigned grid_g = (unsigned)((n_groups + FB_WAVES - 1) / FB_WAVES);
    TraceScope trace(frozen ? K_EXTEND_FINISH_BEAM : K_FINISH_BEAM, stream);
    hipLaunchKernelGGL(fb_pack_held_kernel, dim3(grid_n), dim3(FB_THREADS), 0, stream, idx, n, d, h[0], h[1]);
    he = fb_sort_keys(plan, h[0], h[1], h[2], h[3], h[4], h[5], n, temp, stream);
    if (he != hipSuccess) return fail(LCREC_EHIP, "%s: sort: %s", who, hipGetErrorString(he));
    const bool fz = n_frozen > 0;
    hipLaunchKernelGGL(fz ? fb_pack_cand_kernel<true> : fb_pack_cand_kernel<false>, dim3(grid_c), dim3(FB_THREADS), 0, stream, cand,
                       tuple_members, plan.mw, width, n_frozen, d, c[0], c[1]);
    he = fb_sort_keys(plan, c[0], c[1], c[2], c[3], c[4], c[5], plan.mw, temp, stream);
    if (he != hipSuccess) return fail(LCREC_EHIP, "%s: sort: %s", who, hipGetErrorString(he));
    he = hipMemsetAsync(p.best, 0xff, (size_t)plan.mw * 8, stream);
    if (he == hipSuccess) he = hipMemsetAsync(claimed, 0, (size_t)plan.mw, stream);
    if (he != hipSuccess) return fail(LCREC_EHIP, "%s: %s", who, hipGetErrorString(he));
    hipLaunchKernelGGL(fz ? fb_mark_kernel<true> : fb_mark_kernel<false>, dim3(grid_c), dim3(FB_THREADS), 0, stream, p, d,
                       n_frozen);
    hipLaunchKernelGGL(fb_init_kernel, dim3(grid_m), dim3(FB_THREADS), 0, stream, p);
    hipLaunchKernelGGL(fz ? fb_keepers_kernel<true> : fb_keepers_kernel<false>, dim3(grid_g), dim3(FB_THREADS), 0, stream, p, n_groups,
                       n_frozen);
    // the fixed `width` rounds, whatever happens in them: a round without a proposer does nothing, and nothing is read back
    for (int r = 0; r < width; ++r) {
        hipLaunchKernelGGL(fb_propose_kernel, dim3(grid_m), dim3(FB_THREADS), 0, stream, p);
        hipLaunchKernelGGL(fb_resolve_kernel, dim3(grid_m), dim3(FB_THREADS), 0, stream, p, L, r);
    }
    hipLaunchKernelGGL(fb_finalize_kernel, dim3(1), dim3(1), 0, stream, p.counters);
    return check_launch(frozen ? "extend_finish_beam kernels" : "finish_beam kernels");
}

}  // namespace lcrec
