// Index trie: the prefix trie over the tuples of an index matrix (lcrec_index_trie_build), longest-prefix descent through it
// (lcrec_index_trie_find) and the constrained-decoding mask of a [beams, vocab] logits matrix (lcrec_index_trie_mask_logits).
// Beyond the reference, whose data.py:67-89 keeps one set of allowed tokens per position and whose index/ stage has no way back
// from a tuple to its items.  include/lcrec.h states the three rules and the layout of lcrec_index_trie; tests/trie_ref.py
// restates them in numpy.
//
// Build (all on device, O(n) memory): the keys of tuple_key.h, a stable LSD radix sort of (key, id) as in collide.hip -- the low
// word, then the high word of keys wider than 64 bits; the last pass writes straight into trie->order --, then
//   trie_prefix_kernel   every sorted item's common-prefix length with its predecessor, in levels (-1 for the first item, so that
//                        "a node of depth d starts at sorted position i" is cpl[i] < d at every depth, 0 included), and the
//                        sorted keys side by side for the level passes
//   per depth d = 1..L   an inclusive scan of the flags cpl[i] < d (a transform iterator: no flag array) numbers the nodes of depth
//                        d, and trie_level_kernel scatters: the node's last code, its parent's first-child link (the previous
//                        depth's scan is kept: two scan buffers alternate), at depth L the leaf's first position; the last
//                        sorted item writes counts[d] and the sentinels.
//
// Find: a lane per row; at most `depth` binary searches over a node's contiguous, ascending child codes.
//
// Mask (the hot path; it only stores): a grid of (chunk of MASK_CHUNK columns, row).  A workgroup clears a bitmap of its chunk in
// LDS, marks the allowed tokens that fall into the chunk from the node's at most K[depth] children (or eos), and then walks the
// chunk in groups of four columns that start on a 16-byte boundary of the ROW'S ADDRESS: bit i of the bitmap is column
// c0 - s + i with s = (row address / 4 + c0) mod 4, so a group is one nibble of one word.  A whole group with an empty nibble is one
// 16-byte store of -inf, consecutive lanes store consecutive groups (a wave: 1 KB in a row); a group with an allowed column, and the
// partial groups at the chunk's two ends, go column by column.  logits is never loaded.
#include "tuple_key.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace lcrec {

constexpr int TRIE_THREADS = 256;
constexpr int MASK_THREADS = 256;
constexpr int MASK_CHUNK = 4096;                        // columns per workgroup: 16 KB of stores
constexpr int MASK_WORDS = (MASK_CHUNK + 4 + 31) / 32;  // bitmap words: the chunk and the up to 3 bits before its first column
constexpr int MASK_MAX_ROWS = 65535;                    // grid.y; a row loop does the rest
constexpr int TRIE_ARRAYS = 11;                         // n-element arrays in the build's workspace

struct KeyLayout {
    PackDesc d;
    int total_bits;
};

__global__ void trie_pack_kernel(const int64_t *__restrict__ idx, int64_t idx_stride, int64_t n, PackDesc d, uint64_t *klo,
                                 uint64_t *khi, int64_t *ids)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned __int128 key = pack_tuple_key(idx + i * idx_stride, d);
    klo[i] = (uint64_t)key;
    khi[i] = (uint64_t)(key >> 64);
    ids[i] = i;
}

__global__ void trie_gather_kernel(const uint64_t *src, const int64_t *ids, int64_t n, uint64_t *dst)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[ids[i]];
}

__global__ void trie_prefix_kernel(const uint64_t *__restrict__ klo, const uint64_t *__restrict__ khi, const int64_t *__restrict__ order,
                                   int64_t n, KeyLayout k, uint64_t *sklo, uint64_t *skhi, int *cpl)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t a = order[i];
    const uint64_t alo = klo[a], ahi = khi[a];
    sklo[i] = alo;
    skhi[i] = ahi;
    int c = -1;
    if (i > 0) {
        const int64_t b = order[i - 1];
        const uint64_t xlo = alo ^ klo[b], xhi = ahi ^ khi[b];
        c = k.d.L;
        if (xlo | xhi) {
            const int top = xhi ? 127 - __builtin_clzll(xhi) : 63 - __builtin_clzll(xlo);   // the highest differing bit
            int shift = k.total_bits;
            for (int l = 0; l < k.d.L; ++l) {
                shift -= k.d.bits[l];
                if (k.d.bits[l] > 0 && shift <= top) { c = l; break; }                      // the level that holds it
            }
        }
    }
    cpl[i] = c;
}

struct StartsAt {
    int d;
    __device__ __host__ int64_t operator()(int c) const { return c < d ? 1 : 0; }
};

struct LevelParams {
    int64_t n;
    int d, L;              // the depth being filled, 1 .. L
    int shift, bits;       // where level d-1 lies in the key
    const int *cpl;
    const int64_t *scan_prev, *scan_cur;   // 1-based node numbers at depth d-1 (unused at d == 1) and d
    const uint64_t *sklo, *skhi;
    int64_t *counts, *child, *first;
    int *code;
};

__global__ void trie_level_kernel(LevelParams p)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n) return;
    const int64_t cur = p.scan_cur[i] - 1;
    const int c = p.cpl[i];
    if (c < p.d) {                                           // a node of depth d starts here
        const unsigned __int128 key = ((unsigned __int128)p.skhi[i] << 64) | p.sklo[i];
        p.code[(int64_t)(p.d - 1) * p.n + cur] = (int)((uint64_t)(key >> p.shift) & ((1ULL << p.bits) - 1ULL));
        if (p.d == p.L) p.first[cur] = i;
    }
    if (c < p.d - 1) {                                       // ... and one of depth d-1: cur is its first child
        const int64_t parent = p.d == 1 ? 0 : p.scan_prev[i] - 1;
        p.child[(int64_t)(p.d - 1) * (p.n + 1) + parent] = cur;
    }
    if (i == p.n - 1) {
        const int64_t parents = p.d == 1 ? 1 : p.scan_prev[i];
        p.counts[p.d] = cur + 1;
        p.child[(int64_t)(p.d - 1) * (p.n + 1) + parents] = cur + 1;
        if (p.d == 1) p.counts[0] = 1;
        if (p.d == p.L) p.first[cur + 1] = p.n;
    }
}

__global__ void trie_find_kernel(lcrec_index_trie t, const int64_t *__restrict__ prefix, int64_t prefix_stride, int64_t B, int depth,
                                 int64_t *node_out, int *depth_out)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int64_t node = 0;
    int d = 0;
    for (; d < depth && t.n > 0; ++d) {
        const int64_t c = prefix[b * prefix_stride + d];
        if (c < 0 || c >= t.K[d]) break;
        const int64_t *row = t.child + (int64_t)d * (t.n + 1);
        const int *codes = t.code + (int64_t)d * t.n;
        int64_t lo = row[node], hi = row[node + 1];
        while (lo < hi) {                                    // the first child whose code is >= c
            const int64_t mid = lo + (hi - lo) / 2;
            if (codes[mid] < (int)c) lo = mid + 1; else hi = mid;
        }
        if (lo >= row[node + 1] || codes[lo] != (int)c) break;
        node = lo;
    }
    if (depth_out) {
        node_out[b] = node;
        depth_out[b] = d;
    } else {
        node_out[b] = d == depth ? node : -1;
    }
}

__global__ __launch_bounds__(MASK_THREADS) void trie_mask_kernel(lcrec_index_trie t, const int64_t *__restrict__ node, int64_t B,
                                                                   int depth, const int *__restrict__ token_ids, int eos,
                                                                   float *__restrict__ logits, int64_t ld, int64_t V)
{
    __shared__ unsigned bitmap[MASK_WORDS];
    const int tid = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * MASK_CHUNK;
    const int len = (int)(V - c0 < MASK_CHUNK ? V - c0 : MASK_CHUNK);     // columns [c0, c0 + len), len >= 1
    const float ninf = -__builtin_inff();
    const f32x4 ninf4 = {ninf, ninf, ninf, ninf};
    for (int64_t b = blockIdx.y; b < B; b += gridDim.y) {
        float *row = logits + b * ld;
        const int s = (int)((((uintptr_t)row >> 2) + (uintptr_t)c0) & 3);   // bit i of the bitmap is column c0 - s + i
        if (tid < MASK_WORDS) bitmap[tid] = 0u;
        __syncthreads();
        const int64_t at = node[b];
        if (depth < t.L && at >= 0 && at < t.counts[depth]) {
            int64_t lo = 0, hi = 0;
            if (t.n > 0) {
                lo = t.child[(int64_t)depth * (t.n + 1) + at];
                hi = t.child[(int64_t)depth * (t.n + 1) + at + 1];
            }
            const int *codes = t.code + (int64_t)depth * t.n;
            for (int64_t k = lo + tid; k < hi; k += MASK_THREADS) {
                const int c = codes[k];
                const int64_t tok = token_ids ? token_ids[c] : c;
                if (tok >= c0 && tok < c0 + len) {
                    const int bit = (int)(tok - c0) + s;
                    atomicOr(&bitmap[bit >> 5], 1u << (bit & 31));
                }
            }
        } else if (tid == 0 && eos >= c0 && eos < c0 + len) {
            const int bit = (int)(eos - c0) + s;
            bitmap[bit >> 5] |= 1u << (bit & 31);
        }
        __syncthreads();
        float *base = row + c0 - s;                          // 16-byte aligned; columns before c0 are never stored to
        const int end = s + len;
        for (int i = 4 * tid; i < end; i += 4 * MASK_THREADS) {
            const unsigned nib = (bitmap[i >> 5] >> (i & 31)) & 15u;
            if (i >= s && i + 4 <= end && nib == 0u) {
                *reinterpret_cast<f32x4 *>(base + i) = ninf4;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (i + j >= s && i + j < end && !((nib >> j) & 1u)) base[i + j] = ninf;
            }
        }
        __syncthreads();                                     // the bitmap is cleared for the next row
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
static size_t trie_temp_bytes(int64_t n)
{
    size_t a = 0, b = 0;
    (void)rocprim::radix_sort_pairs(nullptr, a, (uint64_t *)nullptr, (uint64_t *)nullptr, (int64_t *)nullptr, (int64_t *)nullptr,
                                    (size_t)n, 0, 64, (hipStream_t)0, false);
    (void)rocprim::inclusive_scan(nullptr, b, rocprim::make_transform_iterator((const int *)nullptr, StartsAt{1}), (int64_t *)nullptr,
                                  (size_t)n, rocprim::plus<int64_t>(), (hipStream_t)0, false);
    size_t m = a > b ? a : b;
    // the size query needs a device; without one (build host) fall back to a generous bound
    const size_t floor_bytes = (size_t)n * 32 + (1u << 20);
    if (m < 256) m = floor_bytes;
    return align_up(m, 256) + 256;
}

static bool aligned_to(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// n, L and K of a build, or of a trie handed to find / mask
static int check_shape(const char *who, int64_t n, int L, const int *K, int *bits, int *total_bits)
{
    if (L < 1 || L > LCREC_MAX_LEVELS) return fail(LCREC_EINVAL, "%s: L=%d outside 1 .. %d", who, L, LCREC_MAX_LEVELS);
    if (n < 0) return fail(LCREC_EINVAL, "%s: n=%lld", who, (long long)n);
    for (int l = 0; l < L; ++l)
        if (K[l] < 1) return fail(LCREC_EINVAL, "%s: K[%d]=%d", who, l, K[l]);
    *total_bits = key_bits(K, L, bits);
    if (*total_bits > 128) return fail(LCREC_EINVAL, "%s: tuples need %d key bits (> 128)", who, *total_bits);
    return LCREC_OK;
}

static int check_trie(const char *who, const lcrec_index_trie *t)
{
    if (!t) return fail(LCREC_EINVAL, "%s: trie is NULL", who);
    if (int rc = first_null(who, {{t->order, "trie->order"}, {t->counts, "trie->counts"}, {t->child, "trie->child"},
                                  {t->code, "trie->code"}, {t->first, "trie->first"}}))
        return rc;
    if (!aligned_to(t->order, 8) || !aligned_to(t->counts, 8) || !aligned_to(t->child, 8) || !aligned_to(t->first, 8))
        return fail(LCREC_EINVAL, "%s: trie->order, counts, child and first must be 8-byte aligned", who);
    if (!aligned_to(t->code, 4)) return fail(LCREC_EINVAL, "%s: trie->code must be 4-byte aligned", who);
    return LCREC_OK;
}

static int check_built_trie(const char *who, const lcrec_index_trie *t)
{
    if (int rc = check_trie(who, t)) return rc;
    int bits[LCREC_MAX_LEVELS], total = 0;
    return check_shape(who, t->n, t->L, t->K, bits, &total);
}

static int64_t trie_stride(int64_t n) { return (int64_t)align_up((size_t)n * 8, 256); }

size_t index_trie_build_workspace(int64_t n, int L)
{
    if (n < 0 || L < 1 || L > LCREC_MAX_LEVELS) return 0;
    if (n == 0) return 0;
    return (size_t)TRIE_ARRAYS * (size_t)trie_stride(n) + trie_temp_bytes(n);
}

int index_trie_build(const int64_t *idx, int64_t idx_stride, int64_t n, int L, const int *K, lcrec_index_trie *trie, void *workspace,
                     size_t workspace_bytes, hipStream_t stream)
{
    const char *who = "trie_build";
    if (!K) return fail(LCREC_EINVAL, "%s: K is NULL", who);
    KeyLayout k{};
    if (int rc = check_shape(who, n, L, K, k.d.bits, &k.total_bits)) return rc;
    if (idx_stride < 0 || (idx_stride != 0 && idx_stride < L))
        return idx_stride < 0 ? fail(LCREC_EINVAL, "%s: idx_stride=%lld", who, (long long)idx_stride)
                              : fail(LCREC_EINVAL, "%s: idx_stride=%lld < L=%d", who, (long long)idx_stride, L);
    if (n > 0 && !idx) return fail(LCREC_EINVAL, "%s: idx is NULL", who);
    if (!aligned_to(idx, 8)) return fail(LCREC_EINVAL, "%s: idx must be 8-byte aligned", who);
    if (int rc = check_trie(who, trie)) return rc;
    if (!aligned_to(workspace, 16)) return fail(LCREC_EINVAL, "%s: workspace must be 16-byte aligned", who);
    const size_t need = index_trie_build_workspace(n, L);
    if (need && (!workspace || workspace_bytes < need))
        return fail(LCREC_EWORKSPACE, "%s: workspace of %zu bytes, %zu needed (lcrec_index_trie_build_workspace)", who,
                    workspace ? workspace_bytes : (size_t)0, need);
    k.d.L = L;
    trie->n = n;
    trie->L = L;
    for (int l = 0; l < LCREC_MAX_LEVELS; ++l) {
        trie->K[l] = l < L ? K[l] : 0;
        k.d.K[l] = l < L ? K[l] : 0;
    }
    if (idx_stride == 0) idx_stride = L;

    hipError_t he;
    if (n == 0) {                                            // counts = {1, 0, ...}, child[d][0] = 0, first[0] = 0: no launch
        he = hipMemsetAsync(trie->counts, 0, (size_t)(L + 1) * sizeof(int64_t), stream);
        if (he == hipSuccess) he = hipMemsetAsync(trie->counts, 1, 1, stream);               // (little endian: the int64 1)
        if (he == hipSuccess) he = hipMemsetAsync(trie->child, 0, (size_t)L * sizeof(int64_t), stream);
        if (he == hipSuccess) he = hipMemsetAsync(trie->first, 0, sizeof(int64_t), stream);
        return he == hipSuccess ? LCREC_OK : fail(LCREC_EHIP, "%s: %s", who, hipGetErrorString(he));
    }

    const size_t arr = (size_t)trie_stride(n);
    char *ws = reinterpret_cast<char *>(workspace);
    auto take = [&]() { char *p = ws; ws += arr; return p; };
    uint64_t *klo = (uint64_t *)take(), *khi = (uint64_t *)take(), *ka = (uint64_t *)take(), *kb = (uint64_t *)take();
    int64_t *ia = (int64_t *)take(), *ib = (int64_t *)take();
    uint64_t *sklo = (uint64_t *)take(), *skhi = (uint64_t *)take();
    int *cpl = (int *)take();
    int64_t *scan[2] = {(int64_t *)take(), (int64_t *)take()};
    void *temp = ws;
    const size_t temp_bytes = need - (size_t)TRIE_ARRAYS * arr;
    const int lo_bits = k.total_bits > 64 ? 64 : (k.total_bits > 0 ? k.total_bits : 1);
    const int hi_bits = k.total_bits > 64 ? k.total_bits - 64 : 0;

    const unsigned grid = (unsigned)((n + TRIE_THREADS - 1) / TRIE_THREADS);
    TraceScope trace(K_TRIE_BUILD, stream);
    hipLaunchKernelGGL(trie_pack_kernel, dim3(grid), dim3(TRIE_THREADS), 0, stream, idx, idx_stride, n, k.d, klo, khi, ia);
    // stable sort by the low word, then (if the tuple is wider than 64 bits) by the high word; the last pass lands in trie->order
    size_t tb = temp_bytes;
    he = rocprim::radix_sort_pairs(temp, tb, klo, ka, ia, hi_bits ? ib : trie->order, (size_t)n, 0, lo_bits, stream, false);
    if (he != hipSuccess) return fail(LCREC_EHIP, "%s: sort: %s", who, hipGetErrorString(he));
    if (hi_bits) {
        hipLaunchKernelGGL(trie_gather_kernel, dim3(grid), dim3(TRIE_THREADS), 0, stream, khi, ib, n, ka);
        tb = temp_bytes;
        he = rocprim::radix_sort_pairs(temp, tb, ka, kb, ib, trie->order, (size_t)n, 0, hi_bits, stream, false);
        if (he != hipSuccess) return fail(LCREC_EHIP, "%s: sort: %s", who, hipGetErrorString(he));
    }
    hipLaunchKernelGGL(trie_prefix_kernel, dim3(grid), dim3(TRIE_THREADS), 0, stream, klo, khi, trie->order, n, k, sklo, skhi, cpl);
    int shift = k.total_bits;
    for (int d = 1; d <= L; ++d) {
        shift -= k.d.bits[d - 1];
        tb = temp_bytes;
        he = rocprim::inclusive_scan(temp, tb, rocprim::make_transform_iterator((const int *)cpl, StartsAt{d}), scan[d & 1], (size_t)n,
                                     rocprim::plus<int64_t>(), stream, false);
        if (he != hipSuccess) return fail(LCREC_EHIP, "%s: scan: %s", who, hipGetErrorString(he));
        LevelParams p;
        p.n = n; p.d = d; p.L = L; p.shift = shift; p.bits = k.d.bits[d - 1];
        p.cpl = cpl; p.scan_prev = scan[(d - 1) & 1]; p.scan_cur = scan[d & 1]; p.sklo = sklo; p.skhi = skhi;
        p.counts = trie->counts; p.child = trie->child; p.first = trie->first; p.code = trie->code;
        hipLaunchKernelGGL(trie_level_kernel, dim3(grid), dim3(TRIE_THREADS), 0, stream, p);
    }
    return check_launch("trie_build kernels");
}

int index_trie_find(const lcrec_index_trie *trie, const int64_t *prefix, int64_t prefix_stride, int64_t B, int depth, int64_t *node_out,
                    int *depth_out, hipStream_t stream)
{
    const char *who = "trie_find";
    if (int rc = check_built_trie(who, trie)) return rc;
    if (B < 0) return fail(LCREC_EINVAL, "%s: B=%lld", who, (long long)B);
    if (depth < 0 || depth > trie->L) return fail(LCREC_EINVAL, "%s: depth=%d outside [0, L=%d]", who, depth, trie->L);
    if (prefix_stride < 0 || (prefix_stride != 0 && prefix_stride < depth))
        return prefix_stride < 0 ? fail(LCREC_EINVAL, "%s: prefix_stride=%lld", who, (long long)prefix_stride)
                                 : fail(LCREC_EINVAL, "%s: prefix_stride=%lld < depth=%d", who, (long long)prefix_stride, depth);
    if (B > 0 && depth > 0 && !prefix) return fail(LCREC_EINVAL, "%s: prefix is NULL", who);
    if (B > 0 && !node_out) return fail(LCREC_EINVAL, "%s: node_out is NULL", who);
    if (!aligned_to(prefix, 8) || !aligned_to(node_out, 8)) return fail(LCREC_EINVAL, "%s: prefix and node_out must be 8-byte aligned", who);
    if (!aligned_to(depth_out, 4)) return fail(LCREC_EINVAL, "%s: depth_out must be 4-byte aligned", who);
    if (B == 0) return LCREC_OK;
    if (prefix_stride == 0) prefix_stride = depth;
    const int64_t blocks = (B + TRIE_THREADS - 1) / TRIE_THREADS;
    if (blocks > 0x7fffffffLL) return fail(LCREC_EINVAL, "%s: B=%lld is more than one launch holds", who, (long long)B);
    TraceScope trace(K_TRIE_FIND, stream);
    hipLaunchKernelGGL(trie_find_kernel, dim3((unsigned)blocks), dim3(TRIE_THREADS), 0, stream, *trie, prefix, prefix_stride, B, depth,
                       node_out, depth_out);
    return check_launch("trie_find_kernel");
}

int index_trie_mask_logits(const lcrec_index_trie *trie, const int64_t *node, int64_t B, int depth, const int *token_ids, int eos,
                           float *logits, int64_t ld, int64_t V, hipStream_t stream)
{
    const char *who = "trie_mask";
    if (int rc = check_built_trie(who, trie)) return rc;
    if (B < 0) return fail(LCREC_EINVAL, "%s: B=%lld", who, (long long)B);
    if (depth < 0 || depth > trie->L) return fail(LCREC_EINVAL, "%s: depth=%d outside [0, L=%d]", who, depth, trie->L);
    if (V < 1) return fail(LCREC_EINVAL, "%s: V=%lld", who, (long long)V);
    if (ld < V) return fail(LCREC_EINVAL, "%s: ld=%lld < V=%lld", who, (long long)ld, (long long)V);
    if (B > 0 && !node) return fail(LCREC_EINVAL, "%s: node is NULL", who);
    if (B > 0 && !logits) return fail(LCREC_EINVAL, "%s: logits is NULL", who);
    if (!aligned_to(node, 8)) return fail(LCREC_EINVAL, "%s: node must be 8-byte aligned", who);
    if (!aligned_to(logits, 4) || !aligned_to(token_ids, 4)) return fail(LCREC_EINVAL, "%s: logits and token_ids must be 4-byte aligned", who);
    if (B == 0) return LCREC_OK;
    const int64_t chunks = (V + MASK_CHUNK - 1) / MASK_CHUNK;
    if (chunks > 0x7fffffffLL) return fail(LCREC_EINVAL, "%s: V=%lld is more than one launch holds", who, (long long)V);
    const unsigned rows = (unsigned)(B < MASK_MAX_ROWS ? B : MASK_MAX_ROWS);
    TraceScope trace(K_TRIE_MASK, stream);
    hipLaunchKernelGGL(trie_mask_kernel, dim3((unsigned)chunks, rows), dim3(MASK_THREADS), 0, stream, *trie, node, B, depth, token_ids, eos,
                       logits, ld, V);
    return check_launch("trie_mask_kernel");
}

}  // namespace lcrec

using namespace lcrec;

LCREC_API size_t lcrec_index_trie_build_workspace(int64_t n, int L) { return index_trie_build_workspace(n, L); }

LCREC_API int lcrec_index_trie_build(const int64_t *idx, int64_t idx_stride, int64_t n, int L, const int *K, lcrec_index_trie *trie,
                                     void *workspace, size_t workspace_bytes, void *stream)
{
    return index_trie_build(idx, idx_stride, n, L, K, trie, workspace, workspace_bytes, (hipStream_t)stream);
}

LCREC_API int lcrec_index_trie_find(const lcrec_index_trie *trie, const int64_t *prefix, int64_t prefix_stride, int64_t B, int depth,
                                    int64_t *node_out, int *depth_out, void *stream)
{
    return index_trie_find(trie, prefix, prefix_stride, B, depth, node_out, depth_out, (hipStream_t)stream);
}

LCREC_API int lcrec_index_trie_mask_logits(const lcrec_index_trie *trie, const int64_t *node, int64_t B, int depth, const int *token_ids,
                                           int eos, float *logits, int64_t ld, int64_t V, void *stream)
{
    return index_trie_mask_logits(trie, node, B, depth, token_ids, eos, logits, ld, V, (hipStream_t)stream);
}
