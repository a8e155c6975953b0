// The <=128-bit key of an index tuple, shared by collide.hip (lcrec_collision_groups) and finish_beam.hip (lcrec_finish_beam): two
// tuples are the same tuple exactly when their keys are equal.  include/lcrec.h, lcrec_collision_plan, states the layout: the
// clamped codes, level 0 in the highest bits, bits[l] = ceil(log2 K[l]) bits per level; bit b of the key is bit b of the low word
// for b < 64, bit b - 64 of the high word above.
#pragma once
#include "common.h"

namespace lcrec {

struct PackDesc {
    int L;
    int bits[LCREC_MAX_LEVELS];
    int K[LCREC_MAX_LEVELS];
};

// bits[l] and their sum for K[0 .. L); K[l] >= 1 is the caller's check
inline int key_bits(const int *K, int L, int *bits)
{
    int total = 0;
    for (int l = 0; l < L; ++l) {
        int b = 0;
        while ((1LL << b) < K[l]) ++b;
        bits[l] = b;
        total += b;
    }
    return total;
}

#ifdef __HIPCC__
// The key of the L codes at `codes`, each clamped into its level: v < 0 counts as 0, v >= K[l] as K[l] - 1.
__device__ __forceinline__ unsigned __int128 pack_tuple_key(const int64_t *__restrict__ codes, const PackDesc &d)
{
    unsigned __int128 key = 0;
    for (int l = 0; l < d.L; ++l) {
        int64_t v = codes[l];
        v = v < 0 ? 0 : (v >= d.K[l] ? d.K[l] - 1 : v);
        key = (key << d.bits[l]) | (unsigned __int128)(uint64_t)v;
    }
    return key;
}
#endif

}  // namespace lcrec
