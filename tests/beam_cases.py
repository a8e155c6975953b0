"""The case table of the beam-search quantiser (lcrec_rq_beam), shared by tests/test_beam_host.py (CPU: the numpy rule of
tests/beam_ref.py alone, on every row) and tests/test_gpu_beam.py (GPU: the kernel against that rule, bit for bit).

Shapes.  e in {16, 32, 64}; W in {1, 2, 4, 8}; ks in {(48, 100, 7), (256, 256, 256, 256), (1, 300), (3, 5, 2), (2,)}: a K below 64
that is no multiple of 32; K = 1, so the beam stays at one parent for a level; K < W, so the live beams grow 3 -> 8; and a product of
all K below W, so there are dead output rows.  An item owns W lanes and a wave holds 64 / W items, so n goes around that boundary:
{1, 64 / W - 1, 64 / W, 64 / W + 1}, plus a partial workgroup (257) and several workgroups (1000).  To keep the product small every
n runs at one ks per e, and every ks at n = 257; every W on each.  Inputs as audit_cases.inputs: standard-normal latents, level-l
codebooks scaled by 0.7^l (so the oracle's greedy tuples of the same inputs come with them)."""
import functools

import audit_cases as ac
from beam_ref import beam_ref

ES = (16, 32, 64)
WS = (1, 2, 4, 8)
KS = ((48, 100, 7), (256, 256, 256, 256), (1, 300), (3, 5, 2), (2,))
KS_FOR_ALL_N = {16: (48, 100, 7), 32: (256, 256, 256, 256), 64: (1, 300)}
N_FOR_ALL_KS = 257
# The item loop: the launch's grid is 256 CUs x the workgroups of the level a CU holds at once (what its K * (4 e + 20) bytes of LDS
# allow, at most 4), each workgroup taking 256 / W items per trip.  So a second trip needs n > 256 * 4 * 256 / W: rows with one more
# trip's start and a ragged tail at the cheapest shape (two small levels at e = 16: the residuals and links between the levels go
# through the loop too), at the widest and at a narrow beam.
LOOPING = ((16, (48, 7), 8, 1024 * 32 + 37), (16, (48, 7), 2, 1024 * 128 + 65))
# ADDED (at the end of shapes()): the largest level the entry admits at each e (audit_cases.LARGEST, which derives it from the LDS
# formula: one workgroup per CU, the staging loops at their largest number of trips) at the narrowest and the widest beam; and the
# 16-level quantiser audit_cases.KS_DEEP at e = 16 -- the link walk-back over 15 earlier launches, both halves of the ping-pong
# workspace used 7 times each, and at W = 8 the live count going 2, 2, 4, 8, 8, ....
WS_LARGEST = (1, 8)
WS_DEEP = (2, 8)


def ns_for(W):
    return (1, 64 // W - 1, 64 // W, 64 // W + 1, 257, 1000)


def shapes():
    """(e, ks, W, n) rows, without repeats"""
    rows = []
    for e in ES:
        for W in WS:
            for n in ns_for(W):
                rows.append((e, KS_FOR_ALL_N[e], W, n))
            for ks in KS:
                if (e, ks, W, N_FOR_ALL_KS) not in rows:
                    rows.append((e, ks, W, N_FOR_ALL_KS))
    return rows + added_shapes()


def added_shapes():
    rows = [(e, (ac.LARGEST[e],), W, N_FOR_ALL_KS) for e in ES for W in WS_LARGEST]
    return rows + [(ac.DEEP_E, ac.KS_DEEP, W, N_FOR_ALL_KS) for W in WS_DEEP]


def shape_id(row):
    e, ks, W, n = row
    return f"e{e}-{'_'.join(map(str, ks))}-w{W}-n{n}"


def inputs(e, ks, n):
    """(z [n, e], codebooks, the oracle's greedy tuples int64 [n, L]) -- audit_cases' inputs of the shape, read only"""
    z, cbs, greedy, _, _ = ac.inputs(e, ks, n)
    return z, cbs, greedy


@functools.lru_cache(maxsize=None)
def reference(e, ks, W, n):
    """beam_ref of the shape: computed once, shared, read only"""
    z, cbs, _ = inputs(e, ks, n)
    ref = beam_ref(z, cbs, W)
    for a in ref.values():
        a.setflags(write=False)
    return ref


def deep(ks):
    """at least two levels with more than one code: the shapes on which a beam can beat the greedy walk"""
    return sum(1 for k in ks if k > 1) >= 2


def tie_case():
    """Exact ties at two levels: audit_cases.tie_case's small-integer codebook (rows 40 and 41 copies of row 7; every product and sum
    exact in fp32) at both levels, its latents (the first four exactly row 7).  -> (z, codebooks); run at W = 4"""
    z, cbs, _ = ac.tie_case()
    return z, [cbs[0], cbs[0]]


# An item that IS row 7 is at distance 0 from codes 7, 40 and 41 of level 0 and leaves a zero residual behind each; at level 1 every
# one of those three parents then scores cc_k, least at code 0, next at codes 7 = 40 = 41.  Ties go by parent, then by code: the three
# parents in order with code 0, then parent 0 with code 7 (before its codes 40 and 41, and before parents 1 and 2 with code 7).
TIE_BEAMS_OF_ROW_7 = [[7, 0], [40, 0], [41, 0], [7, 7]]


def nan_case():
    """audit_cases.nan_case's inputs: e = 32, ks = (48, 100), row 9 of the level-0 codebook holds a NaN (its distance is +inf for
    everyone), latent row 3 is all NaN, latent row 5 holds an inf.  -> (z, codebooks)"""
    z, cbs, _ = ac.nan_case()
    return z, cbs
