"""The case table of the index audit (lcrec_rq_audit), shared by tests/test_audit_host.py (CPU: the numpy rule of tests/audit_ref.py
alone, on every row) and tests/test_gpu_audit.py (GPU: the kernel against that rule, bit for bit).

Shapes.  e in {16, 32, 64}; ks in {[48, 100, 7], [256, 256, 256, 256], [1, 300], [576] (e = 64 only: the largest level the entry
admits there, the LDS edge)}; n in {1, 63, 64, 65, 257, 1000}: a lone lane, the wave boundary from both sides, a partial workgroup
and several workgroups (none of these makes a second trip of the item loop: LOOPING below does); K below 64, K no multiple of 32 or
64, K = 1 and the largest admitted level.  To keep the product small every n runs at one ks per e, and every ks at n = 257.
Inputs: standard-normal latents, level-l codebooks scaled by 0.7^l.  Each shape is audited twice: with the oracle's greedy tuples
(all ranks 0) and with uniformly random tuples (ranks up to K - 1).

ADDED (at the end of shapes(), so that every earlier row keeps its place): the largest level the entry admits at each e, LARGEST --
one workgroup resident per CU, the staging loops at their largest number of trips -- and a quantiser of LCREC_MAX_LEVELS = 16
levels, KS_DEEP: flag bit 15, sixteen launches, the residual through the workspace fifteen times."""
import functools

import numpy as np

import golden_inputs as gi
from audit_ref import audit_ref
from oracle import cpu_oracle

ES = (16, 32, 64)
NS = (1, 63, 64, 65, 257, 1000)
KS = ((48, 100, 7), (256, 256, 256, 256), (1, 300))
KS_EDGE = (576,)                                            # e = 64 only
KS_FOR_ALL_N = {16: (48, 100, 7), 32: (256, 256, 256, 256), 64: (1, 300)}
N_FOR_ALL_KS = 257
# The item loop: the launch's grid is 256 CUs x the workgroups of the level a CU holds at once (what its K * (4 e + 20) bytes of LDS
# allow, at most 8), each workgroup taking 256 items per trip.  So a second trip needs n > 256 * 256 * per_cu: rows with one more
# full trip's start and a ragged tail -- two small levels at e = 16 (per_cu = 8 on both, and the residual between the levels goes
# through the loop too), and the largest level at e = 64 (per_cu = 1).  Random tuples only: the reference costs a second or two.
LOOPING = ((16, (48, 7), 256 * 256 * 8 + 65), (64, (576,), 256 * 256 + 65))
N_RANK_SPREAD = 321                                         # random tuples reach rank >= K / 2 at every level with K >= 48
# The largest level lcrec_rq_audit (and lcrec_rq_beam, and lcrec_rq_assign) admits at L = 1: rq_level_fits of include/lcrec.h,
#   rows * (4 e + 20) + 32 L <= 160 KB = 163840 with rows = K rounded up to 32
# so rows <= (163840 - 32) / (4 e + 20) = 1950.09, 1106.8 and 593.5 at e = 16, 32 and 64, rounded down to a multiple of 32.  The
# kernel's own dynamic LDS, K * (4 e + 20), is then 161280, 161024 and 158976 bytes.  largest_level() is that derivation.
LDS_PER_CU = 160 * 1024
LARGEST = {16: 1920, 32: 1088, 64: 576}
MAX_LEVELS = 16
KS_DEEP = (2, 1, 2) + (3,) * 13                             # e = 16 only; with a beam of 8 the live count goes 2, 2, 4, 8, 8, ...
DEEP_E = 16


def level_fits(K, e, L=1):
    rows = (K + 31) & ~31
    return K >= 1 and rows * (4 * e + 20) + 32 * L <= LDS_PER_CU


def largest_level(e, L=1):
    """the largest K with level_fits(K, e, L), found by walking up"""
    K = 1
    while level_fits(K + 1, e, L):
        K += 1
    return K


def largest_admitted(admits, refused=4096):
    """The largest K with admits(K), by bisection between 1 (admitted) and `refused`.  admits(K) asks an ENTRY: a call at n = 0, which
    passes the admission check and launches nothing, is True; a refusal with the "does not fit" text is False."""
    lo, hi = 1, refused
    assert admits(lo) and not admits(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if admits(mid) else (lo, mid)
    return lo


def shapes():
    """(e, ks, n) rows, without repeats"""
    rows = []
    for e in ES:
        for n in NS:
            rows.append((e, KS_FOR_ALL_N[e], n))
        for ks in KS + ((KS_EDGE,) if e == 64 else ()):
            if (e, ks, N_FOR_ALL_KS) not in rows:
                rows.append((e, ks, N_FOR_ALL_KS))
    return rows + added_shapes()


def added_shapes():
    """the largest level at e = 16 and 32 (e = 64: KS_EDGE above) and the 16-level quantiser, at n = 257"""
    return [(e, (LARGEST[e],), N_FOR_ALL_KS) for e in ES if (LARGEST[e],) != KS_EDGE] + [(DEEP_E, KS_DEEP, N_FOR_ALL_KS)]


def shape_id(row):
    e, ks, n = row
    return f"e{e}-{'_'.join(map(str, ks))}-n{n}"


@functools.lru_cache(maxsize=None)
def inputs(e, ks, n):
    """(z [n, e], codebooks, greedy tuples int64 [n, L], the oracle's residuals [L + 1, n, e], random tuples int64 [n, L])"""
    r = gi.rs(5000 + 7 * e + 13 * n + sum(ks) + len(ks))
    z = gi.f32(r.standard_normal((n, e)))
    cbs = [gi.f32(r.standard_normal((k, e)) * (0.7 ** l)) for l, k in enumerate(ks)]
    rq = cpu_oracle.rq_assign(z, cbs, want_resid=True)
    rand = np.stack([r.randint(0, k, size=n) for k in ks], axis=1).astype(np.int64)
    for a in [z, rq["idx"], rq["resid"], rand] + cbs:
        a.setflags(write=False)
    return z, cbs, rq["idx"].astype(np.int64), rq["resid"], rand


@functools.lru_cache(maxsize=None)
def reference(e, ks, n, which):
    """audit_ref of the shape's greedy (`which` = "greedy") or random ("random") tuples: computed once, shared, read only"""
    z, cbs, greedy, _, rand = inputs(e, ks, n)
    ref = audit_ref(z, cbs, greedy if which == "greedy" else rand)
    for a in ref.values():
        a.setflags(write=False)
    return ref


def tie_case():
    """Exact ties: small-integer codebook and latents in [-2, 2] (every product and sum exact in fp32), e = 32, K = 48, rows 40 and
    41 copies of row 7, latents drawn from codebook rows, the first four exactly row 7.  Every item holds code 41."""
    e, K, n = 32, 48, 96
    r = gi.rs(5100)
    cb = gi.f32(r.randint(-2, 3, size=(K, e)))
    cb[40] = cb[7]
    cb[41] = cb[7]
    z = gi.f32(cb[r.randint(0, K, size=n)])
    z[:4] = cb[7]
    return z, [cb], np.full((n, 1), 41, dtype=np.int64)


def out_of_range_case(L):
    """Codes -1, K, 2^40 and a valid one, cycling over the items, at level 0 of L = 1, at level 1 of L = 3 or at level 15 of L = 16
    (KS_DEEP; the other levels hold the greedy code).  -> (z, codebooks, tuples, level, K of that level)
    (The valid one is code 5 where the level has more than 5 codes, else its last code.)"""
    e, n = 16, 70
    ks = {1: (48,), 3: (48, 100, 7), MAX_LEVELS: KS_DEEP}[L]
    level = {1: 0, 3: 1, MAX_LEVELS: MAX_LEVELS - 1}[L]
    z, cbs, greedy, _, _ = inputs(e, ks, n)
    idx = greedy.copy()
    idx[:, level] = np.resize(np.array([-1, ks[level], 1 << 40, min(5, ks[level] - 1)], dtype=np.int64), n)
    return z, cbs, idx, level, ks[level]


def nan_case():
    """e = 32, ks = (48, 100): row 9 of the level-0 codebook holds a NaN (its distance is +inf for everyone), latent row 3 is all
    NaN, latent row 5 holds an inf.  Random tuples; items 0 .. 2 hold code 9 at level 0."""
    e, ks, n = 32, (48, 100), 130
    z, cbs, _, _, rand = inputs(e, ks, n)
    z, cbs, idx = z.copy(), [c.copy() for c in cbs], rand.copy()
    cbs[0][9, 4] = np.nan
    z[3] = np.nan
    z[5, 1] = np.inf
    idx[:3, 0] = 9
    return z, cbs, idx


def collide_case():
    """The finishing link: ks = [4, 48] and 3 * 48 items, so every bucket of pass 1 holds more items than distinct nearest codes.
    -> (z, codebooks, the oracle's greedy tuples, its residuals)"""
    return inputs(16, (4, 48), 144)[:4]
