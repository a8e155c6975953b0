"""The case table of the decode pass (lcrec_decode_tuples), shared by tests/test_decode_host.py (CPU: the numpy rule of
tests/decode_ref.py alone, on every row) and tests/test_gpu_decode.py (GPU: the kernels against that rule, bit for bit).

Quantiser shapes, as tests/audit_cases.py (whose inputs are reused: standard-normal latents, level-l codebooks scaled by 0.7^l, the
oracle's greedy tuples and uniformly random ones): e in {16, 32, 64}; ks in {(48, 100, 7), (256, 256, 256, 256), (1, 300)}; n in
{1, 63, 64, 65, 257, 1000}; every n at one ks per e, every ks at n = 257.  For the gather kernel (e / 4 lanes per item, 256 threads:
64, 32 or 16 items per workgroup) these are a lone item, a workgroup's item count from both sides and several workgroups.

Decoders: [e, 40, w] without and with folded BatchNorm, and the single layer [e, w]; the three forms take turns over the quantiser
shapes at w = 100.  Widths: at n = 257 (three workgroups of the error kernel, the last with one row) every form runs at
  w in {4, 32, 36, 100, 128, 772}   below, at and just past the error kernel's column tile (32 columns), ragged (3 tiles + 4), a
                                    whole number of tiles, and 24 tiles + 4
  w in {6, 33, 70}                  ADDED: a width that is no multiple of 4 makes rows start off 16 bytes, and the error kernel then
                                    stages its tiles float by float instead of in 16-byte pieces (the GEMM's epilogue stores by
                                    single floats too): below a tile, just past one, and two tiles + 6.
x (the embeddings the error is taken against) is standard normal.
ADDED, as the table's last row: audit_cases.KS_DEEP, the 16-level quantiser (LCREC_MAX_LEVELS) at e = 16 and n = 257 under the
single-layer decoder at w = 100; out_of_range_case(16) puts its bad codes at level 15 (flag bit 15).  audit_cases' largest levels
are left out like KS_EDGE.

LOOPING: one row per new kernel at the smallest n that makes its item loop take a second trip, plus 65, with e = 16 and the decoder
[16, 8] (random tuples only, and codebooks drawn here without the oracle, so the reference costs a second or two).  The grid rules:
  rq_decode_gather   at most 1024 workgroups, each taking 256 / (e / 4) items per trip: a second trip needs n > 1024 * 64 at e = 16
  recon_row_error    at most 1024 workgroups (4 on each of 256 CUs: 33 KB of LDS each), each taking 128 rows per trip: n > 1024 * 128
(the second row makes the gather loop twice as well)."""
import functools

import numpy as np

import audit_cases as ac
import golden_inputs as gi
from decode_ref import decode_ref

WIDTHS = (4, 32, 36, 100, 128, 772)
WIDTHS_UNALIGNED = (6, 33, 70)
W_REST = 100
HIDDEN = 40
FORMS = ("hidden", "hidden_bn", "single")                   # [e, 40, w], the same with folded BatchNorm, [e, w]
N_FOR_ALL_W = 257
SHAPE_FOR_ALL_W = (32, (48, 100, 7))
LOOPING = (("rq_decode_gather", 16, (48, 7), 1024 * 64 + 65), ("recon_row_error", 16, (48, 7), 1024 * 128 + 65))
LOOPING_W = 8
CHUNKINGS = lambda n: (0, 1, 64, 100, n - 1, n, n + 1)      # noqa: E731  (every positive one; 0 = the built-in chunk)


def rows():
    """(e, ks, n, form, w) rows, without repeats"""
    out = []
    for i, (e, ks, n) in enumerate(ac.shapes()):
        if ks == ac.KS_EDGE or (e, ks, n) in ac.added_shapes():   # (the audit's LDS edges: the decode pass stages nothing in LDS)
            continue
        out.append((e, ks, n, FORMS[i % len(FORMS)], W_REST))
    e, ks = SHAPE_FOR_ALL_W
    for w in WIDTHS + WIDTHS_UNALIGNED:
        for form in FORMS:
            if (e, ks, N_FOR_ALL_W, form, w) not in out:
                out.append((e, ks, N_FOR_ALL_W, form, w))
    # ADDED: the 16-level quantiser (LCREC_MAX_LEVELS: the gather's sixteen codebook pointers and sixteen adds per element) under
    # the single-layer decoder
    out.append((ac.DEEP_E, ac.KS_DEEP, ac.N_FOR_ALL_KS, "single", W_REST))
    return out


def row_id(row):
    e, ks, n, form, w = row
    return f"e{e}-{'_'.join(map(str, ks))}-n{n}-{form}-w{w}"


@functools.lru_cache(maxsize=None)
def decoder(e, form, w):
    """(dims, weights, biases, bn_scales | None, bn_shifts | None) of a decoder: Xavier-scaled weights, small biases, random
    eval-mode BatchNorm statistics folded to scale / shift (golden_inputs.encoder_weights / fold_bn)"""
    dims = [e, w] if form == "single" else [e, HIDDEN, w]
    Ws, bs, bns = gi.encoder_weights(dims, seed=6100 + w, bn=form == "hidden_bn")
    scs = shs = None
    if form == "hidden_bn":
        folded = [gi.fold_bn(b) for b in bns]
        scs, shs = [f[0] for f in folded], [f[1] for f in folded]
    for a in Ws + bs + [v for v in (scs or []) + (shs or []) if v is not None]:
        a.setflags(write=False)
    return dims, Ws, bs, scs, shs


@functools.lru_cache(maxsize=None)
def embeddings(n, w, seed=6200):
    x = gi.f32(gi.rs(seed + 3 * n + w).standard_normal((n, w)))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(e, ks, n, form, w, which):
    """decode_ref of the row's greedy (`which` = "greedy") or random ("random") tuples: computed once, shared, read only"""
    _, cbs, greedy, _, rand = ac.inputs(e, ks, n)
    _, Ws, bs, scs, shs = decoder(e, form, w)
    ref = decode_ref(greedy if which == "greedy" else rand, cbs, Ws, bs, scs, shs, embeddings(n, w))
    for a in ref.values():
        a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def greedy_path(e, ks, n):
    """the oracle's own quantiser outputs for the shape's latents: dict of idx, xq (the straight-through sum) and resid [L + 1, n, e]"""
    from oracle import cpu_oracle
    z, cbs, _, _, _ = ac.inputs(e, ks, n)
    return cpu_oracle.rq_assign(z, cbs, want_resid=True)


def out_of_range_case(L):
    """audit_cases.out_of_range_case: codes -1, K, 2^40 and a valid one, cycling over the 70 items, at level 0 of L = 1, at level 1
    of L = 3 or at level 15 of L = 16; decoder [16, 40, 100].  -> (codebooks, tuples, level, K of that level, decoder, x)"""
    _, cbs, idx, level, K = ac.out_of_range_case(L)
    return cbs, idx, level, K, decoder(16, "hidden", W_REST), embeddings(len(idx), W_REST)


def nan_case():
    """e = 32, ks = (48, 100), n = 130, the single-layer decoder [32, 100] (behind a hidden layer the ReLU, t > 0 ? t : 0, would turn
    the NaN into 0): row 9 of the level-0 codebook holds a NaN and items 0 .. 2 hold code 9 there (their q holds a NaN, so their whole
    output row is NaN); row 3 of x is all NaN, row 5 of x holds an inf.
    -> (codebooks, tuples, decoder, x)"""
    e, ks, n = 32, (48, 100), 130
    _, cbs, _, _, rand = ac.inputs(e, ks, n)
    cbs, idx, x = [c.copy() for c in cbs], rand.copy(), embeddings(n, W_REST).copy()
    cbs[0][9, 4] = np.nan
    idx[:3, 0] = 9
    idx[3:, 0] = np.where(idx[3:, 0] == 9, 10, idx[3:, 0])
    x[3] = np.nan
    x[5, 1] = np.inf
    return cbs, idx, decoder(e, "single", W_REST), x


@functools.lru_cache(maxsize=None)
def looping_inputs(e, ks, n):
    """(codebooks, random tuples int64 [n, L], decoder [e, LOOPING_W], x [n, LOOPING_W]) without the oracle"""
    r = gi.rs(6300 + n)
    cbs = [gi.f32(r.standard_normal((k, e)) * (0.7 ** l)) for l, k in enumerate(ks)]
    idx = np.stack([r.randint(0, k, size=n) for k in ks], axis=1).astype(np.int64)
    return cbs, idx, decoder(e, "single", LOOPING_W), embeddings(n, LOOPING_W)
