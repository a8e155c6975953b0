"""The case table of the residual quantiser kernel (rq_assign_kernel of csrc/rq_assign.hip: 20 instantiations E x THREADS x WANT_XQ x
WANT_MARGIN, and on top of them the run-time forms -- split or one tile per wave, one launch or several, one trip of the tile loop or
several, the sums of squares finished by ticket or by rq_sse_finalize_kernel, xq_accumulate, idx_stride > L, near-tie bits carried
from launch to launch), shared by tests/test_rq_plan_host.py (CPU: every row reaches the form and the paths it claims, its inputs
exercise them under the oracle alone, and the judge refuses wrong outputs) and tests/test_gpu_rq_forms.py (GPU: every row once
through lcrec_debug_rq_assign into guarded buffers, bit for bit against the oracle).

A row is (n, e, Ks) with the three forcing arguments of lcrec_debug_rq_assign_plan (include/lcrec.h: split -1 / 0 / 1, threads 0 /
256 / 512, grid 0 / g) and the outputs it asks for, with the plan it must get (`expect`) and the kernel paths it exists for
(`covers`, names of PROPERTIES).  Each property is a predicate over the row and its plan, so a row cannot claim a path its shape
does not reach, and REQUIRED lists the paths some row must keep claiming.  Shapes are the smallest that reach their path; the plan,
not this file, decides what a shape reaches.

Values: oracle.rq_assign (the C restatement of the arithmetic contract) -- idx, xq, every residual, margin and near-tie word must
be np.array_equal to it; the per-level sums of squares, whose order of addition is the kernel's own, to rtol 1e-6 (the project's
bound for this quantity; tests/test_rq_plan_host.py shows that at these row counts one missing item moves a sum by more than 100
times that).  Every output buffer has GUARD rows past n, idx has idx_stride = L + 2, all pre-filled with NaN (-1 for integers):
lanes with item >= n compute, and must not write."""
import functools
from collections import namedtuple

import numpy as np

GUARD = 64                           # rows past n in every output
PAD_COLS = 2                         # idx_stride = L + PAD_COLS
SSE_RTOL = 1e-6                      # tests/test_gpu_kernels.py::test_rq_assign_bit_exact's bound for the sums of squares
TAU = 0.05                           # the near-tie threshold of the Gaussian rows: flags some item on every one of them
TRACE_LABEL, TRACE_FINALIZE = "rq_assign", "rq_sse_finalize"
WAVES_SPLIT = 4                      # the split form's workgroup: 256 threads

Case = namedtuple("Case", "group n e Ks split threads grid xq margin ticket accumulate codebook tau seed expect covers")


def _case(group, n, e, Ks, force, covers, xq=True, margin=True, ticket=True, accumulate=False, codebook="gauss", tau=TAU, seed=0,
          **expect):
    split, threads, grid = force
    return Case(group, n, e, tuple(Ks), split, threads, grid, bool(xq), bool(margin), bool(ticket), bool(accumulate), codebook,
                tau, seed, expect, tuple(covers))


def case_id(c):
    form = {-1: "auto", 0: "wave", 1: "split"}[c.split]
    return (f"{c.group}-{c.n}x{c.e}-{'_'.join(map(str, c.Ks))}-{form}-t{c.threads}-g{c.grid}-xq{int(c.xq)}-m{int(c.margin)}"
            + ("" if c.ticket else "-noticket") + ("-acc" if c.accumulate else ""))


def force_of(c):
    return (c.split, c.threads, c.grid)


# ---- the path properties: name -> predicate(case, plan)
INSTANTIATIONS = [(e, t, xq, m) for e in (16, 32, 64) for t in (256, 512) for xq in (False, True) for m in (False, True)
                  if not (e == 64 and t == 512)]


def _runs(p):
    return [b - a for a, b in zip(p["l0"], p["l1"])]


def _nblk(K):
    return (K + 31) // 32


PROPERTIES = {}
for _e, _t, _xq, _m in INSTANTIATIONS:
    # rq_assign_kernel<E, THREADS, WANT_XQ, WANT_MARGIN> in the one-tile-per-wave form ...
    PROPERTIES[f"wave_{_e}_{_t}_xq{int(_xq)}_m{int(_m)}"] = (lambda c, p, _k=(_e, _t, _xq, _m):
                                                            not p["split"] and (c.e, p["threads"], c.xq, c.margin) == _k)
    if _t == 256:                                                                          # ... and in the split form
        PROPERTIES[f"split_{_e}_xq{int(_xq)}_m{int(_m)}"] = (lambda c, p, _k=(_e, _xq, _m):
                                                            p["split"] == 1 and (c.e, c.xq, c.margin) == _k)
PROPERTIES.update({
    # the tile loop
    "wave_unequal_trips": lambda c, p: not p["split"] and p["trips_max"] > p["trips_min"] >= 1,
    "wave_idle_waves": lambda c, p: not p["split"] and p["trips_min"] == 0,                 # a wave with no tile at all
    "wave_512_unequal_trips": lambda c, p: not p["split"] and p["threads"] == 512 and p["trips_max"] > p["trips_min"] >= 1,
    "split_three_trips": lambda c, p: p["split"] == 1 and p["trips_min"] == 3,
    "split_one_trip": lambda c, p: p["split"] == 1 and p["trips_max"] == 1 and p["grid"] > 1,
    "ragged_last_tile_split": lambda c, p: p["split"] == 1 and c.n > 64 and c.n % 64 != 0,
    "ragged_last_tile_wave": lambda c, p: not p["split"] and c.n > 64 and c.n % 64 != 0,
    # the hand-over buffers of the split form: consecutive uses with the same level parity
    "handover_reuse_one_launch": lambda c, p: p["handover_reuse"] == 1 and p["launches"] == 1,
    "handover_reuse_one_level_launches": lambda c, p: p["handover_reuse"] == 1 and p["launches"] > 1 and set(_runs(p)) == {1},
    "handover_even_run_several_trips": lambda c, p: p["split"] == 1 and p["handover_reuse"] == 0 and p["trips_max"] > 1,
    # the deal of a level's code blocks over the split form's waves
    "split_shares_2_2_1_0": lambda c, p: p["split"] == 1 and any(_nblk(K) == 5 and per == 2 and idle == 1 for K, per, idle
                                                                  in zip(c.Ks, p["blocks_per_wave"], p["idle_waves"])),
    "split_one_block_three_idle": lambda c, p: p["split"] == 1 and any(_nblk(K) == 1 and idle == 3 for K, idle in zip(c.Ks, p["idle_waves"])),
    "split_several_blocks_per_wave": lambda c, p: p["split"] == 1 and max(p["blocks_per_wave"]) >= 8,
    # codebook sizes
    "last_block_one_code_split": lambda c, p: p["split"] == 1 and any(K % 32 == 1 and K > 32 for K in c.Ks),
    "last_block_one_code_wave": lambda c, p: not p["split"] and any(K % 32 == 1 and K > 32 for K in c.Ks),
    "one_code_split": lambda c, p: p["split"] == 1 and 1 in c.Ks and c.margin,              # margin +inf
    "one_code_wave": lambda c, p: not p["split"] and 1 in c.Ks and c.margin,
    # levels over launches
    "split_one_level_per_launch": lambda c, p: p["split"] == 1 and len(c.Ks) >= 3 and set(_runs(p)) == {1},
    "wave_one_level_per_launch": lambda c, p: not p["split"] and p["threads"] == 256 and len(c.Ks) >= 3 and set(_runs(p)) == {1},
    "wave_512_one_level_per_launch": lambda c, p: not p["split"] and p["threads"] == 512 and len(c.Ks) >= 3 and set(_runs(p)) == {1},
    "split_launches_2_then_1": lambda c, p: p["split"] == 1 and _runs(p) == [2, 1],
    "wave_launches_2_then_1": lambda c, p: not p["split"] and _runs(p) == [2, 1],
    "split_e64_two_launches": lambda c, p: p["split"] == 1 and c.e == 64 and p["launches"] == 2,
    "wave_e64_two_launches": lambda c, p: not p["split"] and c.e == 64 and p["launches"] == 2,
    "neartie_carried_split": lambda c, p: p["split"] == 1 and p["launches"] > 1 and c.margin and c.tau > 0,
    "neartie_carried_wave": lambda c, p: not p["split"] and p["launches"] > 1 and c.margin and c.tau > 0,
    # exact ties: the lowest index wins across every boundary the kernel merges over
    "exact_ties_split": lambda c, p: p["split"] == 1 and c.codebook == "ties" and c.tau == 0 and c.margin,
    "exact_ties_wave": lambda c, p: not p["split"] and c.codebook == "ties" and c.tau == 0 and c.margin,
    # xq_accumulate from a non-zero x_q
    "accumulate_split_one_launch": lambda c, p: c.accumulate and p["split"] == 1 and p["launches"] == 1,
    "accumulate_split_several_launches": lambda c, p: c.accumulate and p["split"] == 1 and p["launches"] > 1,
    "accumulate_wave_one_launch": lambda c, p: c.accumulate and not p["split"] and p["launches"] == 1,
    "accumulate_wave_several_launches": lambda c, p: c.accumulate and not p["split"] and p["launches"] > 1,
    # the sums of squares without a ticket: rq_sse_finalize_kernel
    "no_ticket_split_one_launch": lambda c, p: not c.ticket and p["split"] == 1 and p["launches"] == 1,
    "no_ticket_split_several_launches": lambda c, p: not c.ticket and p["split"] == 1 and p["launches"] > 1,
    "no_ticket_wave_one_launch": lambda c, p: not c.ticket and not p["split"] and p["launches"] == 1,
    "no_ticket_wave_several_launches": lambda c, p: not c.ticket and not p["split"] and p["launches"] > 1,
    "no_ticket_production_grid": lambda c, p: not c.ticket and c.grid == 0,
    "no_ticket_several_trips": lambda c, p: not c.ticket and p["split"] == 1 and p["trips_max"] > 1,
})
for _n in (1, 63, 64, 65):
    # tile edges, in production's own choice and in both forced forms
    PROPERTIES[f"edge_{_n}_production"] = lambda c, p, _n=_n: c.n == _n and force_of(c) == (-1, 0, 0)
    PROPERTIES[f"edge_{_n}_split"] = lambda c, p, _n=_n: c.n == _n and c.split == 1 and p["split"] == 1
    PROPERTIES[f"edge_{_n}_wave"] = lambda c, p, _n=_n: c.n == _n and c.split == 0 and not p["split"]
REQUIRED = frozenset(PROPERTIES)     # every path above must be claimed by at least one row of CASES


# ---- the table
def _inst(e, t, xq, m, split):
    return f"split_{e}_xq{int(xq)}_m{int(m)}" if split else f"wave_{e}_{t}_xq{int(xq)}_m{int(m)}"


CASES = []
# A: every instantiation once, one tile per wave.  20 tiles over 8 or 16 waves (trips 3 / 2, or 2 / 1), the last tile has 5 items,
# K = 33 is one full code block plus one code
for _e, _t, _xq, _m in INSTANTIATIONS:
    _extra = ["wave_unequal_trips", "ragged_last_tile_wave", "last_block_one_code_wave"] + (["wave_512_unequal_trips"] if _t == 512 else [])
    CASES.append(_case("A", 1221, _e, [96, 33], (0, _t, 2), [_inst(_e, _t, _xq, _m, False)] + _extra, xq=_xq, margin=_m,
                       split=0, threads=_t, grid=2, launches=1, trips=(3, 2) if _t == 256 else (2, 1), handover_reuse=0))
# B: every 256-thread instantiation in the split form.  Three trips; an odd run of levels in one launch; 160 codes are 5 blocks
# over 4 waves: shares 2, 2, 1, 0; ragged last tile of 7 items
for _e in (16, 32, 64):
    for _xq in (False, True):
        for _m in (False, True):
            CASES.append(_case("B", 327, _e, [256, 128, 160], (1, 0, 2),
                               [_inst(_e, 256, _xq, _m, True), "split_three_trips", "handover_reuse_one_launch", "split_shares_2_2_1_0",
                                "ragged_last_tile_split"], xq=_xq, margin=_m,
                               split=1, threads=256, grid=2, launches=1, trips=(3, 3), handover_reuse=1, blocks_per_wave=[2, 1, 2],
                               idle_waves=[0, 0, 1]))
# C1: one level per launch, all outputs, near-tie bits carried across launches
CASES += [
    _case("C1", 327, 32, [1024, 1024, 1000], (1, 0, 2), ["split_one_level_per_launch", "handover_reuse_one_level_launches",
                                                        "neartie_carried_split", "split_several_blocks_per_wave"],
          split=1, threads=256, grid=2, launches=3, runs=[1, 1, 1], trips=(3, 3), handover_reuse=1),
    _case("C1", 327, 32, [1024, 1024, 1000], (0, 256, 1), ["wave_one_level_per_launch", "neartie_carried_wave"],
          split=0, threads=256, grid=1, launches=3, runs=[1, 1, 1], trips=(2, 1), handover_reuse=0),
    _case("C1", 327, 32, [1024, 1024, 1000], (0, 512, 1), ["wave_512_one_level_per_launch", "wave_idle_waves"],
          split=0, threads=512, grid=1, launches=3, runs=[1, 1, 1], trips=(1, 0), handover_reuse=0),
    # C2: launches of 2 levels then 1.  At 84 bytes per row 1824 rows take 159 456 B with the split buffers, which fits; 1952 rows
    # take 163 968 B and more, which does not
    _case("C2", 327, 16, [1024, 800, 100], (1, 0, 2), ["split_launches_2_then_1"],
          split=1, threads=256, grid=2, launches=2, runs=[2, 1], rows=[1824, 128], lds_first=159456, trips=(3, 3), handover_reuse=1),
    _case("C2", 327, 16, [1024, 800, 100], (0, 0, 1), ["wave_launches_2_then_1"],
          split=0, threads=256, grid=1, launches=2, runs=[2, 1], rows=[1824, 128], trips=(2, 1), handover_reuse=0),
    # C3: e = 64 over two launches, in both forms
    _case("C3", 327, 64, [512, 512], (1, 0, 2), ["split_e64_two_launches"],
          split=1, threads=256, grid=2, launches=2, runs=[1, 1], trips=(3, 3), handover_reuse=1),
    _case("C3", 327, 64, [512, 512], (0, 0, 1), ["wave_e64_two_launches"],
          split=0, threads=256, grid=1, launches=2, runs=[1, 1], trips=(2, 1), handover_reuse=0),
]
# D: tile edges in production's choice (the split form: 128 codes) and both forced forms; K = 7 is one block: three waves idle in
# the split form
for _n in (1, 63, 64, 65):
    _grid = (_n + 63) // 64
    CASES += [
        _case("D", _n, 32, [128, 7], (-1, 0, 0), [f"edge_{_n}_production"] + (["split_one_trip"] if _n == 65 else []),
              split=1, threads=256, grid=_grid, launches=1, trips=(1, 1), handover_reuse=0),
        _case("D", _n, 32, [128, 7], (1, 0, 0), [f"edge_{_n}_split", "split_one_block_three_idle"],
              split=1, threads=256, grid=_grid, launches=1, trips=(1, 1), blocks_per_wave=[1, 1], idle_waves=[0, 3]),
        _case("D", _n, 32, [128, 7], (0, 0, 0), [f"edge_{_n}_wave"],
              split=0, threads=256, grid=1, launches=1, trips=(1, 0)),
    ]
# D: K = 1 (margin +inf), a last block with one real code
CASES += [
    _case("D", 130, 32, [1], (1, 0, 0), ["one_code_split"], split=1, threads=256, grid=3, launches=1, idle_waves=[3]),
    _case("D", 130, 32, [1], (0, 0, 0), ["one_code_wave"], split=0, threads=256, grid=1, launches=1),
    _case("D", 130, 32, [129], (1, 0, 0), ["last_block_one_code_split", "split_shares_2_2_1_0"], seed=1,
          split=1, threads=256, grid=3, launches=1, blocks_per_wave=[2], idle_waves=[1]),
    _case("D", 130, 32, [129], (0, 0, 0), ["last_block_one_code_wave"], seed=1, split=0, threads=256, grid=1, launches=1),
    _case("D", 130, 32, [256, 1], (1, 0, 0), ["one_code_split"], split=1, threads=256, grid=3, launches=1, idle_waves=[0, 3]),
    _case("D", 130, 32, [256, 1], (0, 0, 0), ["one_code_wave"], split=0, threads=256, grid=1, launches=1),
    # E: exact ties (small-integer codebook, twice), duplicates placed so that the tie crosses each boundary the kernel merges over
    _case("E", 327, 32, [256, 256], (1, 0, 2), ["exact_ties_split", "handover_even_run_several_trips"], codebook="ties", tau=0.0,
          split=1, threads=256, grid=2, launches=1, trips=(3, 3), handover_reuse=0, blocks_per_wave=[2, 2]),
    _case("E", 327, 32, [256, 256], (0, 0, 2), ["exact_ties_wave"], codebook="ties", tau=0.0,
          split=0, threads=256, grid=2, launches=1, trips=(1, 0)),
]
# F: xq_accumulate = 1 from a non-zero x_q; G: the sums of squares with ticket = NULL -- one launch and several, both forms
for _Ks, _launches, _tag in (([256, 128], 1, "one_launch"), ([1024, 1024], 2, "several_launches")):
    CASES += [
        _case("F", 327, 32, _Ks, (1, 0, 2), [f"accumulate_split_{_tag}"], accumulate=True,
              split=1, threads=256, grid=2, launches=_launches, trips=(3, 3)),
        _case("F", 327, 32, _Ks, (0, 0, 2), [f"accumulate_wave_{_tag}"], accumulate=True,
              split=0, threads=256, grid=2, launches=_launches, trips=(1, 0)),
        _case("G", 327, 32, _Ks, (1, 0, 0), [f"no_ticket_split_{_tag}", "no_ticket_production_grid"], ticket=False,
              split=1, threads=256, grid=6, launches=_launches, trips=(1, 1)),
        _case("G", 327, 32, _Ks, (1, 0, 2), [f"no_ticket_split_{_tag}", "no_ticket_several_trips"], ticket=False,
              split=1, threads=256, grid=2, launches=_launches, trips=(3, 3)),
        # (one tile per wave: production's grid for 327 items IS 2, so "production" and "2" are one launch; grid 1 is the other)
        _case("G", 327, 32, _Ks, (0, 0, 0), [f"no_ticket_wave_{_tag}", "no_ticket_production_grid"], ticket=False,
              split=0, threads=256, grid=2, launches=_launches, trips=(1, 0)),
        _case("G", 327, 32, _Ks, (0, 0, 1), [f"no_ticket_wave_{_tag}"], ticket=False,
              split=0, threads=256, grid=1, launches=_launches, trips=(2, 1)),
    ]


def plan(case, force=None):
    """lcrec_debug_rq_assign_plan for the row (or for its shape under another forcing triple): the dict of
    lcrec_amd.ops.rq_assign_plan.  Host code of the library, no GPU."""
    import lcrec_amd
    return lcrec_amd.ops.rq_assign_plan(case.n, case.e, list(case.Ks), *(force_of(case) if force is None else force))


def check_claims(case, p):
    """What of `case`'s expect / covers does NOT hold for plan `p`: a list of messages that name the field or the property
    (empty: the row tests what it says)."""
    got = {"split": p["split"], "threads": p["threads"], "grid": p["grid"], "launches": p["launches"],
           "trips": (p["trips_max"], p["trips_min"]), "handover_reuse": p["handover_reuse"], "runs": _runs(p), "rows": p["rows"],
           "lds_first": p["lds_bytes"][0], "blocks_per_wave": p["blocks_per_wave"], "idle_waves": p["idle_waves"]}
    bad = [f"{key}: the plan gives {got.get(key)}, the row says {want}" for key, want in case.expect.items() if got.get(key) != want]
    for name in case.covers:
        if not PROPERTIES[name](case, p):
            bad.append(f"property {name} does not hold")
    return bad


# ---- inputs and the reference
TIE_GROUPS = ((5, 100, 200), (8, 12), (36, 37))   # equal codes: the first of each group must win


def ties_codebook(e=32, K=256):
    """The small-integer codebook of tests/test_gpu_kernels.py::test_rq_assign_exact_ties_take_first_index -- every product and sum
    is exact in fp32 in any order, so ties are real ties -- with duplicates across: two block shares of different waves of the
    split form (5 / 100 / 200: waves 0, 1 and 3 at two blocks a wave), the two halves of one block (8 / 12: register groups h = 0
    and h = 1), two registers of one half (36 / 37)."""
    rs = np.random.RandomState(7)
    cb = rs.randint(-3, 4, size=(K, e)).astype(np.float32)
    for first, *rest in TIE_GROUPS:
        for j in rest:
            cb[j] = cb[first]
    return cb


def inputs(case):
    """(z [n, e], [codebook [K_l, e]], xq_init [n, e] | None), all fp32.  Gaussian rows: z = N(0, 1), level l = 0.8 ** l * N(0, 1)
    as in test_rq_assign_bit_exact, seeded per shape and the row's `seed` (a seed whose inputs miss a condition of conditions()
    is replaced by the next, never the condition).  Tie rows: every fourth item sits next to a duplicated code, the last tile's too."""
    rs = np.random.RandomState(1000 * case.seed + case.n + case.e + sum(case.Ks))
    if case.codebook == "ties":
        cb = ties_codebook(case.e, case.Ks[0])
        assert all(K == case.Ks[0] for K in case.Ks)
        src = rs.randint(0, case.Ks[0], size=case.n)
        dup = [j for g in TIE_GROUPS for j in g]
        src[::4] = [dup[i % len(dup)] for i in range(len(src[::4]))]
        z = cb[src] + rs.randint(-1, 2, size=(case.n, case.e)).astype(np.float32)
        cbs = [cb] * len(case.Ks)
    else:
        z = rs.standard_normal((case.n, case.e)).astype(np.float32)
        cbs = [(rs.standard_normal((K, case.e)) * (0.8 ** l)).astype(np.float32) for l, K in enumerate(case.Ks)]
    init = rs.standard_normal((case.n, case.e)).astype(np.float32) if case.accumulate else None
    return z, cbs, init


Reference = namedtuple("Reference", "idx xq sse resid margin scale")


@functools.lru_cache(maxsize=None)
def _reference(n, e, Ks, codebook, seed):
    from oracle import cpu_oracle
    z, cbs, _ = inputs(Case("", n, e, Ks, 0, 0, 0, True, True, True, False, codebook, 0.0, seed, {}, ()))
    o = cpu_oracle.rq_assign(z, cbs, want_resid=True, want_margin=True)
    ref = Reference(o["idx"], o["xq"], o["sse"], o["resid"], o["margin"], o["scale"])
    for a in ref:
        a.setflags(write=False)
    return ref


def reference(case):
    """oracle.rq_assign(..., want_resid=True, want_margin=True) for the row's inputs; computed once per distinct problem and shared
    (read-only)."""
    return _reference(case.n, case.e, case.Ks, case.codebook, case.seed)


def neartie_bits(case):
    """The flag word as the existing test computes it: bit l = margin_l <= float32(tau) * scale_l."""
    ref = reference(case)
    flags = ref.margin <= np.float32(case.tau) * ref.scale
    return (flags.astype(np.int64) << np.arange(len(case.Ks))).sum(1).astype(np.int32)


def expected_xq(case):
    """The oracle's x_q; with xq_accumulate, in numpy fp32: xq = init; xq += r_l + (c_l - r_l) level by level from the oracle's
    residuals and codes (elementwise, so exact to restate)."""
    ref = reference(case)
    if not case.accumulate:
        return ref.xq
    _, cbs, init = inputs(case)
    xq = init.copy()
    for l, cb in enumerate(cbs):
        r = ref.resid[l]
        c = cb[ref.idx[:, l]]
        xq = (xq + (r + (c - r)).astype(np.float32)).astype(np.float32)
    return xq


def blank(case):
    """The guarded output buffers of the row, pre-filled: a dict of numpy arrays (None for an output the row does not ask for)."""
    n, e, L = case.n, case.e, len(case.Ks)
    out = {"idx": np.full((n + GUARD, L + PAD_COLS), -1, np.int64),
           "xq": np.full((n + GUARD, e), np.nan, np.float32) if case.xq else None,
           "sse": np.full(L + GUARD, np.nan, np.float64),
           "resid": np.full(((L + 1) * n + GUARD, e), np.nan, np.float32),
           "margin": np.full((n + GUARD, L), np.nan, np.float32) if case.margin else None,
           "neartie": np.full(n + GUARD, -1, np.int32) if case.margin else None}
    if case.accumulate:
        out["xq"][:n] = inputs(case)[2]
    return out


def expected(case):
    """The oracle's outputs in the layout of blank(): what a correct run leaves in the buffers."""
    n, L = case.n, len(case.Ks)
    ref = reference(case)
    out = blank(case)
    out["idx"][:n, :L] = ref.idx
    if case.xq:
        out["xq"][:n] = expected_xq(case)
    out["sse"][:L] = ref.sse
    out["resid"][:(L + 1) * n] = ref.resid.reshape((L + 1) * n, case.e)
    if case.margin:
        out["margin"][:n] = ref.margin
        out["neartie"][:n] = neartie_bits(case)
    return out


def item_sse(case):
    """[n, L] float64: each item's own term of the oracle's per-level sum of squares, from its residuals and codes."""
    ref = reference(case)
    _, cbs, _ = inputs(case)
    cols = []
    for l, cb in enumerate(cbs):
        t = (cb[ref.idx[:, l]] - ref.resid[l]).astype(np.float32)
        cols.append((t.astype(np.float64) ** 2).sum(1))
    return np.stack(cols, axis=1)


def conditions(case, p):
    """What the row's inputs fail to exercise, under the oracle alone: a list of messages (empty: the row runs what it is for).
    A row with fewer items than a level has wave shares cannot give every share a winner, and one item need not be a near tie:
    the two conditions on the winners are asked of the rows with at least 63 items."""
    ref = reference(case)
    bad = []
    L = len(case.Ks)
    sse = item_sse(case)
    total = sse.sum(0)
    if not np.allclose(total, ref.sse, rtol=1e-9):
        bad.append(f"the per-item terms add up to {total}, the oracle's sums are {ref.sse}")
    for l in range(L):
        if not sse[:, l].min() > 100 * SSE_RTOL * ref.sse[l]:
            bad.append(f"level {l}: item {int(sse[:, l].argmin())}'s term {sse[:, l].min():.3e} is not above 100 x {SSE_RTOL} x the "
                       f"sum {ref.sse[l]:.6e}: the bound on the sum would not miss it")
    if case.n < 63:
        return bad
    if p["split"]:
        for l, K in enumerate(case.Ks):
            per = p["blocks_per_wave"][l]
            for w in range(WAVES_SPLIT - p["idle_waves"][l]):
                lo, hi = w * per * 32, min((w + 1) * per * 32, K)
                if not ((ref.idx[:, l] >= lo) & (ref.idx[:, l] < hi)).any():
                    bad.append(f"level {l}: no item's winner is among wave {w}'s codes {lo} .. {hi - 1}")
    if case.codebook == "ties":
        for first, *rest in TIE_GROUPS:
            at = ref.idx[:, 0] == first
            if not (at.any() and (ref.margin[at, 0] == 0).all() and ((neartie_bits(case)[at] & 1) == 1).all()):
                bad.append(f"code {first}: no item wins it at level 0 with margin 0 and bit 0 set at tau = 0")
            if np.isin(ref.idx[:, 0], rest).any():
                bad.append(f"the oracle itself takes one of {rest}, the later copies of code {first}")
        if not (at_last_tile(case, ref.idx[:, 0])):
            bad.append("no item of the ragged last tile wins a duplicated code")
    elif max(case.Ks) > 1 and not (neartie_bits(case) != 0).any():          # (one code: the margin is +inf, nothing to flag)
        bad.append(f"tau = {case.tau} flags no item")
    return bad


def at_last_tile(case, col):
    firsts = [g[0] for g in TIE_GROUPS]
    return bool(np.isin(col[case.n - case.n % 64:], firsts).any()) if case.n % 64 else True


# ---- the judge
def _first(mask):
    return tuple(int(v) for v in np.argwhere(mask)[0])


def where(case, p, item):
    """Item `item` in the kernel's own coordinates under plan `p`."""
    tile, lane = divmod(item, 64)
    if p["split"]:
        return (f"item {item}: tile {tile}, lane {lane}; workgroup {tile % p['grid']} of {p['grid']}, its trip {tile // p['grid']} "
                f"of {-(-(p['tiles'] - tile % p['grid']) // p['grid'])} (split form)")
    walkers = p["grid"] * p["threads"] // 64
    gw = tile % walkers
    return (f"item {item}: tile {tile}, lane {lane}; workgroup {gw // (p['threads'] // 64)} of {p['grid']}, wave {gw % (p['threads'] // 64)}, "
            f"its trip {tile // walkers} (one tile per wave, {p['threads']} threads)")


def _differs(a, b):
    """Elementwise: not the same bits (NaN equal to NaN: the guards)."""
    if a.dtype.kind == "f":
        return ~((a == b) | (np.isnan(a) & np.isnan(b)))
    return a != b


def judge(case, p, out):
    """The buffers a run left (layout of blank()) against the oracle: None when idx, xq, every residual, margin and near-tie word
    are the oracle's bit for bit, the sums of squares are within SSE_RTOL, and every guard row and column is untouched; else a
    message that says which, and where the first wrong item sits in plan `p`."""
    n, L = case.n, len(case.Ks)
    want = expected(case)
    msg = []
    for name in ("idx", "xq", "resid", "margin", "neartie"):
        g, w = out.get(name), want[name]
        if w is None:
            continue
        if g is None or g.shape != w.shape or g.dtype != w.dtype:
            msg.append(f"{name}: not the buffer of blank()")
            continue
        rows = (L + 1) * n if name == "resid" else n
        diff = _differs(g, w)
        body = diff[:rows, :L] if name == "idx" else diff[:rows]
        if body.any():
            at = _first(body)
            extra = f" (entry {at[0] // n})" if name == "resid" else ""
            msg.append(f"{name} differs in {int(body.sum())} elements, first at {at}{extra}: got {g[at]!r}, want {w[at]!r}; "
                       f"{where(case, p, at[0] % n)}")
        if diff[rows:].any():
            msg.append(f"{name}: guard rows past the end were written, first at row {rows + _first(diff[rows:])[0]}")
        if name == "idx" and diff[:n, L:].any():
            at = _first(diff[:n, L:])
            msg.append(f"idx: guard column {L + at[1]} (idx_stride {L + PAD_COLS}) was written at item {at[0]}")
    g, w = out["sse"], want["sse"]
    if g.shape != w.shape:
        msg.append("sse: not the buffer of blank()")
    else:
        with np.errstate(invalid="ignore"):
            err = np.abs(g[:L] - w[:L])
        if not (err <= SSE_RTOL * np.abs(w[:L])).all():
            msg.append(f"sse: got {g[:L]}, want {w[:L]} within rtol {SSE_RTOL}")
        if not np.isnan(g[L:]).all():
            msg.append("sse: entries past L were written")
    if not msg:
        return None
    return "\n  ".join([case_id(case)] + msg)
