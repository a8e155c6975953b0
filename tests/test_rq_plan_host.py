"""CPU: every row of tests/rq_cases.py gets the form and reaches the paths it claims -- asked of the library's own plan
(lcrec_debug_rq_assign_plan: the function rq_assign launches by, nothing launched) --, production's plan is what the dispatch rule
says at the shapes the rule turns on, every forced form that cannot take a shape is refused, every row's inputs exercise what the row
is for under the oracle alone, and the judge passes the oracle's own output and refuses it with one element wrong."""
import threading

import numpy as np
import pytest

import rq_cases as rq


@pytest.fixture(scope="module")
def ops():
    import lcrec_amd
    lcrec_amd._lib.load()
    return lcrec_amd.ops


def _in_thread(fn):
    """fn() in a thread of its own: the library's last-error text is per thread and is never cleared, and
    tests/test_host_logic.py::test_library_exports_every_declared_symbol asserts that the main thread's is still empty (as
    tests/test_sinkhorn_plan_host.py does for its refused calls)."""
    box = {}

    def run():
        try:
            box["value"] = fn()
        except Exception as exc:                    # noqa: BLE001 -- handed to the caller
            box["error"] = exc
    t = threading.Thread(target=run)
    t.start()
    t.join()
    if "error" in box:
        raise box["error"]
    return box["value"]


def _lds_bytes(rows, e, L, waves, split):
    """The kernel's LDS layout, restated: [rows][e + 4] codes, [roundup4(rows)] norms, [waves][L] doubles, and the split form's
    [2][waves][64] x 3 floats."""
    return (rows * (e + 4) + ((rows + 3) & ~3)) * 4 + waves * L * 8 + (2 * waves * 64 * 3 * 4 if split else 0)


@pytest.mark.parametrize("case", rq.CASES, ids=rq.case_id)
def test_row_reaches_what_it_claims(ops, case):
    p = rq.plan(case)
    bad = rq.check_claims(case, p)
    assert not bad, f"{rq.case_id(case)}:\n  " + "\n  ".join(bad) + f"\n  plan: {p}"
    # the numbers the plan reports, against the shape itself
    L, waves = len(case.Ks), p["threads"] // 64
    assert p["tiles"] == -(-case.n // 64) and p["threads"] in (256, 512) and 1 <= p["grid"] <= 256
    walkers = p["grid"] if p["split"] else p["grid"] * waves
    assert (p["trips_max"], p["trips_min"]) == (-(-p["tiles"] // walkers), p["tiles"] // walkers)
    assert p["l0"][0] == 0 and p["l1"][-1] == L and p["l0"][1:] == p["l1"][:-1] and all(a < b for a, b in zip(p["l0"], p["l1"]))
    for i, (a, b) in enumerate(zip(p["l0"], p["l1"])):
        rows = sum((K + 31) & ~31 for K in case.Ks[a:b])
        assert p["rows"][i] == rows and p["lds_bytes"][i] == _lds_bytes(rows, case.e, L, waves, p["split"]) <= 160 * 1024
        assert p["row_off"][a:b] == [sum((K + 31) & ~31 for K in case.Ks[a:l]) for l in range(a, b)]
        if b < L:                                     # greedy: the next level no longer fits
            assert _lds_bytes(rows + ((case.Ks[b] + 31) & ~31), case.e, L, waves, p["split"]) > 160 * 1024
    if p["split"]:
        assert p["threads"] == 256
        for K, per, idle in zip(case.Ks, p["blocks_per_wave"], p["idle_waves"]):
            nblk = -(-K // 32)
            shares = [max(0, min(nblk, (w + 1) * per) - w * per) for w in range(4)]
            assert per == -(-nblk // 4) and sum(shares) == nblk and idle == shares.count(0)
    else:
        assert p["blocks_per_wave"] == p["idle_waves"] == [0] * L
    odd = any((b - a) % 2 for a, b in zip(p["l0"], p["l1"]))
    assert p["handover_reuse"] == int(bool(p["split"]) and odd and p["trips_max"] > 1)
    # a forced form is that form or an error
    if case.split >= 0:
        assert p["split"] == case.split
    if case.threads:
        assert p["threads"] == case.threads
    if case.grid:
        assert p["grid"] == case.grid and case.grid <= rq.plan(case, (case.split, case.threads, 0))["grid"]
    assert not (case.e == 64 and p["threads"] == 512)


def test_every_path_is_claimed_by_a_row(ops):
    claimed = {name for case in rq.CASES for name in case.covers}
    assert not (claimed - set(rq.PROPERTIES)), claimed - set(rq.PROPERTIES)
    missing = rq.REQUIRED - claimed
    assert not missing, f"no row of rq_cases.CASES claims {sorted(missing)}: the path has lost its only test"
    for case in rq.CASES:
        assert case.covers, f"{rq.case_id(case)} claims no path"
        for key in ("split", "threads", "grid", "launches"):
            assert key in case.expect, (rq.case_id(case), key)
    assert len({rq.case_id(c) for c in rq.CASES}) == len(rq.CASES)
    # all 20 instantiations of the kernel are some row's -- by the plan --, and the 12 with 256 threads in the split form too
    ran = {(bool(p["split"]), c.e, p["threads"], c.xq, c.margin) for c, p in ((c, rq.plan(c)) for c in rq.CASES)}
    assert len(rq.INSTANTIATIONS) == 20
    assert {k[1:] for k in ran if not k[0]} >= set(rq.INSTANTIATIONS)
    assert {k[1:] for k in ran if k[0]} >= {k for k in rq.INSTANTIATIONS if k[1] == 256}


def test_a_changed_row_fails_with_the_field_or_the_property_named(ops):
    case = next(c for c in rq.CASES if c.group == "B" and c.e == 32 and c.xq and c.margin)
    p = rq.plan(case)
    assert rq.check_claims(case, p) == []
    for key, wrong, shown in (("split", 0, "split: the plan gives 1, the row says 0"),
                              ("threads", 512, "threads: the plan gives 256, the row says 512"),
                              ("grid", 6, "grid: the plan gives 2, the row says 6"),
                              ("launches", 2, "launches: the plan gives 1, the row says 2"),
                              ("trips", (1, 1), "trips: the plan gives (3, 3), the row says (1, 1)"),
                              ("handover_reuse", 0, "handover_reuse: the plan gives 1, the row says 0"),
                              ("idle_waves", [0, 0, 0], "idle_waves: the plan gives [0, 0, 1], the row says [0, 0, 0]")):
        changed = case._replace(expect=dict(case.expect, **{key: wrong}))
        assert rq.check_claims(changed, p) == [shown]
    moved = case._replace(Ks=(256, 128, 160, 64))            # the shape changed under the row: the plan says what moved
    assert rq.check_claims(moved, rq.plan(moved)) == [
        "handover_reuse: the plan gives 0, the row says 1", "blocks_per_wave: the plan gives [2, 1, 2, 1], the row says [2, 1, 2]",
        "idle_waves: the plan gives [0, 0, 1, 2], the row says [0, 0, 1]", "property handover_reuse_one_launch does not hold"]
    # every claimed property, moved to a row whose plan does not have it, fails with the property named
    plans = [(c, rq.plan(c)) for c in rq.CASES]
    for name in sorted(rq.REQUIRED):
        other = next(((c, q) for c, q in plans if not rq.PROPERTIES[name](c, q)), None)
        assert other is not None, f"{name} holds of every row: it distinguishes nothing"
        c, q = other
        assert f"property {name} does not hold" in rq.check_claims(c._replace(covers=(name,)), q)


# n, e, Ks -> what production's plan (no forcing, environment knobs unset) must say
_PRODUCTION = [
    (16859, 32, [256] * 4, dict(split=1, grid=256, trips_max=2, trips_min=1, handover_reuse=0, launches=1)),
    (20000, 32, [256] * 3, dict(split=1, handover_reuse=1, launches=1)),
    (20000, 32, [1024] * 8, dict(split=1, launches=8, handover_reuse=1)),
    (32768, 32, [256] * 4, dict(split=1, grid=256, trips_max=2, trips_min=2)),
    (32769, 32, [256] * 4, dict(split=0, threads=256)),
    (131071, 32, [256] * 4, dict(split=0, threads=256, grid=256)),
    (131072, 32, [256] * 4, dict(split=0, threads=512, grid=256)),
    (131072, 64, [256] * 4, dict(split=0, threads=256)),
    (70001, 32, [256] * 4, dict(split=0, threads=256, grid=256)),
    (100, 32, [1088, 256], dict(split=0, launches=2)),           # (the hand-over buffers would push 1088 codes out of LDS)
    (64, 32, [96], dict(split=0)),                               # (max K < 128)
    (1024, 32, [256] * 4, dict(split=1, threads=256, grid=16, trips_max=1, launches=1, handover_reuse=0)),
]


@pytest.mark.parametrize("n,e,Ks,want", _PRODUCTION, ids=[f"{n}x{e}-{len(Ks)}x{Ks[0]}" for n, e, Ks, _ in _PRODUCTION])
def test_production_plan_at_the_shapes_the_rule_turns_on(ops, n, e, Ks, want):
    import os
    assert "LCREC_RQ_SPLIT" not in os.environ and "LCREC_RQ_SPLIT_TILES" not in os.environ
    p = ops.rq_assign_plan(n, e, Ks)
    assert {k: p[k] for k in want} == want, p


def test_forced_forms_refuse_and_never_fall_through(ops):
    import lcrec_amd

    def refused(*args):
        def call():
            with pytest.raises(lcrec_amd.LcrecError) as info:
                ops.rq_assign_plan(*args)
            return str(info.value)
        return _in_thread(call)
    msg = refused(1221, 64, [96, 33], 0, 512, 0)                                # 512 threads with e = 64
    assert "(-2)" in msg and "e=64 runs 256-thread workgroups" in msg
    msg = refused(327, 32, [256], 1, 512, 0)                                    # 512 threads in the split form
    assert "(-2)" in msg and "the split form runs 256-thread workgroups" in msg
    msg = refused(100, 32, [1088, 256], 1, 0, 0)                                # split: a level then exceeds the LDS budget
    assert "(-2)" in msg and "the split form cannot take level 0 (K=1088, e=32)" in msg
    assert ops.rq_assign_plan(100, 32, [1088, 256], 0, 0, 0)["launches"] == 2   # ... which fits without the hand-over buffers
    assert "(-2)" in refused(100, 32, [4416], -1, 0, 0) and "does not fit" in refused(100, 32, [4416], 0, 0, 0)
    for args, top in (((327, 32, [256], 1, 0, 7), 6), ((327, 32, [256], 0, 0, 3), 2), ((1221, 16, [96, 33], 0, 512, 4), 3),
                      ((100000, 32, [256], 1, 0, 257), 256)):                   # a grid out of range
        msg = refused(*args)
        assert "(-2)" in msg and f"forced grid {args[-1]} (1 .. {top} for this form)" in msg
        assert ops.rq_assign_plan(*args[:-1], top)["grid"] == top
    for args in ((327, 32, [256], 2, 0, 0), (327, 32, [256], -2, 0, 0), (327, 32, [256], 0, 128, 0), (327, 32, [256], 0, 0, -1),
                 (0, 32, [256], -1, 0, 0), (327, 32, [], -1, 0, 0), (327, 32, [256, 0], -1, 0, 0)):
        assert "(-1)" in refused(*args), args
    assert "(-2)" in refused(327, 24, [256], -1, 0, 0)
    # forcing the split form past production's own limits is a form, not an error: the tile loop takes the rest
    p = ops.rq_assign_plan(100000, 32, [96], 1, 0, 0)
    assert (p["split"], p["grid"], p["trips_max"], p["trips_min"]) == (1, 256, 7, 6)


@pytest.mark.parametrize("case", rq.CASES, ids=rq.case_id)
def test_row_inputs_exercise_the_row_and_the_judge_refuses_wrong_outputs(ops, case):
    """Under the oracle alone: every split-form wave that has blocks supplies a winner for some item at every level, tau flags
    some item (rows of 63 items and more), no item's term is small enough for the bound on a sum of squares to miss it; the
    judge passes the oracle's own output and refuses it with each single change a wrong kernel could make."""
    p = rq.plan(case)
    assert rq.conditions(case, p) == [], rq.case_id(case)
    n, e, L = case.n, case.e, len(case.Ks)
    z, cbs, init = rq.inputs(case)
    again = rq.inputs(case)
    assert z.shape == (n, e) and z.dtype == np.float32 and [c.shape for c in cbs] == [(K, e) for K in case.Ks]
    assert np.array_equal(z, again[0]) and all(np.array_equal(a, b) for a, b in zip(cbs, again[1]))
    assert (init is not None) == case.accumulate and (init is None or np.abs(init).min() > 0)
    good = rq.expected(case)
    assert rq.judge(case, p, good) is None
    assert rq.judge(case, p, rq.blank(case)) is not None

    def changed(name, at, value=None, ulp=False):
        out = {k: (None if v is None else v.copy()) for k, v in good.items()}
        if ulp:
            out[name][at] = np.nextafter(out[name][at], np.float32(np.inf))
        else:
            out[name][at] = value
        return rq.judge(case, p, out)
    item, level = n - 1, L - 1                                   # the last item of the (ragged) last tile, the last level
    ref = rq.reference(case)
    other = (int(ref.idx[item, level]) + 1) % max(2, case.Ks[level])
    assert "idx differs in 1 elements" in changed("idx", (item, level), other)
    assert "idx differs in 1 elements" in changed("idx", (0, 0), int(ref.idx[0, 0]) + 32)
    assert "guard rows past the end" in changed("idx", (n, 0), 0)
    assert "guard rows past the end" in changed("idx", (n + rq.GUARD - 1, L - 1), 0)
    assert f"guard column {L}" in changed("idx", (item, L), 0)
    assert f"guard column {L + 1}" in changed("idx", (0, L + 1), int(ref.idx[0, 0]))
    for entry in range(L + 1):
        assert f"resid differs in 1 elements, first at ({entry * n + item}, {e - 1}) (entry {entry})" in \
            changed("resid", (entry * n + item, e - 1), ulp=True)
    assert "resid: guard rows" in changed("resid", ((L + 1) * n, 0), 0.0)
    if case.xq:
        assert "xq differs in 1 elements" in changed("xq", (item, 0), ulp=True)
        assert "xq: guard rows" in changed("xq", (n, e - 1), 0.0)
    if case.margin:
        finite = np.argwhere(np.isfinite(ref.margin))
        if len(finite):
            assert "margin differs in 1 elements" in changed("margin", tuple(finite[-1]), ulp=True)
        else:
            assert "margin differs in 1 elements" in changed("margin", (item, level), np.float32(3e38))
        assert "margin: guard rows" in changed("margin", (n, 0), np.float32(0))
        for l in range(L):
            assert "neartie differs in 1 elements" in changed("neartie", (item,), good["neartie"][item] ^ np.int32(1 << l))
        assert "neartie: guard rows" in changed("neartie", (n + 1,), 0)
    # one item missing from a sum of squares: the smallest term of each level, the hardest to see
    terms = rq.item_sse(case)
    for l in range(L):
        assert "sse: got" in changed("sse", (l,), ref.sse[l] - terms[:, l].min()), (l, terms[:, l].min(), ref.sse[l])
    assert "sse: entries past L" in changed("sse", (L,), 0.0)
    msg = changed("idx", (item, level), other)
    tile = item // 64
    assert f"item {item}: tile {tile}, lane {item % 64}" in msg and ("split form" in msg) == bool(p["split"])


def test_tie_rows_cross_every_boundary_the_kernel_merges_over(ops):
    """The duplicated codes of the tie rows, in the kernel's coordinates: register t of half h of block b holds code
    32 b + (t & 3) + 8 (t >> 2) + 4 h; the split form deals two blocks to each wave at 256 codes."""
    def coords(code, per=2):
        b, local = divmod(code, 32)
        h = (local >> 2) & 1
        t = (local & 3) + 4 * (local >> 3)
        assert 32 * b + (t & 3) + 8 * (t >> 2) + 4 * h == code
        return b // per, b, h, t
    a, b, c = (coords(x) for x in (5, 100, 200))
    assert len({a[0], b[0], c[0]}) == 3                                      # three different waves' shares
    a, b = coords(8), coords(12)
    assert a[:2] == b[:2] and (a[2], b[2]) == (0, 1)                        # one block, its two halves
    a, b = coords(36), coords(37)
    assert a[:3] == b[:3] and a[3] + 1 == b[3]                              # one half, neighbouring registers
    cb = rq.ties_codebook()
    for first, *rest in rq.TIE_GROUPS:
        assert all(np.array_equal(cb[first], cb[j]) for j in rest)
    rows = [c for c in rq.CASES if c.codebook == "ties"]
    assert {rq.plan(c)["split"] for c in rows} == {0, 1}
    for case in rows:
        assert rq.plan(case)["blocks_per_wave"] in ([2, 2], [0, 0]) and case.tau == 0 and case.margin
