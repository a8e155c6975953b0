"""CPU: every row of tests/sinkhorn_group_cases.py gets the launches it expects and reaches the paths it claims -- asked of the
library's own plan (lcrec_debug_sinkhorn_groups_plan: the function lcrec_sinkhorn_assign launches by, nothing launched) --, no
plan asks for more LDS than a workgroup can have, every row's inputs can be judged on every row of every group under the reference
alone, the recorded tolerance is the measured one, and the judge refuses the reference made wrong in each of the ways the table
is there to catch."""
import ctypes
import threading

import numpy as np
import pytest

import sinkhorn_group_cases as gc


@pytest.fixture(scope="module")
def ops():
    import lcrec_amd
    lcrec_amd._lib.load()
    return lcrec_amd.ops


def _in_thread(fn):
    """fn() in a thread of its own: the library's last-error text is per thread and is never cleared, and
    tests/test_host_logic.py::test_library_exports_every_declared_symbol asserts that the main thread's is still empty."""
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


@pytest.mark.parametrize("case", gc.CASES, ids=gc.case_id)
def test_row_plan_is_the_expected_one_and_reaches_what_it_claims(ops, case):
    import lcrec_amd
    p = gc.plan(case)
    bad = gc.check_claims(case, p)
    assert not bad, f"{gc.case_id(case)}:\n  " + "\n  ".join(bad) + f"\n  plan: {p}"
    offs = gc.offsets(case)
    K = case.K
    # the plan's numbers against the table itself
    classes = [gc.sk_class(g, K) if g else -1 for g in case.sizes]
    mids = [g for g, k in zip(case.sizes, classes) if k == gc.SLAB]
    assert p["slab_ok"] == (len(mids) > 0 and max(mids) * 12.0 * (K / 256.0) * ((len(mids) + 255) // 256) <= 500.0 * len(mids))
    routed = [gc.BATCH if (k == gc.SLAB and not p["slab_ok"]) else k for k in classes]
    assert [r[0] for r in p["routes"]] == routed
    at, slab = 0, 0
    for cls in range(5):
        mine = [g for g, k in enumerate(routed) if k == cls]
        c = p["cls"][cls]
        assert c["groups"] == len(mine) and c["table_first"] == at and c["threads"] == (1024 if cls == gc.SLAB else 256)
        assert c["maxg"] == max([case.sizes[g] for g in mine], default=0)
        if not mine:
            assert c["label"] is None and c["lds_bytes"] == 0 and c["set_attribute"] == 0
            continue
        m = c["maxg"]
        assert c["lds_bytes"] == (0 if cls == gc.SLAB else (m * K + ((m + 1) & ~1) + K) * 8)
        assert c["set_attribute"] == (c["lds_bytes"] > 48 * 1024) and c["lds_bytes"] + gc.LDS_STATIC <= gc.LDS_LIMIT
        assert c["label"] == ("sinkhorn_slab" if cls == gc.SLAB else "sinkhorn_tiny" if m * K <= 2048 else "sinkhorn_small")
        for g in mine:                                       # offset order inside the class; slab slices cumulative
            size = case.sizes[g]
            assert p["routes"][g] == (cls, at, slab if cls == gc.SLAB else 0), (g, p["routes"][g])
            at += 1
            if cls == gc.SLAB:
                slab += size * K + ((size + 1) & ~1) + K
    assert p["table_groups"] == at and p["slab_doubles"] == slab
    for g, k in enumerate(routed):
        if k in (-1, gc.BATCH):
            assert p["routes"][g] == (k, -1, 0)
    batch = [case.sizes[g] for g, k in enumerate(routed) if k == gc.BATCH]
    assert (p["batch_groups"], p["batch_biggest"]) == (len(batch), max(batch, default=0))
    assert p["transport"] == (0 if at == 0 else gc.ARGUMENT if at <= 4 else gc.RING if case.context else gc.SYNCHRONOUS)
    lds, mid = p["cls"][0]["groups"], sum(p["cls"][k]["groups"] for k in (1, 2, 3))
    assert p["fork_mask"] == ((1 if case.context and slab and lds + mid else 0) | (2 if case.context and lds and mid else 0))
    # the workspace is the one lcrec_sinkhorn_assign asks for, whatever the context
    oarr = offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    assert p["workspace_bytes"] == lcrec_amd._lib.load().lcrec_sinkhorn_assign_workspace(gc.rows(case), K, oarr, len(case.sizes))
    other = ops.sinkhorn_groups_plan(K, offs, has_context=not case.context, routes=True)
    assert other["workspace_bytes"] == p["workspace_bytes"] and other["routes"] == p["routes"] and other["cls"] == p["cls"]
    assert np.isfinite(np.exp(1.0 / case.eps))


def test_every_path_is_claimed_by_a_row(ops):
    claimed = {name for case in gc.CASES for name in case.covers}
    assert not (claimed - set(gc.PROPERTIES)), claimed - set(gc.PROPERTIES)
    missing = gc.REQUIRED - claimed
    assert not missing, f"no row of sinkhorn_group_cases.CASES claims {sorted(missing)}: the path has lost its only test"
    for case in gc.CASES:
        assert case.covers, f"{gc.case_id(case)} claims no path"
        for key in ("groups", "maxg", "batch", "transport", "fork", "slab_ok"):
            assert key in case.expect, (gc.case_id(case), key)
    assert len({gc.case_id(c) for c in gc.CASES}) == len(gc.CASES)
    # all six instantiations, by the plan: E x {LDS, slab}
    ran = set()
    for case in gc.CASES:
        p = gc.plan(case)
        ran |= {(case.e, False) for k in p["cls"][:4] if k["groups"]} | ({(case.e, True)} if p["cls"][gc.SLAB]["groups"] else set())
    assert ran == {(e, slab) for e in (16, 32, 64) for slab in (False, True)}
    # every fork mask and every transport; the pairs that run the same sizes with and without a context
    plans = [gc.plan(c) for c in gc.CASES]
    assert {p["fork_mask"] for c, p in zip(gc.CASES, plans) if c.context} == {0, 1, 2, 3}
    assert {p["transport"] for p in plans} == {gc.ARGUMENT, gc.RING, gc.SYNCHRONOUS}
    assert len(with_and_without_context()) >= 2
    # the back-to-back calls: more of them than the ring has slots, every table through the ring, no two alike
    rows = [gc.CASES[i] for i in gc.BACK_TO_BACK]
    assert len(rows) == 6 and len({(c.K, c.sizes) for c in rows}) == 6
    assert all(c.context and gc.plan(c)["transport"] == gc.RING for c in rows)


def with_and_without_context():
    """Pairs of rows that differ in `context` alone."""
    key = lambda c: c._replace(context=True, expect={}, covers=())
    return [(a, b) for a in gc.CASES for b in gc.CASES if a.context and not b.context and key(a) == key(b)]


def test_a_changed_row_fails_with_the_field_named(ops):
    case = gc.CASES[2]
    p = gc.plan(case)
    assert case.sizes == (65, 2, 72, 12, 71, 65) and gc.check_claims(case, p) == []
    for key, wrong, shown in (("groups", (1, 1, 0, 0, 3), "groups: the plan gives (1, 1, 0, 0, 4), the row says (1, 1, 0, 0, 3)"),
                              ("maxg", (2, 12, 0, 0, 71), "maxg: the plan gives (2, 12, 0, 0, 72), the row says (2, 12, 0, 0, 71)"),
                              ("batch", (1, 72), "batch: the plan gives (0, 0), the row says (1, 72)"),
                              ("transport", gc.ARGUMENT, "transport: the plan gives 2, the row says 1"),
                              ("fork", 1, "fork: the plan gives 3, the row says 1"),
                              ("slab_ok", 0, "slab_ok: the plan gives 1, the row says 0")):
        changed = case._replace(expect=dict(case.expect, **{key: wrong}))
        assert gc.check_claims(changed, p) == [shown]
    assert gc.check_claims(case._replace(covers=("g1_degenerate",)), p) == ["property g1_degenerate does not hold"]
    moved = case._replace(context=False)                             # the call changed under the row: the plan says what moved
    assert gc.check_claims(moved, gc.plan(moved)) == ["transport: the plan gives 3, the row says 2", "fork: the plan gives 0, the row says 3",
                                                      "property fork_both does not hold", "property table_by_ring does not hold"]


def test_no_plan_asks_for_more_lds_than_a_workgroup_has(ops):
    """K = 1 .. 4200, g = 1 .. 4100: whatever class a lone group falls into, its launch asks for at most 163 840 B of LDS, the 64 B
    static part included.  (By arithmetic a group that fills the 16 384-double class needs (g K + ((g + 1) & ~1) + K) x 8 B; at
    K = 4096, g = 4 that is 163 872 B.  Such a group belongs to the slab class: pinned here, never launched.)"""
    K = np.arange(1, 4201, dtype=np.int64)[:, None]
    g = np.arange(1, 4101, dtype=np.int64)[None, :]
    q = g * K
    need = (q + ((g + 1) & ~1) + K) * 8 + gc.LDS_STATIC
    fits = (q <= 16384) & (need <= gc.LDS_LIMIT)
    refused = np.argwhere((q <= 16384) & ~fits)
    # the rule bites at both ends of the class: four rows from K = 4094 up (csum is long), and K = 4 from 4094 rows up (rsum is)
    assert {(int(K[k, 0]), int(g[0, j])) for k, j in refused} == {(Kx, 4) for Kx in (4094, 4095, 4096)} | {(4, gx) for gx in (4094, 4095, 4096)}
    # the library's rule, asked group by group where it can differ from the class bound alone (q <= 16384: 150 k plans), and on the
    # diagonal beyond it
    lib_cls = np.full(q.shape, -2, dtype=np.int64)
    import lcrec_amd
    fn = lcrec_amd._lib.load().lcrec_debug_sinkhorn_groups_plan
    plan = lcrec_amd._lib.SinkhornGroupsPlan()
    route = (lcrec_amd._lib.SinkhornGroupRoute * 1)()
    offs = (ctypes.c_int64 * 2)(0, 0)
    worst = 0
    for ki, gi in np.argwhere(q <= 16384 + 4200):
        offs[1] = int(g[0, gi])
        assert fn(int(K[ki, 0]), offs, 1, 1, ctypes.addressof(plan), ctypes.addressof(route)) == 0
        c = plan.cls[route[0].cls] if route[0].cls <= 3 else None
        lib_cls[ki, gi] = route[0].cls
        if c is not None:
            assert c.groups == 1 and c.lds_bytes == need[ki, gi] - gc.LDS_STATIC
            worst = max(worst, int(c.lds_bytes) + gc.LDS_STATIC)
        else:
            assert not fits[ki, gi], (int(K[ki, 0]), int(g[0, gi]))
    assert worst <= gc.LDS_LIMIT and worst > gc.LDS_LIMIT - 64, worst
    asked = lib_cls > -2
    assert np.array_equal((lib_cls <= 3)[asked], fits[asked])
    # the group the issue names, and its neighbours
    for Kx, gx, cls in ((4096, 4, gc.BATCH), (4094, 4, gc.BATCH), (4093, 4, 3), (4096, 3, 3), (4096, 5, gc.BATCH)):
        p = ops.sinkhorn_groups_plan(Kx, [0, gx], routes=True)
        assert p["routes"][0][0] == cls, (Kx, gx, p)        # (alone a slab-sized group is not slab_ok: the batch path)
    p = ops.sinkhorn_groups_plan(4096, [0, 4, 8, 12, 16, 20, 24, 28, 32], routes=True)
    assert [r[0] for r in p["routes"]] == [gc.SLAB] * 8 and p["slab_ok"] == 1 and p["cls"][3]["groups"] == 0
    assert p["cls"][gc.SLAB]["lds_bytes"] == 0 and p["slab_doubles"] == 8 * (4 * 4096 + 4 + 4096)


def test_plan_refusals(ops):
    import lcrec_amd

    def refused(K, offs):
        def call():
            with pytest.raises(lcrec_amd.LcrecError) as info:
                ops.sinkhorn_groups_plan(K, offs)
            return str(info.value)
        return _in_thread(call)
    assert "bad G/K" in refused(0, [0, 2])
    assert "not ascending" in refused(16, [0, 5, 3])
    assert "outside [0, n]" in refused(16, [-1, 3])
    empty = ops.sinkhorn_groups_plan(16, [0, 0, 0], routes=True)
    assert empty["table_groups"] == 0 and empty["transport"] == 0 and empty["routes"] == [(-1, -1, 0)] * 2


@pytest.mark.parametrize("case", gc.CASES, ids=gc.case_id)
def test_row_inputs_are_judgeable_and_the_judge_refuses_wrong_solves(ops, case):
    """Under the reference alone: three fp64 evaluations of the reference's loop (one with reversed sums and jittered exp) agree on
    the winner and the runner-up of every row of every group, so the GPU test excludes no row and tolerates none; each of the three
    passes the judge; and the reference made wrong in each way the row is exposed to does not."""
    assert gc.conditions(case) == [], gc.case_id(case)
    z, cb = gc.inputs(case)
    again = gc.inputs(case)
    n = gc.rows(case)
    assert z.shape == (n, case.e) and cb.shape == (case.K, case.e) and z.dtype == cb.dtype == np.float32
    assert np.array_equal(z, again[0]) and np.array_equal(cb, again[1])
    ref = gc.reference(case)
    offs = gc.offsets(case)
    assert int(ref.grouped.sum()) == sum(case.sizes) and ref.reference_distance <= gc.MEASURED
    assert not ref.grouped[:case.head].any() and not ref.grouped[n - case.tail:].any()
    for pick in (1, 2, 3):                                           # numpy fp64; reversed sums, jittered exp; torch_ref.sinkhorn
        w, r, q = ref.winner.copy(), ref.runner.copy(), ref.ratio64.copy()
        for ev in ref.evaluations:
            lo, hi = offs[ev[0]], offs[ev[0] + 1]
            w[lo:hi], r[lo:hi], q[lo:hi] = ev[pick].winner, ev[pick].runner, ev[pick].ratio
        assert gc.judge(case, w, r, q) is None, pick
    for g, size in enumerate(case.sizes):                            # the degenerate 1 x K problem: index 0, then 1, all equal
        if size == 1:
            assert (ref.winner[offs[g]], ref.runner[offs[g]], ref.ratio64[offs[g]], ref.exact_one[offs[g]]) == (0, 1, 1.0, True)
    # a row of no group that was written, and a grouped row that was not
    w = ref.winner.copy()
    if case.head:
        w[0] = 0
        assert "belong to no group were written" in gc.judge(case, w, ref.runner, ref.ratio64)
    w = ref.winner.copy()
    w[offs[-1] - 1] = -1
    assert "winners differ on 1 of" in gc.judge(case, w, ref.runner, ref.ratio64)
    for hazard, exposed in gc.HAZARDS.items():
        groups = exposed(case)
        if not groups:
            continue
        verdict = gc.judge(case, *gc.perturbed(case, hazard, groups))
        assert verdict is not None, f"{gc.case_id(case)}: the judge accepts the reference with {hazard}"
        if hazard in ("tail_rows_left_out_of_column_sums", "highest_tied_index"):
            for g in groups:                                         # ... and confined to any one group
                assert gc.judge(case, *gc.perturbed(case, hazard, [g])) is not None, (hazard, g, case.sizes[g])


def test_the_recorded_tolerance_is_the_measured_one(ops):
    """MEASURED of the case module is the largest of the per-row reference distances, rounded up (and no more than a quarter above
    what this machine's long double and libm give); every hazard is carried by several rows; the exact ties the table is about are
    there in numbers; and the judge's message says where a wrong row sits."""
    refs = [gc.reference(c) for c in gc.CASES]
    measured = max(r.reference_distance for r in refs)
    assert measured <= gc.MEASURED <= 1.25 * measured, (measured, gc.MEASURED)
    for hazard, exposed in gc.HAZARDS.items():
        assert sum(bool(exposed(c)) for c in gc.CASES) >= 3, hazard
    ones = sum(int(r.exact_one.sum()) for r in refs)
    assert ones >= 200, ones
    assert any(c.iters == 1 and gc.HAZARDS["one_iteration_fewer"](c) for c in gc.CASES)
    case = gc.CASES[0]
    ref = gc.reference(case)
    runner = ref.runner.copy()
    row = int(gc.offsets(case)[15]) + 22                             # the last row of the 23-row group: in the column loop's tail
    runner[row] = 255
    msg = gc.judge(case, ref.winner, runner, ref.ratio64)
    assert f"runner-ups differ on 1 of 235 grouped rows, first row {row} = row 22 of group 15 (23 rows, class 2, 5888 entries, 7 rows" in msg
    ratio = ref.ratio64.copy()
    ratio[row] *= 1 + 1e-9
    msg = gc.judge(case, ref.winner, ref.runner, ratio)
    assert "second / best is beyond the tolerance on 1 rows" in msg and f"worst row {row} = row 22 of group 15" in msg
