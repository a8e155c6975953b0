"""CPU: every row of tests/sinkhorn_cases.py reaches the solver and the paths it claims -- asked of the library's own plan
(lcrec_debug_sinkhorn_plan: the function sinkhorn_big dispatches with, nothing launched) --, every row's inputs can be judged on
every row of the problem under the reference alone, the two measured numbers of the tolerance are what the case module records,
and the judge refuses the reference made wrong in each of the ways an argmax over Gaussian inputs would not show."""
import threading

import numpy as np
import pytest

import sinkhorn_cases as sk


@pytest.fixture(scope="module")
def ops():
    import lcrec_amd
    lcrec_amd._lib.load()
    return lcrec_amd.ops


def _in_thread(fn):
    """fn() in a thread of its own: the library's last-error text is per thread and is never cleared, and
    tests/test_host_logic.py::test_library_exports_every_declared_symbol asserts that the main thread's is still empty (as
    tests/test_cast_host.py and tests/test_dropout_host.py do for their refused calls)."""
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


@pytest.mark.parametrize("case", sk.CASES, ids=sk.case_id)
def test_row_reaches_what_it_claims(ops, case):
    p = sk.plan(case)
    bad = sk.check_claims(case, p)
    assert not bad, f"{sk.case_id(case)}:\n  " + "\n  ".join(bad) + f"\n  plan: {p}"
    # the numbers the plan reports, against the shape itself
    assert p["rows_per_workgroup"] == 8 * p["rw"] and p["workgroups"] == -(-case.B // p["rows_per_workgroup"])
    assert p["padded_columns"] == 64 * p["cpl"] - case.K and 0 <= p["padded_columns"] < 64 * p["cpl"]
    assert p["ragged_wave"] == (case.B % p["rw"] != 0) and p["ragged_workgroup"] == (case.B % p["rows_per_workgroup"] != 0)
    assert p["sets"] == (8 if p["form"] == sk.SCALING_LOCAL else 1)
    assert case.eps >= 0.0015 and np.isfinite(np.exp(1.0 / case.eps))               # exp(1 / eps) finite in fp64
    if case.form != sk.AUTO:
        assert p["form"] == case.form                                               # a forced form is that form or an error
    if p["form"] in sk.SCALING:
        assert case.K % 64 == 0 and (p["cpl"], p["rw"]) in sk.SCALING_PAIRS
    elif p["form"] == sk.PERSISTENT:
        assert (p["cpl"], p["rw"]) in sk.PERSISTENT_PAIRS and p["workgroups"] <= 128
    else:
        assert (p["cpl"], p["rw"], p["rows_per_workgroup"]) == (-(-case.K // 64), 4, 32)
    # the workspace the debug entry asks for is the one lcrec_sinkhorn_assign provides for the lone group it routes there
    if p["batch_route"]:
        import ctypes
        import lcrec_amd
        offs = (ctypes.c_int64 * 2)(0, case.B)
        assert p["workspace_bytes"] + 256 == lcrec_amd._lib.load().lcrec_sinkhorn_assign_workspace(case.B, case.K, offs, 1)


def test_every_path_is_claimed_by_a_row(ops):
    claimed = {name for case in sk.CASES for name in case.covers}
    assert not (claimed - set(sk.PROPERTIES)), claimed - set(sk.PROPERTIES)
    missing = sk.REQUIRED - claimed
    assert not missing, f"no row of sinkhorn_cases.CASES claims {sorted(missing)}: the path has lost its only test"
    for case in sk.CASES:
        assert case.covers, f"{sk.case_id(case)} claims no path"
        for key in ("form", "kernel", "workgroups", "sets"):
            assert key in case.expect, (sk.case_id(case), key)
    assert len({sk.case_id(c) for c in sk.CASES}) == len(sk.CASES)
    # every instantiation of both templates, but the one only LCREC_SK_RW=1 reaches, is some row's kernel -- by the plan
    ran = {(p["form"] in sk.SCALING, p["cpl"], p["rw"]) for p in map(sk.plan, sk.CASES) if p["form"] != sk.MULTI}
    assert {(c, r) for s, c, r in ran if s} == set(sk.SCALING_PAIRS) and len(sk.SCALING_PAIRS) == 16
    assert {(c, r) for s, c, r in ran if not s} == set(sk.PERSISTENT_PAIRS) and sk.PERSISTENT_KNOB_ONLY == [(4, 1)]
    assert any(sk.plan(c)["form"] == sk.MULTI for c in sk.CASES)
    # every row that stands for production's choice is a problem production gives to this solver
    for case in sk.CASES:
        if case.form == sk.AUTO:
            assert sk.plan(case)["batch_route"] == 1, sk.case_id(case)


def test_a_changed_row_fails_with_the_field_named(ops):
    case = next(c for c in sk.CASES if c.B == 300 and c.K == 192 and c.form == sk.AUTO and c.iters == 50 and c.stride == 1)
    p = sk.plan(case)
    assert sk.check_claims(case, p) == []
    for key, wrong, shown in (("form", sk.PERSISTENT, "form: the plan gives 1, the row says 3"),
                              ("kernel", (4, 8), "kernel: the plan gives (4, 4), the row says (4, 8)"),
                              ("workgroups", 11, "workgroups: the plan gives 10, the row says 11"),
                              ("sets", 1, "sets: the plan gives 8, the row says 1"),
                              ("padded", 0, "padded: the plan gives 64, the row says 0"),
                              ("ragged", (1, 1), "ragged: the plan gives (0, 1), the row says (1, 1)")):
        changed = case._replace(expect=dict(case.expect, **{key: wrong}))
        assert sk.check_claims(changed, p) == [shown]
    assert sk.check_claims(case._replace(covers=("persistent_padded",)), p) == ["property persistent_padded does not hold"]
    moved = case._replace(B=600)                                     # the shape changed under the row: the plan says what moved
    assert sk.check_claims(moved, sk.plan(moved)) == ["kernel: the plan gives (4, 8), the row says (4, 4)",
                                                      "property scaling_4_4 does not hold"]


def test_forced_forms_refuse_and_never_fall_through(ops):
    import lcrec_amd

    def refused(*args):
        def call():
            with pytest.raises(lcrec_amd.LcrecError) as info:
                ops.sinkhorn_plan(*args)
            return str(info.value)
        return _in_thread(call)
    assert "(-2)" in refused(130, 64, 50, sk.SCALING_LOCAL) and "form 1 cannot take" in refused(130, 64, 50, sk.SCALING_LOCAL)
    assert "form 2 cannot take" in refused(300, 100, 50, sk.SCALING_AGENT)                 # K % 64 != 0
    assert "form 3 cannot take" in refused(2048, 1024, 50, sk.PERSISTENT)                  # 256 workgroups of 8 rows
    assert "form 3 cannot take" in refused(4100, 48, 50, sk.PERSISTENT)
    assert "K=1025" in refused(300, 1025, 50, sk.MULTI)
    assert "(-1)" in refused(300, 192, 0, sk.AUTO) and "(-1)" in refused(300, 192, 50, 5)
    assert ops.sinkhorn_plan(4100, 48, 50, sk.MULTI)["form"] == sk.MULTI


@pytest.mark.parametrize("case", sk.CASES, ids=sk.case_id)
def test_row_inputs_are_judgeable_and_the_judge_refuses_wrong_solves(ops, case):
    """Under the reference alone: no row of the problem is near a tie for first or second place and no ratio is near the
    denormals, so the GPU test excludes nothing; the fp64 reference and the fp64 scaling form pass the judge; and the reference
    perturbed in each way the row is exposed to does not."""
    p = sk.plan(case)
    assert sk.conditions(case) == [], sk.case_id(case)
    z, cb = sk.inputs(case)
    again = sk.inputs(case)
    assert z.shape == (case.B, case.e) and cb.shape == (case.K, case.e) and z.dtype == cb.dtype == np.float32
    assert np.array_equal(z, again[0]) and np.array_equal(cb, again[1])
    ref = sk.reference(case)
    assert ref.reference_distance <= sk.MEASURED and ref.floor_distance <= sk.FLOOR, (ref.reference_distance, ref.floor_distance)
    cen = sk.centred(z, cb)
    for Q in (sk.solve(cen, case.eps, case.iters, np.float64), sk.solve_scaling(cen, case.eps, case.iters)):
        t = sk.top(Q)
        assert sk.judge(case, p, t.winner, t.runner, t.ratio) is None
    for hazard, exposed in sk.HAZARDS.items():
        if exposed(case, p):
            verdict = sk.judge(case, p, *sk.perturbed(case, p, hazard))
            assert verdict is not None, f"{sk.case_id(case)}: the judge accepts the reference with {hazard}"


def test_the_recorded_tolerance_is_the_measured_one(ops):
    """MEASURED and FLOOR of the case module are the largest of the per-row distances, rounded up (and no more than a quarter
    above what this machine's long double and libm give), every hazard
    is carried by some row, and the judge's message says where a wrong row sits."""
    refs = [sk.reference(c) for c in sk.CASES]
    measured, floor = max(r.reference_distance for r in refs), max(r.floor_distance for r in refs)
    assert measured <= sk.MEASURED <= 1.25 * measured, (measured, sk.MEASURED)
    assert floor <= sk.FLOOR <= 1.25 * floor, (floor, sk.FLOOR)
    for hazard, exposed in sk.HAZARDS.items():
        assert sum(bool(exposed(c, sk.plan(c))) for c in sk.CASES) >= 3, hazard
    case = next(c for c in sk.CASES if c.B == 300 and c.K == 192 and c.form == sk.SCALING_AGENT)
    p, y = sk.plan(case), sk.reference(case).yardstick
    runner = y.runner.copy()
    runner[299] = 200                                                # a padded column, in the ragged last workgroup
    msg = sk.judge(case, p, y.winner, runner, y.ratio)
    assert "runner-ups differ on 1 of 300 rows, first row 299: got 200" in msg and "scaling form, one set at agent scope" in msg
    assert "row 299: workgroup 9 of 10, wave 2, row 3 of the wave's 4" in msg
    assert "runner-up column 200: lane 8, lane-column 3 of 4, a PADDED column" in msg
    assert "the row sits in the ragged tail (rows from 288)" in msg
    ratio = y.ratio.copy()
    ratio[5] *= 1 + 1e-9
    msg = sk.judge(case, p, y.winner, y.runner, ratio)
    assert "second / best is off by" in msg and "(row 5:" in msg and "1 rows are beyond the tolerance" in msg
    assert "row 5: workgroup 0 of 10, wave 1, row 1 of the wave's 4" in msg and "does not sit in the ragged tail" in msg
