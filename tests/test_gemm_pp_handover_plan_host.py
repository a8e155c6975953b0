"""CPU: every row of tests/gemm_pp_handover_cases.py has the launch plan it claims (lcrec_debug_linear_forward_plan for
256 CUs, nothing launched), the rows add the switch combinations tests/gemm_pp_cases.py lacks, and the special-value inputs
hold what they say -- by the oracle, -0.0 does reach the ReLU and comes out as +0.0."""
import numpy as np
import pytest

import gemm_pp_cases as pp
import gemm_pp_handover_cases as ho

CUS = 256


@pytest.mark.parametrize("case", ho.CASES + [ho.SPECIAL], ids=pp.case_id)
def test_row_plan_is_what_it_claims(case):
    launches = pp.plan(case.n, case.k, case.out, CUS)
    bad = ho.check_claims(case, launches)
    assert not bad, f"{pp.case_id(case)} on {CUS} CUs:\n  " + "\n  ".join(bad) + f"\n  plan: {launches}"
    head = launches[0]
    assert len(launches) == 1 and head["workgroups"] == CUS and head["k_tiles"] == case.k // 32
    assert head["tiles"] == (case.n // 256) * (case.out // 128)
    for key in ("form", "head", "tail", "k_tiles", "steady", "lists", "empty", "last_panel"):
        assert key in case.expect, (pp.case_id(case), key)


def test_rows_add_what_the_first_table_lacks():
    have = {(c.relu, c.bn, c.bias) for c in pp.CASES if c.expect["form"] == pp.PERSISTENT}
    new = {(c.relu, c.bn, c.bias) for c in ho.CASES}
    assert len(have | new) == 8, sorted(have | new)                 # every instantiation of the persistent kernel
    assert {(False, True, False), (False, False, False)} <= new - have
    claimed = {name for c in ho.CASES for name in c.covers}
    assert set(ho.EXTRA_PROPERTIES) <= claimed
    assert len({pp.case_id(c) for c in ho.CASES}) == len(ho.CASES)
    # XCD holes as the row says: 12 row panels numbered over 16
    holes = next(c for c in ho.CASES if "pp3_xcd_holes" in c.covers)
    assert (holes.n // 256, holes.out // 128) == (12, 64)


def test_xcd_hole_row_counts():
    holes = next(c for c in ho.CASES if "pp3_xcd_holes" in c.covers)
    head = pp.plan(holes.n, holes.k, holes.out, CUS)[0]
    assert (head["tiles"], head["virtual_tiles"]) == (768, 1024), head


def test_special_inputs(oracle):
    x, W, b, sc, sh, rows = ho.special_inputs()
    c = ho.SPECIAL
    assert x.shape == (c.n, c.k) and W.shape == (c.out, c.k) and all(v.shape == (c.out,) for v in (b, sc, sh))
    first, last = [r for r in rows if r < 256], [r for r in rows if r >= c.n - 256]
    assert len(first) == len(last) == len(ho.SPECIAL_ROWS) and len(first) + len(last) == len(rows)
    for panel in (first, last):
        kinds = {rows[r] for r in panel}
        assert {"nan", "+inf", "-inf", "zero", "one +inf", "one -inf"} <= kinds
    for r, kind in rows.items():
        if kind == "nan":
            assert np.isnan(x[r]).all()
        elif kind in ("+inf", "-inf"):
            assert (x[r] == np.float32(kind)).all()
        elif kind == "zero":
            assert (x[r].view(np.uint32) == 0).all()
        else:
            assert np.isinf(x[r]).sum() == 1
    assert np.isfinite(np.delete(x, sorted(rows), axis=0)).all() and np.isfinite(W).all()
    zc = ho.NEG_SCALE_ZERO_COLUMNS
    assert (b[zc] == 0).all() and (sc[zc] < 0).all() and (sh[zc].view(np.uint32) == 0x80000000).all()
    negative = np.zeros(c.out, dtype=bool)
    negative[zc] = negative[ho.NEG_SCALE_COLUMNS] = True
    assert (sc[negative] < 0).all() and (sc[~negative] > 0).all()
    # by the oracle: a zero row reaches the ReLU as -0.0 in those columns, and leaves it as +0.0; NaN leaves it as +0.0
    sub = sorted(rows)
    pre = oracle.linear(x[sub], W, b, sc, sh, relu=False)
    post = oracle.linear(x[sub], W, b, sc, sh, relu=True)
    zero = [i for i, r in enumerate(sub) if rows[r] == "zero"]
    nan = [i for i, r in enumerate(sub) if rows[r] == "nan"]
    assert (pre[zero][:, zc].view(np.uint32) == 0x80000000).all() and (post[zero][:, zc].view(np.uint32) == 0).all()
    assert np.isnan(pre[nan]).all() and (post[nan].view(np.uint32) == 0).all()
    one = [i for i, r in enumerate(sub) if rows[r].startswith("one")]
    assert np.isposinf(post[one]).any() and not np.isnan(post).any() and not (post.view(np.uint32) == 0x80000000).any()
