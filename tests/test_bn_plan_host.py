"""CPU: the plan of the BatchNorm strip launches (lcrec_debug_bn_plan: the function the five host entries of csrc/train_ops.hip
launch by, nothing launched) against the dispatch rules restated here in a few lines, over a grid of shapes, both alignments and
all five calls; and every row of tests/bn_cases.py gets, for every call, the form it is listed for."""
import pytest

import bn_cases as bn

NS = (1, 2, 255, 256, 257, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 100000)
FS = (1, 4, 30, 32, 36, 66, 126, 128, 252, 256, 508, 512, 516, 2048, 4096)


@pytest.fixture(scope="module")
def ops():
    import lcrec_amd
    lcrec_amd._lib.load()
    return lcrec_amd.ops


def rule(call, n, F, aligned):
    """The dispatch rules, independently of the C++: 1024 lanes per strip.  float4 strips (F % 4 == 0, aligned pointers,
    n * F < 2^29): width 16 from 512 columns, 8 from 256, else 4, halved while n exceeds 8 rows per lane, refused above that.
    dword strips otherwise: width 16; forward / backward halve it towards 8 while n exceeds 32 rows per lane, and keep the rows
    in registers from 1025 rows up to those 32 per lane."""
    form = None
    if F % 4 == 0 and aligned and n * F < 2 ** 29:
        cols = 16 if F >= 512 else (8 if F >= 256 else 4)
        while cols > 4 and n > 8 * (1024 // (cols // 4)):
            cols //= 2
        groups = 1024 // (cols // 4)
        if n <= 8 * groups:
            form = (1, cols, next(r for r in (1, 2, 4, 8) if n <= r * groups), 0)
    if form is None:
        cols = 16
        while call in ("forward", "backward") and cols > 8 and n > 32 * (1024 // cols):
            cols //= 2
        form = (0, cols, 0, int(call in ("forward", "backward") and 1025 <= n <= 32 * (1024 // cols)))
    grid = -(-F // form[1])
    return bn.Form(*form, grid, int(grid % 8 == 0))


def test_plan_is_the_rule_on_the_grid(ops):
    assert ops.BN_CALLS == bn.CALLS
    for call in bn.CALLS:
        for n in NS:
            for F in FS:
                for aligned in (True, False):
                    assert bn.Form(**ops.bn_plan(call, n, F, aligned)) == rule(call, n, F, aligned), (call, n, F, aligned)


@pytest.mark.parametrize("case", bn.CASES, ids=bn.case_id)
def test_row_gets_the_form_it_is_listed_for(ops, case):
    """With the alignment the row's calls have: all pointers on 16 bytes, but gamma where the row passes it as an offset view,
    and the exchange row of bn_stats."""
    takes_gamma = ("forward", "backward", "apply")
    for call, listed in (("forward", case.whole), ("backward", case.whole), ("stats", case.stats), ("reduce", case.reduce),
                         ("apply", case.apply)):
        aligned = not (case.gamma_off and call in takes_gamma)
        assert bn.Form(**ops.bn_plan(call, case.n, case.F, aligned)) == listed == rule(call, case.n, case.F, aligned), (call, case.why)
    assert bn.Form(**ops.bn_plan("stats", case.n, case.F, False)) == bn.stats_row_form(case)
    assert case.why


def test_the_table_reaches_every_form(ops):
    """Every instantiation the rules reach by default is some row's: the float4 (width, rows per lane) pairs and the dword widths,
    the dword ones both in the whole kernels and in the halves."""
    whole = {c.whole for c in bn.CASES}
    assert {(f.cols, f.rows_per_lane) for f in whole if f.float4} >= {(w, r) for w in (4, 8, 16) for r in (1, 2, 4, 8)}
    assert {(f.cols, f.cached) for f in whole if not f.float4} == {(8, 0), (8, 1), (16, 0), (16, 1)}
    assert {f.xcd_order for f in whole if f.float4} == {f.xcd_order for f in whole if not f.float4} == {0, 1}
    for halves in ({c.stats for c in bn.CASES}, {c.reduce for c in bn.CASES}, {c.apply for c in bn.CASES}):
        assert {f.float4 for f in halves} == {0, 1}
    assert len({bn.run_id(r) for r in bn.runs()}) == len(bn.runs()) == len(bn.CASES) + 2


def test_row_inputs_are_judgeable_under_fp64_alone():
    """bn_cases.inputs() asserts its own conditions; here: it is deterministic and leaves no row out."""
    import numpy as np
    for case in bn.CASES[:3] + [c for c in bn.CASES if c.n == 2]:
        first = [a.copy() for a in bn.inputs(case)]
        bn.inputs.cache_clear()
        for a, b in zip(first, bn.inputs(case)):
            assert a.dtype == np.float32 and np.array_equal(a, b)
        t, gamma, beta = first[:3]
        assert np.abs(bn.preactivation(t, gamma, beta)).min() >= bn.MARGIN
