"""CPU: the capture table (tests/capture_cases.py) under the numpy references alone.  A graph replay is judged by what lies in the
output buffers afterwards, so the table has to make three things impossible to confuse: a replay that ran on the new inputs, one
that ran on the inputs of the capture, and one that ran nothing.  For every row: input sets A and B share every host-side argument
(a graph bakes those in); their expected results differ on many items; and the judge of tests/test_gpu_capture_forms.py refuses A's
result offered as B's, B's as A's, and the garbage fill of the output buffers as either."""
import numpy as np
import pytest

import beam_cases as bc
import capture_cases as cc
from beam_ref import beam_ref


def test_the_table_has_one_row_per_entry_and_width():
    assert [(r.entry, r.e) for r in cc.ROWS] == [(entry, e) for entry in cc.ENTRIES for e in (16, 32, 64)]
    assert cc.ENTRIES == ("finish", "extend", "spill", "rq_audit", "rq_beam") and len({cc.row_id(r) for r in cc.ROWS}) == 15
    for row in cc.ROWS:
        if row.entry in ("finish", "extend", "spill"):
            nrow = cc.nearest_free_row(row)
            want = {"finish": ((3, 48), 96, 0), "extend": ((3, 48), 96, 32), "spill": ((6, 40), 218, 0)}[row.entry]
            assert (nrow.ks, nrow.n, nrow.n_frozen) == want and nrow.e == row.e


@pytest.mark.parametrize("row", cc.ROWS, ids=cc.row_id)
def test_both_input_sets_share_every_host_side_argument(oracle, row):
    a, b = cc.variant(row, "A"), cc.variant(row, "B")
    assert a.host == b.host and a.host["e"] == row.e
    assert list(a.inputs) == list(b.inputs) and list(a.expected) == list(b.expected)
    for name in a.inputs:
        assert a.inputs[name].shape == b.inputs[name].shape and a.inputs[name].dtype == b.inputs[name].dtype, name
    for name in a.expected:
        assert a.expected[name].shape == b.expected[name].shape and a.expected[name].dtype == b.expected[name].dtype, name
    # what B changes, and nothing else: the data a graph does not bake in
    changed = {name for name in a.inputs if not np.array_equal(a.inputs[name], b.inputs[name], equal_nan=True)}
    assert changed == {"finish": {"resid"}, "extend": {"resid"}, "spill": {"r2", "r1"}, "rq_audit": {"idx_wide"}, "rq_beam": {"z"}}[row.entry]
    if row.entry in ("finish", "extend"):
        assert np.array_equal(b.inputs["resid"], -a.inputs["resid"]) and a.inputs["resid"].shape == (a.host["n"] - a.host["n_frozen"], row.e)
        assert a.host["n_buckets"] == 3 == len(a.inputs["offsets"]) - 1
    if row.entry == "spill":
        assert np.array_equal(b.inputs["r2"], -a.inputs["r2"]) and (a.host["n_tuple_groups"], a.host["n_super_groups"]) == (3, 1)
        assert a.host["super_members"] == 218 > 64
    if row.entry == "rq_audit":
        L = len(a.host["ks"])
        assert a.inputs["idx_wide"].shape == (257, L + 2) == (a.host["n"], a.host["idx_stride"])
        assert (a.expected["rank"] > 0).any() and (b.expected["rank"] == 0).all()     # random tuples against the greedy ones
    if row.entry == "rq_beam":
        assert np.array_equal(b.inputs["z"], a.inputs["z"][::-1]) and a.host["width"] == 4
        assert (row.e, a.host["ks"], 4, a.host["n"]) in bc.shapes()                  # A's reference is the beam table's own


@pytest.mark.parametrize("row", cc.ROWS, ids=cc.row_id)
def test_the_expected_results_differ_and_the_judge_tells_them_apart(oracle, row):
    a, b = cc.variant(row, "A"), cc.variant(row, "B")
    differ = cc.rows_differing(a.expected, b.expected)
    if row.entry in ("finish", "extend", "spill"):
        start = a.inputs["idx"]
        moved_a = int((a.expected["idx"] != start).any(axis=1).sum())
        moved_b = int((b.expected["idx"] != start).any(axis=1).sum())
        print(cc.row_id(row), "rows that differ between A's and B's result:", differ, "; A's call changes", moved_a, ", B's", moved_b)
        assert moved_a == a.expected["counters"][0] > 0 and moved_b == b.expected["counters"][0] > 0
        assert 2 * differ >= moved_a
    else:
        n = a.host["n"]
        print(cc.row_id(row), "rows that differ between A's and B's result:", differ, "of", n)
        assert 2 * differ >= n
    # the judge: its own result passes, the other set's does not, and neither does a buffer nobody wrote
    assert cc.judge(a.expected, a.expected) and cc.judge(b.expected, b.expected)
    assert not cc.judge(a.expected, b.expected) and not cc.judge(b.expected, a.expected)
    garbage = cc.garbage_like(a.expected)
    assert not cc.judge(garbage, a.expected) and not cc.judge(garbage, b.expected)
    for name in a.expected:                                                           # ... output by output: each one is told apart
        assert not cc.same_bits(garbage[name], a.expected[name]) and not cc.same_bits(garbage[name], b.expected[name]), name
    if row.entry in ("finish", "extend", "spill"):                                   # a replay that left the starting idx alone
        assert not cc.same_bits(a.inputs["idx"], a.expected["idx"]) and not cc.same_bits(a.inputs["idx"], b.expected["idx"])
    missing = {name: v for name, v in a.expected.items() if name != "err"}
    assert row.entry in ("finish", "extend", "spill") or not cc.judge(missing, a.expected)


@pytest.mark.parametrize("e", cc.ES)
def test_the_reversed_beam_reference_is_the_reference_of_the_reversed_items(oracle, e):
    """Items are independent under the rule, which is what lets B's reference be A's reversed: checked against beam_ref itself."""
    b = cc.variant(cc.Row("rq_beam", e), "B")
    _, cbs, _ = bc.inputs(e, cc.KS_WALK, cc.N_WALK)
    direct = beam_ref(b.inputs["z"], cbs, cc.BEAM_W)
    assert cc.judge({name: direct[name] for name in cc.BEAM_NAMES}, b.expected)
