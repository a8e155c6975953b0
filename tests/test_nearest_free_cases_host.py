"""CPU: the case table of the nearest-free kernels (tests/nearest_free_cases.py) under the numpy rules alone -- every row reaches the
paths it claims, every required property is claimed at every e_dim, the listed-buckets form of finish_ref is extend_ref's without
frozen items, and each wrong rule of tests/nearest_free_mutants.py is refused by every row that claims the matching property: the
judge of tests/test_gpu_nearest_free_forms.py (idx, moved, unresolved, bit for bit) would refuse such a kernel."""
import numpy as np
import pytest

import nearest_free_cases as nc
import nearest_free_mutants as nm
from extend_ref import extend_ref
from finish_ref import finish_ref


def _mutated(row, mutant):
    inp = nc.inputs(row)
    idx = inp["idx"]
    if row.entry == "spill":
        tg, sg = nc.tables(row, idx)
        out = nm.spill(idx, row.n_frozen, inp["r2"], inp["r1"], inp["cb_prev"], inp["cb_last"], tg, sg, mutant)
    else:
        out = nm.nearest_free(idx, row.n_frozen, inp["resid"], inp["cb"], nc.tables(row, idx), mutant)
    return nc.Result(out[0], tuple(out[1]), out[2], out[3])


def _same(a, b):
    """the GPU test's judge"""
    return np.array_equal(a.idx, b.idx) and (a.moved, a.unresolved) == (b.moved, b.unresolved)


def test_the_table_is_well_formed():
    ids = [nc.row_id(r) for r in nc.ROWS]
    assert len(set(ids)) == len(ids)
    for row in nc.ROWS:
        assert row.entry in ("finish", "extend", "spill") and row.e in nc.ES and row.covers, nc.row_id(row)
        assert set(row.covers) <= set(nc.PROPERTIES), nc.row_id(row)
        assert (row.entry == "finish") <= (row.n_frozen == 0) and 0 <= row.n_frozen <= row.n
    assert nc.REQUIRED == frozenset(nc.PROPERTIES) and all(p.__doc__ for p in nc.PROPERTIES.values())


@pytest.mark.parametrize("row", nc.ROWS, ids=nc.row_id)
def test_row_reaches_the_paths_it_claims_under_the_reference_alone(oracle, row):
    inp, res = nc.inputs(row), nc.reference(row)
    for name in row.covers:
        assert nc.PROPERTIES[name](row, inp, res), name
    # the plain consequences of the rules, on every row
    idx = inp["idx"]
    changed = np.flatnonzero((res.idx != idx).any(axis=1))
    assert len(changed) == res.moved and set(changed.tolist()) <= set(res.served) and len(res.served) == res.moved + res.unresolved
    assert np.array_equal(res.idx[:row.n_frozen], idx[:row.n_frozen]) and all(i >= row.n_frozen for i in res.served)
    fixed = len(row.ks) - (2 if row.entry == "spill" else 1)                          # the columns no pass ever writes
    assert np.array_equal(res.idx[:, :fixed], idx[:, :fixed])
    # the switchable restatement without a switch is the reference
    plain = _mutated(row, None)
    assert _same(plain, res) and plain.served == res.served
    # a second call on the result, with tables built from it: whoever could move has moved
    again = nc.reference_again(row)
    assert np.array_equal(again.idx, res.idx) and (again.moved, again.unresolved) == (0, res.unresolved)


@pytest.mark.parametrize("row", [r for r in nc.ROWS if r.entry == "finish"], ids=nc.row_id)
def test_finish_ref_with_listed_buckets_is_extend_ref_without_frozen_items(oracle, row):
    inp = nc.inputs(row)
    buckets = nc.tables(row, inp["idx"])
    a = finish_ref(inp["idx"], inp["resid"], inp["cb"], buckets=buckets)
    b = extend_ref(inp["idx"], 0, inp["resid"], inp["cb"], buckets=buckets)
    assert np.array_equal(a[0], b[0]) and list(a[1]) == list(b[1]) and a[2] == b[2]
    if inp["buckets"] is None:                                                        # ... and the default buckets are those groups
        c = finish_ref(inp["idx"], inp["resid"], inp["cb"])
        assert np.array_equal(a[0], c[0]) and sorted(a[1]) == sorted(c[1]) and a[2] == c[2]


def test_every_required_property_is_claimed_at_every_width():
    for e in nc.ES:
        rows = [r for r in nc.ROWS if r.e == e]
        claimed = {name for r in rows for name in r.covers}
        assert claimed == nc.REQUIRED, (e, sorted(nc.REQUIRED - claimed))
        for name in nc.PER_ENTRY:
            assert len([r for r in rows if name in r.covers]) == 1
    # the paths that every entry has are claimed by every entry, at every width
    for name in ("keeper_negative_distance", "keeper_nan", "mover_nan", "code_row_inf", "keeper_exact_tie", "free_exact_tie",
                 "out_of_range_members", "empty_bucket_listed", "walk_straddles_chunk", "walk_runs_out_mid_chunk",
                 "walk_whole_chunk_counted"):
        for entry in ("finish", "extend", "spill"):
            for e in nc.ES:
                assert any(name in r.covers for r in nc.ROWS if (r.entry, r.e) == (entry, e)), (name, entry, e)
    for name in ("frozen_holder_beats_nearest", "frozen_only_bucket_listed", "frozen_boundary_inside_chunk"):
        for entry in ("extend", "spill"):
            for e in nc.ES:
                assert any(name in r.covers for r in nc.ROWS if (r.entry, r.e) == (entry, e)), (name, entry, e)


@pytest.mark.parametrize("mutant", nm.MUTANTS)
def test_a_wrong_rule_is_refused_by_every_row_that_claims_its_property(oracle, mutant):
    props, entries = nc.MUTANT_OF[mutant]
    seen = set()
    for row in nc.ROWS:
        if row.entry in entries and set(props) & set(row.covers):
            assert not _same(_mutated(row, mutant), nc.reference(row)), (mutant, nc.row_id(row))
            seen.add((row.entry, row.e))
    assert seen == {(entry, e) for entry in entries for e in nc.ES}, (mutant, sorted(seen))


def test_the_largest_levels_of_the_table_follow_from_the_lds_formulas():
    for entry, by_e in nc.LARGEST.items():
        for e, K in by_e.items():
            assert nc.level_fits(entry, K, e) and not nc.level_fits(entry, K + 1, e), (entry, e, K)
            assert not any(nc.level_fits(entry, k, e) for k in range(K + 1, 4097)), (entry, e)
            row = [r for r in nc.ROWS if (r.entry, r.e) == (entry, e) and "largest_level_" + entry in r.covers]
            assert len(row) == 1 and row[0].ks == (2, K)
