"""MI355X: every row of the nearest-free case table (tests/nearest_free_cases.py) once through its entry -- ops.finish_nearest_free,
ops.extend_nearest_free or ops.spill_nearest_free -- against the numpy rule of finish_ref.py, extend_ref.py or spill_ref.py.

Every comparison is exact: the kernels and the references evaluate the same fp32 operations and every tie is defined, so `idx`,
`moved` and `unresolved` must agree bit for bit -- there is no tolerance anywhere in this file.  tests/test_nearest_free_cases_host.py
proves on the CPU that each row reaches the paths it claims and that this judge refuses each of seven subtly wrong kernels.

Buffers (as tests/test_gpu_spill.py): idx carries 64 pre-filled guard rows past n, which must come back untouched; the residual rows
of the new items lie inside larger allocations with NaN-filled guard rows before them (n_frozen + 64) and after them.  Every row is
run a second time on the first call's output, with tables built from that output; the result must be the reference's on its own
output.  The largest_level_* rows first find the largest K their entry admits through the entry itself (no bucket listed: nothing
is launched) and compare it with the table's, which is derived from the LDS formulas."""
import numpy as np
import pytest
import torch

import extend_cases as ec
import nearest_free_cases as nc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
FILL = -7


def _table(groups):
    flat = [int(i) for g in groups for i in g]
    offs = np.cumsum([0] + [len(g) for g in groups])
    return torch.tensor(flat, dtype=torch.int64, device=DEV), torch.tensor(offs, dtype=torch.int64, device=DEV)


def _guarded(rows, n_frozen):
    pad = n_frozen + GUARD
    store = torch.full((pad + rows.shape[0] + pad, rows.shape[1]), float("nan"), dtype=torch.float32, device=DEV)
    store[pad:pad + rows.shape[0]] = torch.from_numpy(np.array(rows))
    return store[pad:pad + rows.shape[0]]


def _call(hip, row, idx):
    """one call of the row's entry on `idx`, with the tables of `idx` -> (tuples afterwards, moved, unresolved)"""
    inp = nc.inputs(row)
    n, L = idx.shape
    ks = list(row.ks)
    store_i = torch.full((n + GUARD, L), FILL, dtype=torch.int64, device=DEV)
    store_i[:n] = torch.from_numpy(np.array(idx))
    d_idx = store_i[:n]
    dev = lambda a: torch.from_numpy(np.array(a)).to(DEV)                            # (the shared inputs are read-only: a copy)
    if row.entry == "spill":
        tuples, supers = (_table(g) for g in nc.tables(row, idx))
        out = hip.ops.spill_nearest_free(d_idx, row.n_frozen, _guarded(inp["r2"], row.n_frozen), _guarded(inp["r1"], row.n_frozen),
                                         dev(inp["cb_prev"]), dev(inp["cb_last"]), ks, tuples, supers)
    else:
        members, offsets = _table(nc.tables(row, idx))
        resid = _guarded(inp["resid"], row.n_frozen)
        if row.entry == "extend":
            out = hip.ops.extend_nearest_free(d_idx, row.n_frozen, resid, dev(inp["cb"]), ks, members, offsets)
        else:
            out = hip.ops.finish_nearest_free(d_idx, resid, dev(inp["cb"]), ks, members, offsets)
    assert bool((store_i[n:] == FILL).all())                                      # the guard rows past n
    return d_idx.cpu().numpy(), out[0], out[1]


def _admits(hip, entry, K, e):
    """whether the entry takes a last level of K codes at L = 2: a call that lists no bucket, so nothing is launched"""
    idx = torch.zeros((1, 2), dtype=torch.int64, device=DEV)
    nobody = (torch.zeros(0, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV))
    resid, cb = torch.zeros((1, e), device=DEV), torch.zeros((K, e), device=DEV)

    def call():
        if entry == "extend":
            return hip.ops.extend_nearest_free(idx, 0, resid, cb, [2, K], *nobody)
        return hip.ops.finish_nearest_free(idx, resid, cb, [2, K], *nobody)
    try:
        assert ec.in_thread(call) == (0, 0)
        return True
    except hip.LcrecError as refusal:
        assert "does not fit" in str(refusal) and f"K={K}, e={e}" in str(refusal), str(refusal)
        return False


def _largest_admitted(hip, entry, e):
    lo, hi = 1, 4096                                                              # admitted, refused
    assert _admits(hip, entry, lo, e) and not _admits(hip, entry, hi, e)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if _admits(hip, entry, mid, e) else (lo, mid)
    return lo


@pytest.mark.parametrize("row", nc.ROWS, ids=nc.row_id)
def test_row_matches_the_reference_bit_for_bit_twice(hip, oracle, row):
    if set(row.covers) & set(nc.PER_ENTRY):
        found = _largest_admitted(hip, row.entry, row.e)
        print(row.entry, "e", row.e, "largest admitted K", found, "(derived:", nc.LARGEST[row.entry][row.e], ")")
        assert found == nc.LARGEST[row.entry][row.e] == row.ks[-1]
    inp, want = nc.inputs(row), nc.reference(row)
    got, moved, unresolved = _call(hip, row, inp["idx"])
    print(nc.row_id(row), "served", len(want.served), "moved", moved, "unresolved", unresolved, "(reference:", want.moved,
          want.unresolved, ")")
    assert (moved, unresolved) == (want.moved, want.unresolved)
    bad = np.flatnonzero((got != want.idx).any(axis=1))
    assert bad.size == 0, (bad[:8], got[bad[:8]], want.idx[bad[:8]], inp["idx"][bad[:8]])
    assert np.array_equal(got, want.idx)
    # the second call, on the first call's output
    again = nc.reference_again(row)
    got2, moved2, unresolved2 = _call(hip, row, got)
    assert (moved2, unresolved2) == (again.moved, again.unresolved)
    assert np.array_equal(got2, again.idx)
    if want.unresolved == 0:
        assert moved2 == 0 and np.array_equal(got2, got)                          # nothing moves
