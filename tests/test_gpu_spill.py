"""MI355X: the spill pass (lcrec_spill_nearest_free, ops.spill_nearest_free, generate(spill=True)).

Each case runs finish_ref (extend_ref with frozen items) then spill_ref on the CPU and ops.finish_nearest_free
(ops.extend_nearest_free) then ops.spill_nearest_free on the GPU.  Every comparison is exact: the kernels and tests/spill_ref.py
evaluate the same fp32 operations and every tie is defined, so `idx`, `moved` and `unresolved` must agree bit for bit -- there is no
tolerance anywhere in this file.

Buffers: idx carries 64 pre-filled guard rows past n, which must come back untouched; the residual rows of the new items lie inside
larger allocations with NaN-filled guard rows before them (n_frozen + 64) and after them.  A kernel that indexed the residuals by id
instead of id - n_frozen, in either direction, would read allocated NaNs and produce a wrong tuple; it could not read outside an
allocation."""
import json
import types

import numpy as np
import pytest
import torch

import extend_cases as ec
import golden_inputs as gi
import spill_cases as sc
from extend_ref import extend_ref
from finish_ref import colliding_items, finish_ref
from spill_ref import spill_ref, three_op

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
FILL = -7


def _table(groups):
    flat = [i for g in groups for i in g]
    offs = np.cumsum([0] + [len(g) for g in groups])
    return torch.tensor(flat, dtype=torch.int64, device=DEV), torch.tensor(offs, dtype=torch.int64, device=DEV)


def _listed(hip, d_idx, ks, cols):
    """(members, offsets) of the items sharing the first `cols` columns, the way generate_indices.spill_collisions builds them."""
    n = d_idx.shape[0]
    if cols == 0:
        return torch.arange(n, dtype=torch.int64, device=DEV), torch.tensor([0, n], dtype=torch.int64, device=DEV)
    found = hip.ops.collision_groups(d_idx[:, :cols].contiguous(), ks[:cols], want_groups="device")
    return found["members"], found["offsets"]


def _guarded(rows, n_frozen):
    pad = n_frozen + GUARD
    store = torch.full((pad + rows.shape[0] + pad, rows.shape[1]), float("nan"), dtype=torch.float32, device=DEV)
    store[pad:pad + rows.shape[0]] = torch.from_numpy(rows)
    return store[pad:pad + rows.shape[0]]


def _run(hip, idx, n_frozen, r2, r1, cb2, cb1, ks, listing=None, first="auto"):
    """r2 / r1 hold a row for every item; only the new items' rows reach the device.  -> (tuples after the first pass, its
    (moved, unresolved), tuples after the spill pass, moved, unresolved)."""
    n, L = idx.shape
    store_i = torch.full((n + GUARD, L), FILL, dtype=torch.int64, device=DEV)
    store_i[:n] = torch.from_numpy(idx)
    d_idx = store_i[:n]
    d_r2, d_r1 = _guarded(r2[n_frozen:], n_frozen), _guarded(r1[n_frozen:], n_frozen)
    d_cb2, d_cb1 = torch.from_numpy(cb2).to(DEV), torch.from_numpy(cb1).to(DEV)
    members, offsets = _listed(hip, d_idx, ks, L - 1)
    if first == "extend" or (first == "auto" and n_frozen):
        left = hip.ops.extend_nearest_free(d_idx, n_frozen, d_r1, d_cb1, ks, members, offsets)
    else:
        left = hip.ops.finish_nearest_free(d_idx, d_r1, d_cb1, ks, members, offsets)
    mid = d_idx.cpu().numpy().copy()
    if listing is None:
        tuples, supers = _listed(hip, d_idx, ks, L), _listed(hip, d_idx, ks, L - 2)
    else:
        tuples, supers = (_table(g) for g in listing(mid))
    moved, unresolved = hip.ops.spill_nearest_free(d_idx, n_frozen, d_r2, d_r1, d_cb2, d_cb1, ks, tuples, supers)
    assert bool((store_i[n:] == FILL).all())                                      # the guard rows past n
    return mid, left, d_idx.cpu().numpy(), moved, unresolved


def _check(hip, idx, n_frozen, r2, r1, cb2, cb1, ks, what="", listing=None):
    n, L = idx.shape
    if n_frozen:
        mid_w, _, left_w = extend_ref(idx, n_frozen, r1[n_frozen:], cb1)
    else:
        mid_w, _, left_w = finish_ref(idx, r1, cb1)
    tg, sg = listing(mid_w) if listing else (None, None)
    want, served, unres_w = spill_ref(mid_w, n_frozen, r2[n_frozen:], r1[n_frozen:], cb2, cb1, tg, sg)
    mid, left, got, moved, unresolved = _run(hip, idx, n_frozen, r2, r1, cb2, cb1, ks, listing)
    print(what, "first pass left", left[1], "| served", len(served), "moved", moved, "unresolved", unresolved, "(reference:",
          len(served) - unres_w, unres_w, ")")
    assert np.array_equal(mid, mid_w) and left[1] == left_w, what
    assert (moved, unresolved) == (len(served) - unres_w, unres_w), what
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]], mid[bad[:8]])
    # the stated consequences of the rule
    assert np.array_equal(got[:, :L - 2], idx[:, :L - 2])                          # columns 0 .. L-3 never change
    changed = np.flatnonzero((got != mid).any(1))
    assert len(changed) == moved and set(changed) <= set(served)                   # only movers' rows change
    assert np.array_equal(got[:n_frozen], idx[:n_frozen])                          # frozen rows: bit-identical
    cells, counts = np.unique(got, axis=0, return_counts=True)
    alone = {tuple(c) for c, k in zip(cells, counts) if k == 1}
    assert all(tuple(got[i]) in alone for i in changed)                            # a moved item collides with nobody
    if listing is None:
        assert colliding_items(got) == sc.colliding_among(idx, n_frozen) + unresolved
    return want, served, unres_w, mid_w, left_w


@pytest.mark.parametrize("n,ks", [(90, [8, 16]), (300, [3, 8, 16]), (200, [8, 48])])
@pytest.mark.parametrize("e", [16, 32, 64])
def test_overflowing_buckets_spill_into_their_super_bucket(hip, oracle, e, n, ks):
    idx, r2, r1, cb2, cb1 = sc.skewed_case(n, ks, e, seed=100 + n)
    want, served, unres, mid, left = _check(hip, idx, 0, r2, r1, cb2, cb1, ks, (e, n, ks))
    assert len(served) == left > 0 and unres == 0 and colliding_items(want) == 0


def test_one_cell_per_row(hip, oracle):
    """K1 = 1: every row has one cell, so the choice is made on level L-2 alone."""
    idx, r2, r1, cb2, cb1 = sc.skewed_case(100, [100, 1], 32, seed=200)
    want, served, unres, _, _ = _check(hip, idx, 0, r2, r1, cb2, cb1, [100, 1])
    assert len(served) > 50 and unres == 0 and sorted(want[:, 0].tolist()) == list(range(100)) and (want[:, 1] == 0).all()


def test_one_row_per_thread_exactly(hip, oracle):
    """K2 = 256 rows of 4 cells: the first round's candidates are one per thread."""
    idx, r2, r1, cb2, cb1 = sc.skewed_case(300, [256, 4], 16, seed=400)
    want, served, unres, _, _ = _check(hip, idx, 0, r2, r1, cb2, cb1, [256, 4])
    assert len(served) > 200 and unres == 0 and len(set(want[served, 0].tolist())) > 64


def test_more_cells_than_threads_and_a_ragged_bitmap_word(hip, oracle):
    """K1 = 300: a second trip over the cells, and 12 valid bits in the tenth occupancy word of a row."""
    idx, r2, r1, cb2, cb1 = sc.skewed_case(700, [3, 300], 16, seed=800)
    want, served, unres, _, _ = _check(hip, idx, 0, r2, r1, cb2, cb1, [3, 300])
    assert len(served) > 0 and unres == 0 and (want[:, 1] < 300).all()
    assert (want[served, 1] >= 256).any() and (want[served, 1] >= 288).any()        # cells of the second trip, and of the ragged word


def test_a_super_bucket_of_exactly_all_cells_and_one_of_three_more(hip, oracle):
    ks = [6, 8]
    idx, r2, r1, cb2, cb1 = sc.skewed_case(48, ks, 16, seed=48)
    want, served, unres, _, _ = _check(hip, idx, 0, r2, r1, cb2, cb1, ks)
    assert unres == 0 and sorted(map(tuple, want.tolist())) == [(a, k) for a in range(6) for k in range(8)]
    idx, r2, r1, cb2, cb1 = sc.skewed_case(51, ks, 16, seed=51)
    want, served, unres, _, _ = _check(hip, idx, 0, r2, r1, cb2, cb1, ks)
    assert unres == 3 and {tuple(t) for t in want.tolist()} == {(a, k) for a in range(6) for k in range(8)}
    assert np.array_equal(want[served[-3:]], _after_first(idx, r1, cb1)[served[-3:]])   # the last three served stay where they were


def test_free_cells_run_out_in_a_later_chunk(hip, oracle):
    """One super-bucket of 600 items on 40 cells (rows 0 .. 3, codes 0 .. 9) of 4 x 80 = 320, given to the pass as it stands --
    a first pass would fill every row: 280 free cells for about 560 movers.  The walk takes 256 positions at a time, so the last
    free cell goes in the second or third chunk, the movers behind it in that chunk are counted one by one, and at least one
    whole chunk starts with none left and is counted in parallel."""
    ks, e, n = [4, 80], 16, 600
    r = gi.rs(600)
    idx = np.stack([r.randint(0, 4, size=n), r.randint(0, 10, size=n)], axis=1).astype(np.int64)
    r2 = gi.f32(r.standard_normal((n, e)))
    cb2, cb1 = gi.f32(r.standard_normal((ks[0], e))), gi.f32(r.standard_normal((ks[1], e)))
    r1 = three_op(r2, cb2[idx[:, 0]])
    want, served, unres = spill_ref(idx, 0, r2, r1, cb2, cb1)
    assert unres > 0 and len(served) - unres == 280                                # the case does run out of free cells
    d_idx = torch.from_numpy(idx).to(DEV)
    moved, unresolved = hip.ops.spill_nearest_free(d_idx, 0, torch.from_numpy(r2).to(DEV), torch.from_numpy(r1).to(DEV),
                                                   torch.from_numpy(cb2).to(DEV), torch.from_numpy(cb1).to(DEV), ks,
                                                   _listed(hip, d_idx, ks, 2), _listed(hip, d_idx, ks, 0))
    print("served", len(served), "moved", moved, "unresolved", unresolved, "(reference:", len(served) - unres, unres, ")")
    assert (moved, unresolved) == (len(served) - unres, unres)
    got = d_idx.cpu().numpy()
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]], idx[bad[:8]])


def _after_first(idx, r1, cb1):
    return finish_ref(idx, r1, cb1)[0]


def test_over_full_super_buckets_leave_exactly_their_excess(hip, oracle):
    ks = [5, 12, 20]
    idx, r2, r1, cb2, cb1 = sc.skewed_case(1200, ks, 32, seed=1300)
    want, served, unres, _, _ = _check(hip, idx, 0, r2, r1, cb2, cb1, ks)
    sizes = np.bincount(idx[:, 0], minlength=5)
    assert unres == int(np.maximum(0, sizes - 240).sum()) > 0 and (sizes < 240).any()


@pytest.mark.parametrize("e", [16, 64])
def test_nine_movers_whose_nearest_row_is_the_same(hip, oracle, e):
    """Row 1, two free cells, is the nearest row with room of all nine: they must be served one after the other, each seeing what
    the others took -- two get row 1, the next four fill row 2, the last three go to row 3."""
    idx, r2, r1, cb2, cb1 = sc.nine_movers_case(e)
    d = oracle.distances(r2, cb2)
    assert (np.argmin(d[:, 1:], axis=1) == 0).all()                                 # row 1 is everybody's nearest after the full row 0
    want, served, unres, _, left = _check(hip, idx, 0, r2, r1, cb2, cb1, [6, 4], e)
    assert left == 9 == len(served) and unres == 0
    assert want[served, 0].tolist() == [1, 1, 2, 2, 2, 2, 3, 3, 3] and served == sorted(served)


def test_exact_ties_from_duplicated_rows(hip, oracle):
    """Duplicated codebook rows on both levels tie exactly as rows and as cells (the lowest code wins), duplicated residual rows
    tie exactly as holders (the lowest id keeps)."""
    idx, r2, r1, cb2, cb1 = sc.exact_ties_case()
    want, served, unres, _, _ = _check(hip, idx, 0, r2, r1, cb2, cb1, [6, 8])
    assert len(served) > 16 and unres == 0
    d2 = oracle.distances(r2, cb2)
    assert sum(1 for i in served if (d2[i] == d2[i, want[i, 0]]).sum() > 1) > 0     # the case does exercise exact ties
    assert (want[served[:8], 0] == want[served[0], 0]).all() and want[served[0], 0] in (1, 2)   # the lower of a duplicated pair first


@pytest.mark.parametrize("n,ks", [(2500, [40, 6, 10]), (3000, [300, 4, 6])])
def test_many_super_buckets_touched_and_untouched(hip, oracle, n, ks):
    """40 super-buckets of about 62 items on 60 cells: every one is touched and most are over-full.  300 super-buckets of about ten
    items on 24 cells: more workgroups than the device has CUs, a quarter of them touched.  Items that are not served stay bit for
    bit; two runs give identical bytes."""
    idx, r2, r1, cb2, cb1 = sc.skewed_case(n, ks, 32, seed=100 + n)
    want, served, unres, mid, _ = _check(hip, idx, 0, r2, r1, cb2, cb1, ks, (n, ks))
    touched = {int(idx[i, 0]) for i in served}
    supers = set(idx[:, 0].tolist())
    print("super-buckets", len(supers), "touched", len(touched))
    if ks[0] == 300:
        assert len(supers) > torch.cuda.get_device_properties(0).multi_processor_count and 40 < len(touched) < len(supers)
    else:
        assert len(touched) == len(supers) == 40
    still = np.ones(n, dtype=bool)
    still[served] = False
    assert np.array_equal(want[still], mid[still])
    again = _run(hip, idx, 0, r2, r1, cb2, cb1, ks)
    assert again[2].tobytes() == want.tobytes() and again[3:] == (len(served) - unres, unres)


def test_rows_are_gathered_by_id_not_by_position(hip, oracle):
    """One listed super-bucket of 40 ids far apart among 5000 items, with the shared tuples among them; the other 4960 items
    collide too but are not listed."""
    idx, r2, r1, cb2, cb1, ids = sc.scattered_case()
    listing = lambda mid: (sc.groups_of(mid, ids), [[int(i) for i in ids]])
    want, served, unres, mid, _ = _check(hip, idx, 0, r2, r1, cb2, cb1, [2, 6, 8], listing=listing)
    assert len(served) == 32 and unres == 0 and set(served) <= set(ids.tolist())
    assert colliding_items(want[ids]) == 0 and (want[ids, 0] == 0).all()


@pytest.mark.parametrize("n,ks,e", [(150, [8, 16], 16), (300, [3, 8, 16], 64)])
def test_frozen_items_never_move_and_no_row_is_read_for_them(hip, oracle, n, ks, e):
    """Two thirds of the items are frozen and collide among themselves; the new items' rows alone reach the device, between
    NaN-filled guard rows (see the module's docstring)."""
    idx, r2, r1, cb2, cb1 = sc.skewed_case(n, ks, e, seed=300 + n)
    n0 = 2 * n // 3
    r2[:n0] = np.nan                                                               # (the CPU rule does not look at them either)
    r1[:n0] = np.nan
    want, served, unres, mid, left = _check(hip, idx, n0, r2, r1, cb2, cb1, ks, (n, ks, e))
    assert len(served) == left > 0 and min(served) >= n0
    head, counts = np.unique(idx[:n0], axis=0, return_counts=True)
    new_tuples = {tuple(t) for t in mid[n0:].tolist()}
    only_frozen = [tuple(t) for t, c in zip(head.tolist(), counts) if c >= 2 and tuple(t) not in new_tuples]
    assert only_frozen                                                             # tuples held by frozen items only stay shared
    assert np.array_equal(want[:n0], idx[:n0]) and colliding_items(want) == sc.colliding_among(idx, n0) + unres


def test_without_frozen_items_both_first_passes_lead_to_the_same_result(hip, oracle):
    ks = [8, 16]
    idx, r2, r1, cb2, cb1 = sc.skewed_case(90, ks, 32, seed=190)
    plain = _run(hip, idx, 0, r2, r1, cb2, cb1, ks)
    frozen0 = _run(hip, idx, 0, r2, r1, cb2, cb1, ks, first="extend")
    assert plain[2].tobytes() == frozen0[2].tobytes() and plain[3:] == frozen0[3:] and plain[3] > 0
    # every item frozen: the counters are zeroed and nothing is touched
    d_idx = torch.from_numpy(idx).to(DEV)
    none = torch.zeros((0, 32), device=DEV)
    t = lambda a: torch.from_numpy(a).to(DEV)
    assert hip.ops.spill_nearest_free(d_idx, 90, none, none, t(cb2), t(cb1), ks, _listed(hip, d_idx, ks, 2), _listed(hip, d_idx, ks, 0)) == (0, 0)
    assert np.array_equal(d_idx.cpu().numpy(), idx)


def test_members_out_of_range_take_no_part(hip, oracle):
    """Listed groups that carry ids below 0 and past n, and items whose code of either level is out of range."""
    K2, K1, e, n = 3, 4, 16, 14
    r = gi.rs(71)
    codes = [(0, 0), (0, 0), (0, 1), (0, 2), (0, 3), (0, 0), (0, K1), (0, -1), (K2, 0), (-2, 0), (0, 0), (1, 1), (0, K1), (0, 0)]
    idx = np.array(codes, dtype=np.int64)
    r2 = gi.f32(r.standard_normal((n, e)))
    cb2, cb1 = gi.f32(r.standard_normal((K2, e))), gi.f32(r.standard_normal((K1, e)))
    r1 = three_op(r2, cb2[np.clip(idx[:, 0], 0, K2 - 1)])
    everybody = [-5, -1] + list(range(n)) + [n, n + 3, 1 << 40]
    listing = lambda mid: ([[-1, 0, 1, 5, 10, 13, n], [6, 12], [6, 7, 8, 9, 1 << 40]], [everybody])
    t = lambda a: torch.from_numpy(a).to(DEV)
    d_idx = t(idx)
    tuples, supers = (_table(g) for g in listing(idx))
    want, served, unres = spill_ref(idx, 0, r2, r1, cb2, cb1, *listing(idx))
    got = hip.ops.spill_nearest_free(d_idx, 0, t(r2), t(r1), t(cb2), t(cb1), [K2, K1], tuples, supers)
    assert len(served) == 4 and got == (4, 0) and np.array_equal(d_idx.cpu().numpy(), want)
    assert np.array_equal(want[[6, 7, 8, 9, 12]], idx[[6, 7, 8, 9, 12]])           # nobody out of range is written


def test_refusals_launch_nothing(hip):
    n, K = 64, 48
    idx = torch.zeros((n, 2), dtype=torch.int64, device=DEV)
    members = torch.arange(n, dtype=torch.int64, device=DEV)
    offsets = torch.tensor([0, n], dtype=torch.int64, device=DEV)
    both = (members, offsets)
    f = hip.ops.spill_nearest_free
    z = lambda *shape: torch.zeros(shape, device=DEV)

    def refused(match, *args):
        with pytest.raises(hip.LcrecError, match=match):
            ec.in_thread(f, *args)

    hip.ops.trace_enable(True)
    try:
        for e in (8, 24, 128):
            refused(f"e_dim={e}", idx, 4, z(n - 4, e), z(n - 4, e), z(K, e), z(K, e), [K, K], both, both)
        with pytest.raises(hip.LcrecError, match=r"levels 0 and 1 \(K=512 and K=256, e=64\) need 221696 B of LDS") as refusal:
            ec.in_thread(f, idx, 4, z(n - 4, 64), z(n - 4, 64), z(512, 64), z(256, 64), [512, 256], both, both)
        assert refusal.value.code == hip._lib.EUNSUPPORTED                         # what generate() turns into a warning
        flat = torch.zeros(n * 16 + 4, device=DEV)
        off = flat[1:1 + n * 16].view(n, 16)
        refused("must be 16-byte aligned", idx, 0, off, z(n, 16), z(K, 16), z(K, 16), [K, K], both, both)
        refused("must be 16-byte aligned", idx, 0, z(n, 16), off, z(K, 16), z(K, 16), [K, K], both, both)
        # what the binding itself refuses: one level, n_frozen out of range, one row per new item, shapes, host tensors, a strided matrix
        refused("L=1", idx[:, :1].contiguous(), 0, z(n, 16), z(n, 16), z(K, 16), z(K, 16), [K], both, both)
        refused("n_frozen=-1", idx, -1, z(n, 16), z(n, 16), z(K, 16), z(K, 16), [K, K], both, both)
        refused("n_frozen=65", idx, n + 1, z(0, 16), z(0, 16), z(K, 16), z(K, 16), [K, K], both, both)
        refused("one row per new item", idx, 4, z(n, 16), z(n - 4, 16), z(K, 16), z(K, 16), [K, K], both, both)
        refused("one row per new item", idx, 4, z(n - 4, 16), z(n - 4, 32), z(K, 16), z(K, 16), [K, K], both, both)
        refused("ks", idx, 4, z(n - 4, 16), z(n - 4, 16), z(K + 1, 16), z(K, 16), [K, K], both, both)
        refused("ks", idx, 4, z(n - 4, 16), z(n - 4, 16), z(K, 16), z(K, 16), [K, K + 1], both, both)
        refused("idx must be", idx.cpu(), 4, z(n - 4, 16), z(n - 4, 16), z(K, 16), z(K, 16), [K, K], both, both)
        refused("idx must be", torch.zeros((n, 4), dtype=torch.int64, device=DEV)[:, :2], 4, z(n - 4, 16), z(n - 4, 16), z(K, 16),
                z(K, 16), [K, K], both, both)
        refused("super_groups", idx, 4, z(n - 4, 16), z(n - 4, 16), z(K, 16), z(K, 16), [K, K], both, members)
        # nothing to do: no new item, no shared tuple listed, no super-bucket listed -- the counters are zeroed, nothing is launched
        none = (members[:0], offsets[:1])
        assert f(idx, n, z(0, 16), z(0, 16), z(K, 16), z(K, 16), [K, K], both, both) == (0, 0)
        assert f(idx, 4, z(n - 4, 16), z(n - 4, 16), z(K, 16), z(K, 16), [K, K], none, both) == (0, 0)
        assert f(idx, 4, z(n - 4, 16), z(n - 4, 16), z(K, 16), z(K, 16), [K, K], both, none) == (0, 0)
        torch.cuda.synchronize()
        assert hip.ops.trace_collect() == {}
        # ... and a call that does launch is traced under its two names, once each: 64 items on tuple (0, 0), four of them frozen
        assert f(idx, 4, z(n - 4, 16), z(n - 4, 16), z(K, 16), z(K, 16), [K, K], both, both) == (n - 4, 0)
        torch.cuda.synchronize()
        seen = hip.ops.trace_collect()
        assert sorted(seen) == ["spill_keepers", "spill_nearest_free"] and all(v[0] == 1 for v in seen.values())
    finally:
        hip.ops.trace_enable(False)
    assert int(idx[:4].abs().sum()) == 0 and colliding_items(idx.cpu().numpy()) == 3


def test_spill_collisions_lists_both_tables_itself(hip, oracle):
    from lcrec_amd import generate_indices as gen
    layer = lambda cb: types.SimpleNamespace(embedding=types.SimpleNamespace(weight=torch.from_numpy(cb).to(DEV)))
    for n, ks, supers, largest in ((90, [8, 16], 1, 90), (300, [3, 8, 16], 3, None)):
        idx, r2, r1, cb2, cb1 = sc.skewed_case(n, ks, 16, seed=100 + n)
        mid, _, left = finish_ref(idx, r1, cb1)
        want, served, unres = spill_ref(mid, 0, r2, r1, cb2, cb1)
        model = types.SimpleNamespace(rq=types.SimpleNamespace(vq_layers=[None] * (len(ks) - 2) + [layer(cb2), layer(cb1)]))
        d_idx = torch.from_numpy(mid).to(DEV)
        out = gen.spill_collisions(model, d_idx, 0, torch.from_numpy(r2).to(DEV), torch.from_numpy(r1).to(DEV), ks)
        largest = largest or int(np.bincount(idx[:, 0]).max())
        assert out == {"moved": len(served), "unresolved": 0, "super_buckets": supers, "largest_super_bucket": largest}
        assert np.array_equal(d_idx.cpu().numpy(), want)


# ---- end to end: the F6 checkpoint with its last codebook cut to its first 16 rows ------------------------------------------------
def _cut_checkpoint(tmp_path):
    items, ckpt = gi.toy_checkpoint(tmp_path, cut_last=sc.F6_CUT)
    return sc.f6_cut(), items, ckpt


def test_generate_with_spill_separates_every_item_of_the_cut_f6_model(hip, oracle, tmp_path):
    from lcrec_amd import generate_indices as gen
    f, items, ckpt = _cut_checkpoint(tmp_path)
    ks = [48, 48, sc.F6_CUT]
    file_a, file_b = str(tmp_path / "A.index.json"), str(tmp_path / "B.index.json")
    stats_a = gen.generate(ckpt, file_a, device="cuda:0", verbose=False, finish="nearest_free")
    assert not any(k.startswith("spill") or k == "largest_super_bucket" for k in stats_a)
    assert stats_a["finish_unresolved"] > 0 and stats_a["collision_rate"] > 0
    stats_b = gen.generate(ckpt, file_b, device="cuda:0", verbose=False, finish="nearest_free", spill=True)
    a = gen.load_index_json(file_a, ks)
    assert np.array_equal(a[:, :2], f["idx"][:, :2])                                # the rounds and the finishing pass move last codes only
    want, served, unres = spill_ref(a, 0, f["resid"][1], f["resid"][2], f["cbs"][1], f["cbs"][2])
    got = open(file_b, "rb").read()
    assert got == json.dumps({str(i): t for i, t in enumerate(gen.tokens_for(want.tolist()))}).encode()
    assert unres == 0 and stats_b["spill_unresolved"] == 0
    assert stats_b["spill_moved"] == stats_b["finish_unresolved"] == stats_a["finish_unresolved"] == len(served)
    assert stats_b["collision_rate"] == 0 and stats_b["max_conflicts"] == 1
    sizes = np.bincount(f["idx"][:, 0])
    assert stats_b["spill_super_buckets"] == int((sizes >= 2).sum()) and stats_b["largest_super_bucket"] == int(sizes.max())
    for k, v in stats_a.items():                                                    # without spill no statistic holds a changed value
        if k not in ("max_conflicts", "collision_rate"):
            assert stats_b[k] == v, k
    file_c = str(tmp_path / "C.index.json")
    stats_c = gen.generate(ckpt, file_c, device="cuda:0", verbose=False, finish="nearest_free", spill=True)
    assert open(file_c, "rb").read() == got and stats_c == stats_b


def test_generate_extend_with_spill_keeps_the_base_byte_for_byte(hip, oracle, tmp_path):
    """2000 base items indexed with --finish nearest_free --spill (no collision left), then 1000 new ones around them."""
    from lcrec_amd import generate_indices as gen
    f, items, ckpt = _cut_checkpoint(tmp_path)
    ks = [48, 48, sc.F6_CUT]
    n0, n = 2000, 3000
    npy0 = str(tmp_path / "Toy2000.emb.npy")
    np.save(npy0, items[:n0])
    base_file, out = str(tmp_path / "Base.index.json"), str(tmp_path / "Toy.index.json")
    s0 = gen.generate(ckpt, base_file, device="cuda:0", data_path=npy0, verbose=False, finish="nearest_free", spill=True)
    assert s0["items"] == n0 and s0["collision_rate"] == 0
    base_bytes = open(base_file, "rb").read()
    base = gen.load_index_json(base_file, ks)
    plain = gen.generate(ckpt, str(tmp_path / "Plain.index.json"), device="cuda:0", verbose=False, extend=base_file)
    assert plain["extend_unresolved"] > 0 and "spill_moved" not in plain
    stats = gen.generate(ckpt, out, device="cuda:0", verbose=False, extend=base_file, spill=True)
    got = open(out, "rb").read()
    assert got[:len(base_bytes) - 1] == base_bytes[:-1]                             # the base's bytes, without its closing brace
    after = gen.load_index_json(out, ks)
    assert np.array_equal(after[:n0], base)
    union = np.concatenate([base, f["idx"][n0:]])
    mid, _, left = extend_ref(union, n0, gi.f32(f["resid"][2][n0:]), f["cbs"][2])
    want, served, unres = spill_ref(mid, n0, gi.f32(f["resid"][1][n0:]), gi.f32(f["resid"][2][n0:]), f["cbs"][1], f["cbs"][2])
    assert np.array_equal(after, want)
    assert stats["extend_unresolved"] == plain["extend_unresolved"] == left == len(served) > 0
    assert (stats["spill_moved"], stats["spill_unresolved"]) == (len(served) - unres, unres) and unres == 0
    assert stats["collision_rate"] == 0 and stats["max_conflicts"] == 1 and stats["base_colliding"] == 0
