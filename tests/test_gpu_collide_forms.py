"""MI355X: collision grouping (csrc/collide.hip, lcrec_collision_groups, ops.collision_groups) on every row of
tests/collide_cases.py against tests/collide_ref.py.

Every comparison is integer-exact: counters, members, offsets -- there is no tolerance anywhere in this file.  The C entry is called
through ctypes with buffers this file owns: outputs and the whole workspace are filled with a poison pattern first, what the entry
does not report must still hold it afterwards, and a second run in the same, now dirty, workspace must give the same answer."""
import time

import numpy as np
import pytest
import torch

import collide_cases as cc
from collide_ref import collide_ref, groups_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = 0x5AA55AA55AA55AA5        # no id, offset or count of any row
POISON_BYTE = 0xA5
GUARD = 16                         # poisoned words past the documented size of every output


def _dev(row_data):
    return torch.from_numpy(np.array(row_data)).to(DEV)


def _call(hip, d_idx, ks, members, offsets, counters, ws, ws_bytes):
    lib = hip._lib.load()
    n, L = d_idx.shape
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(DEV):
        rc = lib.lcrec_collision_groups(ptr(d_idx), n, L, hip.ops._ints(ks), ptr(members), ptr(offsets), ptr(counters), ptr(ws), ws_bytes,
                                        hip.ops._stream_ptr())
        hip._lib.check(rc, "lcrec_collision_groups")
        torch.cuda.synchronize()


def _expect(ref):
    return [ref["unique"], ref["n_groups"], len(ref["members"]), ref["max_count"]]


def _check_outputs(c, ref, members, offsets, counters, what):
    got = counters.cpu().numpy()
    print(c.name, what, "counters", got[:4].tolist(), "reference", _expect(ref))
    assert got[:4].tolist() == _expect(ref), (c.name, what)
    assert (got[4:] == POISON).all(), (c.name, what, "counters_out written past its four entries")
    c1, c2 = int(got[1]), int(got[2])
    m, o = members.cpu().numpy(), offsets.cpu().numpy()
    bad = np.flatnonzero(m[:c2] != ref["members"])
    assert bad.size == 0, (c.name, what, "members", bad[:8], m[bad[:8]], ref["members"][bad[:8]])
    assert np.array_equal(o[:c1 + 1], ref["offsets"]), (c.name, what, "offsets")
    assert (m[c2:] == POISON).all(), (c.name, what, "members_out written past counters[2]", np.flatnonzero(m[c2:] != POISON)[:8] + c2)
    assert (o[c1 + 1:] == POISON).all(), (c.name, what, "group_offsets_out written past counters[1] + 1",
                                          np.flatnonzero(o[c1 + 1:] != POISON)[:8] + c1 + 1)


@pytest.mark.parametrize("c", cc.ROWS, ids=cc.case_id)
def test_entry_matches_the_reference_in_poisoned_buffers(hip, c):
    ref = cc.expected(c)
    n, ks = c.n, list(c.ks)
    plan = hip.ops.collision_plan(n, ks)
    need = hip._lib.load().lcrec_collision_groups_workspace(n, len(ks))
    assert need == plan["workspace_bytes"]
    for field, want in c.plan:
        assert plan[field] == want, (c.name, field)
    t0 = time.perf_counter()
    d_idx = _dev(cc.data(c))
    new = lambda words: torch.full((words,), POISON, dtype=torch.int64, device=DEV)
    members, offsets, counters = new(n + GUARD), new(n // 2 + 2 + GUARD), new(4 + GUARD)
    ws = torch.full((need + 256,), POISON_BYTE, dtype=torch.uint8, device=DEV)

    _call(hip, d_idx, ks, members, offsets, counters, ws, need)
    _check_outputs(c, ref, members, offsets, counters, "first run")
    assert bool((ws[need:] == POISON_BYTE).all()), (c.name, "the workspace was written past the size the library asked for")

    # the same workspace again, as the first run left it
    members.fill_(POISON), offsets.fill_(POISON), counters.fill_(POISON)
    _call(hip, d_idx, ks, members, offsets, counters, ws, need)
    _check_outputs(c, ref, members, offsets, counters, "second run, dirty workspace")
    kept = (members.clone(), offsets.clone())

    # counters alone
    counters.fill_(POISON)
    _call(hip, d_idx, ks, None, None, counters, ws, need)
    got = counters.cpu().numpy()
    assert got[:4].tolist() == [ref["unique"], 0, 0, ref["max_count"]] and (got[4:] == POISON).all(), (c.name, "members_out == NULL")
    assert torch.equal(members, kept[0]) and torch.equal(offsets, kept[1])
    assert bool((ws[need:] == POISON_BYTE).all())
    assert np.array_equal(d_idx.cpu().numpy(), cc.data(c)), (c.name, "the index matrix was written")
    print(c.name, "n", n, "wall %.3f s (copy in, three runs, checks; the reference is computed once per row, outside)" % (time.perf_counter() - t0))


@pytest.mark.parametrize("c", cc.ROWS, ids=cc.case_id)
def test_ops_modes_match_the_reference(hip, c):
    ref = cc.expected(c)
    d_idx = _dev(cc.data(c))
    ks = list(c.ks)
    rate = (c.n - ref["unique"]) / c.n
    lists = hip.ops.collision_groups(d_idx, ks, want_groups=True)
    assert (lists["unique"], lists["max_count"], lists["n_groups"], lists["collision_rate"]) == (ref["unique"], ref["max_count"], ref["n_groups"], rate)
    assert lists["groups"] == groups_of(ref)
    dev = hip.ops.collision_groups(d_idx, ks, want_groups="device")
    assert (dev["unique"], dev["max_count"], dev["n_groups"], dev["collision_rate"]) == (ref["unique"], ref["max_count"], ref["n_groups"], rate)
    assert dev["members"].is_cuda and dev["offsets"].is_cuda and "groups" not in dev
    assert np.array_equal(dev["members"].cpu().numpy(), ref["members"]) and np.array_equal(dev["offsets"].cpu().numpy(), ref["offsets"])
    none = hip.ops.collision_groups(d_idx, ks, want_groups=False)
    assert none == {"unique": ref["unique"], "max_count": ref["max_count"], "collision_rate": rate}
    assert np.array_equal(d_idx.cpu().numpy(), cc.data(c))


@pytest.mark.parametrize("name", ["80 bits", "65 bits", "narrow", "clamp, 80 bits"])
def test_ops_takes_a_view_without_the_last_level(hip, name):
    """idx[:, :L-1] is not contiguous: the binding must group by the columns of the view, not by the memory under it."""
    c = next(r for r in cc.ROWS if r.name == name)
    d_idx = _dev(cc.data(c))
    view, ks = d_idx[:, :-1], list(c.ks[:-1])
    assert not view.is_contiguous()
    ref = collide_ref(cc.data(c)[:, :-1], ks)
    full = cc.expected(c)
    assert ref["unique"] <= full["unique"] and ref["n_groups"] > 0
    for mode in (True, "device", False):
        got = hip.ops.collision_groups(view, ks, want_groups=mode)
        assert (got["unique"], got["max_count"]) == (ref["unique"], ref["max_count"]), (name, mode)
        if mode == "device":
            assert np.array_equal(got["members"].cpu().numpy(), ref["members"]) and np.array_equal(got["offsets"].cpu().numpy(), ref["offsets"])
        elif mode:
            assert got["groups"] == groups_of(ref)
    assert np.array_equal(d_idx.cpu().numpy(), cc.data(c))


def test_no_items_write_one_offset_and_need_no_workspace(hip):
    new = lambda words: torch.full((words,), POISON, dtype=torch.int64, device=DEV)
    members, offsets, counters = new(GUARD), new(2 + GUARD), new(4 + GUARD)
    d_idx = torch.zeros((0, 3), dtype=torch.int64, device=DEV)
    _call(hip, d_idx, [16, 16, 16], members, offsets, counters, None, 0)
    assert counters.tolist() == [0, 0, 0, 0] + [POISON] * GUARD
    assert offsets.tolist() == [0] + [POISON] * (GUARD + 1) and members.tolist() == [POISON] * GUARD


@pytest.mark.parametrize("ks,total", cc.REFUSED_BITS)
def test_wider_than_128_bits_is_refused_and_launches_nothing(hip, ks, total):
    idx = torch.zeros((4, len(ks)), dtype=torch.int64, device=DEV)
    hip.ops.trace_enable(True)
    try:
        for mode in (True, "device", False):
            with pytest.raises(hip.LcrecError, match=r"tuples need %d bits \(> 128\)" % total) as err:
                hip.ops.collision_groups(idx, ks, want_groups=mode)
            assert err.value.code == hip._lib.EUNSUPPORTED
        torch.cuda.synchronize()
        assert hip.ops.trace_collect() == {}
    finally:
        hip.ops.trace_enable(False)
