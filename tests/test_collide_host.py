"""CPU: the host side of collision grouping (csrc/collide.hip, lcrec_collision_groups) -- every row of tests/collide_cases.py has the
properties it is listed for and the plan it claims (asked of the library's own lcrec_debug_collision_plan, by which the entry runs),
tests/collide_ref.py agrees with the dict-based helpers it restates, and the entry's refusals come back before a device is touched."""
import ctypes
import os
import re
import threading

import numpy as np
import pytest

import collide_cases as cc
from collide_ref import clamp, collide_ref, groups_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_ROWS = [c for c in cc.ROWS if c.n <= cc.SMALL]


def _plan(c):
    import lcrec_amd
    return lcrec_amd.ops.collision_plan(c.n, c.ks)


def test_header_declares_and_library_exports_the_plan_entry():
    import lcrec_amd
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lcrec.h")).read(), flags=re.S)
    assert re.search(r"\blcrec_debug_collision_plan\s*\(", header)
    assert "lcrec_debug_collision_plan" in lcrec_amd._lib.EXPORTS and hasattr(lcrec_amd._lib.load(), "lcrec_debug_collision_plan")
    assert lcrec_amd._lib.MAX_LEVELS == cc.MAX_LEVELS
    text = open(os.path.join(ROOT, "include", "lcrec.h")).read()
    assert "v < 0 counts as 0" in text and "entries 1 and 2 are 0 when members_out is NULL" in text


def test_required_properties_are_claimed_and_names_are_known():
    claimed = {k for c in cc.ROWS for k in c.covers}
    assert claimed <= set(cc.PROPERTIES), claimed - set(cc.PROPERTIES)
    assert set(cc.REQUIRED) <= claimed, set(cc.REQUIRED) - claimed
    assert len({cc.case_id(c) for c in cc.ROWS}) == len(cc.ROWS)
    # what the issue names, by the name it has here
    for name in ("lo_equal_hi_differs", "hi_equal_lo_differs", "straddle", "straddle_upper_only", "straddle_lower_only", "straddle_both",
                 "bit63", "bit127", "zero_bits", "max_groups_even", "max_groups_odd", "id_bits_9_late_group", "id_bits_10_late_group",
                 "sort_single_block", "sort_merge", "sort_onesweep", "clamp"):
        assert name in cc.REQUIRED, name
    big = [c for c in cc.ROWS if c.n > cc.SMALL]
    assert [(c.n, list(c.ks)) for c in big] == [(2 ** 20 + 1, [256] * 3), (2 ** 20 + 1, [1024] * 8)]     # the only large rows


@pytest.mark.parametrize("c", cc.ROWS, ids=cc.case_id)
def test_row_has_the_properties_and_the_plan_it_claims(c):
    plan = _plan(c)
    for name in c.covers:
        assert cc.PROPERTIES[name](c, plan), (c.name, name)
    rows = cc.data(c)
    assert rows.dtype == np.int64 and rows.shape == (c.n, len(c.ks)) and rows.flags.c_contiguous
    if "clamp" not in c.covers:
        assert (rows >= 0).all() and (rows < np.asarray(c.ks)[None, :]).all()
    # the plan: what the row claims, what the rule of include/lcrec.h gives, and the sizes that hang together
    for field, want in c.plan:
        assert plan[field] == want, (c.name, field, plan[field], want)
    assert plan["bits"] == cc.bits_of(c.ks) and plan["total_bits"] == sum(plan["bits"])
    assert plan["stride"] % 256 == 0 and 0 <= plan["stride"] - 8 * c.n < 256
    assert plan["temp_bytes"] > 0 and plan["workspace_bytes"] == 10 * plan["stride"] + plan["temp_bytes"]
    import lcrec_amd
    assert lcrec_amd._lib.load().lcrec_collision_groups_workspace(c.n, len(c.ks)) == plan["workspace_bytes"]


def test_plan_at_the_edges_of_its_rule():
    import lcrec_amd
    plan = lcrec_amd.ops.collision_plan
    assert [plan(n, [4])["id_bits"] for n in (0, 1, 2, 3, 4, 5, 256, 257, 2 ** 31, 2 ** 31 + 1)] == [1, 1, 1, 2, 2, 3, 8, 9, 31, 32]
    assert plan(0, [4])["workspace_bytes"] == plan(1, [4])["workspace_bytes"]
    for ks, total, lo, hi in (([1], 0, 1, 0), ([2], 1, 1, 0), ([3], 2, 2, 0), ([2 ** 31 - 1] * 2, 62, 62, 0), ([2 ** 16] * 4, 64, 64, 0),
                              ([2 ** 16] * 4 + [2], 65, 64, 1), ([2 ** 16 + 1] * 4, 68, 64, 4), ([2 ** 16] * 8, 128, 64, 64),
                              ([1] * 16, 0, 1, 0)):
        p = plan(7, ks)
        assert (p["total_bits"], p["lo_bits"], p["hi_bits"]) == (total, lo, hi), ks


@pytest.mark.parametrize("c", SMALL_ROWS, ids=cc.case_id)
def test_reference_equals_the_dict_helpers(c):
    """collide_ref against generate_indices.get_collision_item / get_indices_count and oracle/generate_ref.collision_groups, on the
    clamped tuples (the helpers know no clamp: it is applied to their input)."""
    from lcrec_amd import generate_indices as gen
    from oracle import generate_ref
    ref = cc.expected(c)
    keys = [tuple(r) for r in clamp(cc.data(c), c.ks).tolist()]
    counts = gen.get_indices_count(keys)
    want = gen.get_collision_item(keys)
    assert groups_of(ref) == want == generate_ref.collision_groups(keys)
    assert ref["unique"] == len(counts) and ref["max_count"] == max(counts.values())
    assert ref["n_groups"] == len(want) and ref["offsets"][-1] == len(ref["members"]) == sum(len(g) for g in want)
    assert gen.check_collision(keys) == (ref["n_groups"] == 0)
    assert sorted(keys[i] for i in ref["firsts"].tolist()) == sorted(counts)


def test_reference_on_cases_written_out_by_hand():
    ks = [4, 3]
    idx = np.array([[3, 2], [0, 0], [3, 2], [1, 1], [0, 0], [3, 2], [2, 2]], dtype=np.int64)
    ref = collide_ref(idx, ks)
    assert (ref["unique"], ref["max_count"], ref["n_groups"]) == (4, 3, 2)
    assert ref["members"].tolist() == [0, 2, 5, 1, 4] and ref["offsets"].tolist() == [0, 3, 5] and ref["firsts"].tolist() == [0, 1, 3, 6]
    # the clamp: -1 and INT64_MIN are code 0; K, 2^40 are code K - 1; nothing else moves
    idx = np.array([[-1, 0], [0, -2 ** 63], [0, 0], [4, 3], [2 ** 40, 2], [3, 1], [1, 0]], dtype=np.int64)
    ref = collide_ref(idx, ks)
    assert groups_of(ref) == [[0, 1, 2], [3, 4]] and ref["unique"] == 4 and ref["max_count"] == 3
    empty = collide_ref(np.zeros((0, 2), dtype=np.int64), ks)
    assert (empty["unique"], empty["max_count"], empty["n_groups"]) == (0, 0, 0) and empty["offsets"].tolist() == [0]
    one = collide_ref(np.zeros((1, 2), dtype=np.int64), ks)
    assert (one["unique"], one["max_count"], one["n_groups"]) == (1, 1, 0) and one["offsets"].tolist() == [0] and len(one["members"]) == 0


def test_entry_refuses_before_the_device_is_touched():
    """Every refusal below returns from the argument checks: the pointers are host addresses that a launch or a memset could not
    take, and no device is present where this test runs.  (In a thread of its own: the library's last-error text is per thread.)"""
    import lcrec_amd
    lib = lcrec_amd._lib.load()
    EINVAL, EUNSUPPORTED, EWORKSPACE = (lcrec_amd._lib.CONSTANTS[k] for k in ("LCREC_EINVAL", "LCREC_EUNSUPPORTED", "LCREC_EWORKSPACE"))
    seen = []

    def calls():
        buf = (ctypes.c_int64 * 64)()
        p = ctypes.c_void_p(ctypes.addressof(buf))
        ints = lambda *v: (ctypes.c_int * len(v))(*v)
        need = lib.lcrec_collision_groups_workspace(8, 3)

        def call(code, word, idx=p, n=8, L=3, K=ints(48, 48, 48), mem=p, off=p, counters=p, ws=p, ws_bytes=need):
            rc = lib.lcrec_collision_groups(idx, n, L, K, mem, off, counters, ws, ws_bytes, None)
            seen.append((rc, code, word, lib.lcrec_last_error()))

        call(EINVAL, b"bad n or L", L=0)
        call(EINVAL, b"bad n or L", L=cc.MAX_LEVELS + 1, K=ints(*[2] * (cc.MAX_LEVELS + 1)))
        call(EINVAL, b"bad n or L", n=-1)
        call(EINVAL, b"K[1]=0", K=ints(48, 0, 48))
        call(EINVAL, b"K[2]=-5", K=ints(48, 48, -5))
        for ks, total in cc.REFUSED_BITS:
            call(EUNSUPPORTED, b"tuples need %d bits (> 128)" % total, L=len(ks), K=ints(*ks))
        call(EINVAL, b"members_out and offsets_out go together", off=None)
        call(EINVAL, b"members_out and offsets_out go together", mem=None)
        call(EWORKSPACE, b"workspace %d B < required %d B" % (need - 1, need), ws_bytes=need - 1)
        call(EWORKSPACE, b"workspace 0 B < required", ws_bytes=0)
        call(EWORKSPACE, b"< required", ws=None)
        call(EINVAL, b"NULL pointer", idx=None)
        call(EINVAL, b"NULL pointer", K=None)
        call(EINVAL, b"NULL pointer", counters=None)
        plan = lcrec_amd._lib.CollisionPlan()
        out = ctypes.c_void_p(ctypes.addressof(plan))
        for code, word, args in ((EINVAL, b"bad n or L", (8, 0, ints(4), out)), (EINVAL, b"bad n or L", (-1, 1, ints(4), out)),
                                 (EINVAL, b"K[0]=0", (8, 1, ints(0), out)), (EINVAL, b"NULL pointer", (8, 1, None, out)),
                                 (EINVAL, b"NULL pointer", (8, 1, ints(4), None)),
                                 (EUNSUPPORTED, b"129 bits", (8, 9, ints(*cc.REFUSED_BITS[0][0]), out))):
            seen.append((lib.lcrec_debug_collision_plan(*args), code, word, lib.lcrec_last_error()))

    worker = threading.Thread(target=calls)
    worker.start()
    worker.join()
    assert len(seen) == 21
    for rc, code, word, text in seen:
        assert rc == code and word in text and b"collision_groups" in text, (rc, code, word, text)
