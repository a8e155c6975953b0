"""CPU: the host side of the beam finishing pass -- the lcrec_finish_beam entry (declared, exported, bound; its argument checks
return before any launch; its workspace query), the flags of generate, the numpy statement of the rule (tests/beam_finish_ref.py) on
every row of the case table against the consequences include/lcrec.h states, and what the rule does on the trained F6 model."""
import ctypes
import os
import re
import subprocess
import threading
import types

import numpy as np
import pytest

import beam_finish_cases as bfc
from audit_ref import audit_ref
from beam_finish_ref import clamp, colliding_items, finish_beam_ref
from finish_ref import finish_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_entries():
    import lcrec_amd
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lcrec.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lcrec_[a-z_0-9]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", lcrec_amd._lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (lcrec_[a-z_0-9]+)", out))
    lib = lcrec_amd._lib.load()                                                       # (loads without a device)
    for name in ("lcrec_finish_beam", "lcrec_finish_beam_workspace"):
        assert name in declared and name in exported and name in lcrec_amd._lib.EXPORTS and hasattr(lib, name)
    assert len(lib.lcrec_finish_beam.argtypes) == 17 and lib.lcrec_finish_beam.argtypes[11] is ctypes.c_int
    assert lib.lcrec_finish_beam_workspace.restype is ctypes.c_size_t and len(lib.lcrec_finish_beam_workspace.argtypes) == 4
    assert callable(lcrec_amd.ops.finish_beam) and callable(__import__("lcrec_amd.generate_indices", fromlist=["x"]).beam_finish_collisions)
    assert re.search(r"#define LCREC_ABI_VERSION 3\b", open(os.path.join(ROOT, "include", "lcrec.h")).read())


def test_entry_reports_argument_errors_before_any_launch():
    """Each refusal names its argument and comes back before anything is enqueued, so no device is needed.  (In a thread of its own:
    the library's last-error text is per thread, and other tests expect this thread's to be empty.)"""
    import lcrec_amd
    lib = lcrec_amd._lib.load()
    seen, sizes = [], []

    def calls():
        buf = (ctypes.c_double * 64)()
        p = ctypes.c_void_p((ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15)
        off2, off4 = (ctypes.c_void_p(p.value + o) for o in (2, 4))
        ints = lambda *v: (ctypes.c_int * len(v))(*v)
        f = lib.lcrec_finish_beam

        def call(rc, word, idx=p, n=8, L=3, K=ints(48, 100, 7), mem=p, off=p, G=2, M=4, eh=p, cand=p, ce=p, W=4, choice=p, cnt=p, ws=p,
                 ws_bytes=1 << 40):
            seen.append((f(idx, n, L, K, mem, off, G, M, eh, cand, ce, W, choice, cnt, ws, ws_bytes, None), rc, word,
                         lib.lcrec_last_error()))

        for W in (0, 3, 6, 16, -1):
            call(-1, b"width=%d" % W, W=W)
        call(-1, b"L=0", L=0)
        call(-1, b"L=17", L=17)
        call(-1, b"n=-1", n=-1)
        call(-1, b"n=4294967296", n=1 << 32)
        call(-1, b"n_members=-1", M=-1)
        call(-1, b"n_tuple_groups=-1", G=-1)
        call(-1, b"K is NULL", K=None)
        call(-1, b"counters_out is NULL", cnt=None)
        call(-1, b"K[1]=0", K=ints(48, 0, 7))
        call(-1, b"K[2]=-5", K=ints(48, 100, -5))
        words = {"idx": "idx", "mem": "tuple_members", "off": "tuple_offsets", "eh": "err_held", "cand": "cand", "ce": "cand_err",
                 "choice": "choice_out"}
        for name, word in words.items():
            call(-1, (word + " is NULL").encode(), **{name: None})
        for name in ("idx", "mem", "off", "cand", "cnt", "ws"):
            call(-1, b"must be 8-byte aligned", **{name: off4})
        for name in ("eh", "ce", "choice"):
            call(-1, b"must be 4-byte aligned", **{name: off2})
        call(-2, b"tuples need 130 bits", K=ints(*([1 << 10] * 13)), L=13)
        need = lib.lcrec_finish_beam_workspace(8, 4, 3, 4)
        call(-3, b"workspace of %d bytes, %d needed" % (need - 1, need), ws_bytes=need - 1)
        call(-3, b"workspace of 0 bytes, %d needed" % need, ws=None)
        q = lib.lcrec_finish_beam_workspace
        sizes.extend([need, q(1000, 300, 3, 8), q(0, 0, 1, 1), q(8, 4, 0, 4), q(8, 4, 17, 4), q(8, 4, 3, 3), q(-1, 4, 3, 4),
                      q(8, -1, 3, 4), q(1 << 32, 4, 3, 4)])

    worker = threading.Thread(target=calls)
    worker.start()
    worker.join()
    assert len(seen) == 34
    for rc, want, word, text in seen:
        assert rc == want and word in text and b"finish_beam" in text, (rc, want, word, text)
    # six arrays of n and six of M * W 8-byte words, M * W bytes, M ints, each rounded up to 256 bytes, and the sorts' scratch behind
    up = lambda v: (v + 255) // 256 * 256
    assert sizes[0] > 6 * up(8 * 8) + 6 * up(16 * 8) + up(16) + up(16) and sizes[0] % 256 == 0
    assert sizes[1] > 6 * up(8000) + 6 * up(2400 * 8) + up(2400) + up(1200) and sizes[2] > 0
    assert sizes[3:] == [0] * 6                                                       # refused arguments


def test_generate_takes_the_flags_and_refuses_them_where_they_cannot_run(tmp_path):
    from lcrec_amd import generate_indices as gen
    base = ["--ckpt_path", "c.pth", "--output_dir", "out"]
    a = gen.parse_args(base)
    assert (a.finish, a.finish_width, a.rounds) == ("none", 8, 20) and gen.MAX_ROUNDS == 20 and "beam" in gen.FINISH_MODES
    a = gen.parse_args(base + ["--finish", "beam", "--finish_width", "4", "--rounds", "0", "--beam", "2", "--spill"])
    assert (a.finish, a.finish_width, a.rounds, a.beam, a.spill) == ("beam", 4, 0, 2, True)
    for bad in (["--finish_width", "1"], ["--finish_width", "3"], ["--finish", "beams"], ["--rounds", "x"]):
        with pytest.raises(SystemExit):
            gen.parse_args(base + bad)
    no, out = str(tmp_path / "no.pth"), str(tmp_path / "out.json")
    # refused before the checkpoint is even opened (none of these files exist)
    with pytest.raises(ValueError, match="--finish beam with --extend"):
        gen.generate(no, out, device="cpu", finish="beam", extend=str(tmp_path / "base.json"))
    with pytest.raises(ValueError, match="--finish beam with --recheck_neartie"):
        gen.generate(no, out, device="cpu", finish="beam", recheck=True)
    ctx = types.SimpleNamespace(enabled=True, rank=0, world_size=2)
    with pytest.raises(ValueError, match="--finish beam under torchrun"):
        gen.generate(no, out, device="cpu", ctx=ctx, finish="beam")
    with pytest.raises(ValueError, match="--finish_width 3"):
        gen.generate(no, out, device="cpu", finish="beam", finish_width=3)
    with pytest.raises(ValueError, match="--rounds -1"):
        gen.generate(no, out, device="cpu", rounds=-1)
    for kw in ({"finish": "beam"}, {"finish": "beam", "spill": True, "rounds": 0, "finish_width": 2, "beam": 4, "audit": True},
               {"rounds": 3}):
        with pytest.raises(FileNotFoundError):
            gen.generate(no, out, device="cpu", **kw)
    assert not os.path.exists(out)


# ---- the rule alone, on every row of the case table ------------------------------------------------------------------------------
@pytest.mark.parametrize("row", bfc.rows())
def test_rule_has_the_consequences_the_header_states(oracle, row):
    c = bfc.case(row)
    idx, choice, counters = bfc.reference(row)
    movers, moved, unresolved, rounds = counters
    ks, W, n = c["ks"], c["W"], len(c["idx"])
    members = c["members"]
    print(row, "n", n, "members", len(members), "groups", len(c["offsets"]) - 1, "counters", counters)
    assert movers == moved + unresolved and rounds <= W and (rounds > 0) == (moved > 0)
    assert moved == int((choice >= 0).sum()) and unresolved == int((choice == -2).sum()) and (choice < W).all()
    part = (members >= 0) & (members < n)
    assert (choice[~part] == -1).all()
    moved_items = members[choice >= 0]
    # rows of non-movers are bit-identical
    same = np.ones(n, dtype=bool)
    same[moved_items] = False
    assert np.array_equal(idx[same], c["idx"][same]) and len(set(moved_items.tolist())) == moved
    # a moved item holds its chosen candidate, a live one, and no other item holds that tuple
    for j in np.flatnonzero(choice >= 0):
        t = c["cand"][j, choice[j]]
        assert np.array_equal(idx[members[j]], t) and (t >= 0).all() and (t < np.asarray(ks)).all()
    rows_after = [tuple(r) for r in clamp(idx, ks).tolist()]
    count = {}
    for t in rows_after:
        count[t] = count.get(t, 0) + 1
    assert all(count[rows_after[i]] == 1 for i in moved_items.tolist())
    # and it is a tuple nobody held before
    before = {tuple(r) for r in clamp(c["idx"], ks).tolist()}
    assert all(rows_after[i] not in before for i in moved_items.tolist())
    if bfc.true_groups(row):
        assert colliding_items(c["idx"], ks) == movers and colliding_items(idx, ks) == unresolved
    # every group keeps exactly one member in place, the one with the smallest error (a NaN as +inf), the lowest id on a tie
    for g in range(len(c["offsets"]) - 1):
        js = [j for j in range(c["offsets"][g], c["offsets"][g + 1]) if part[j]]
        if len(js) < 2:
            continue
        keep = [j for j in js if choice[j] == -1]
        assert len(keep) == 1
        err = np.where(np.isnan(c["err_held"][js]), np.inf, c["err_held"][js])
        assert err[js.index(keep[0])] == err.min() and members[keep[0]] == min(members[j] for j, v in zip(js, err) if v == err.min())
    if W == 1:
        assert set(choice.tolist()) <= {-2, -1, 0}
    # a function of the inputs alone
    again = finish_beam_ref(c["idx"], ks, members, c["offsets"], c["err_held"], c["cand"], c["cand_err"])
    assert np.array_equal(again[0], idx) and np.array_equal(again[1], choice) and tuple(again[2]) == counters


def test_rows_cover_what_they_are_there_for(oracle):
    ref = {row: bfc.reference(row)[2] for row in bfc.rows()}
    assert ref["q-nogroup-W8"] == (0, 0, 0, 0) and len(bfc.case("q-nogroup-W8")["members"]) == 0
    assert ref["s-n1"] == (0, 0, 0, 0)
    c = bfc.case("q-2-W8")                                                            # two tuples, 65 items: nobody can move
    assert ref["q-2-W8"] == (63, 0, 63, 0) and np.array_equal(bfc.reference("q-2-W8")[0], c["idx"])
    assert ref["q-3_5_2-W8"][2] > 10 * ref["q-3_5_2-W8"][1]                           # nearly everything unresolved
    assert ref["q-repeat10-W8"][3] == 8 and ref["q-repeat10-W8"][0] == 360             # every round is used
    for row in ("q-48_100_7-W2", "q-48_100_7-W4", "q-48_100_7-W8", "q-8_8_8-W8", "q-deep-W8", "s-wide-hi", "s-wide-lo", "s-wide-both",
                "s-dead", "s-own", "s-nan", "s-foreign", "s-n255", "s-n256", "s-n257", "s-w1", "s-large"):
        assert ref[row][1] > 0 and ref[row][0] > 0, row
    assert ref["q-48_100_7-W2"][1] <= ref["q-48_100_7-W4"][1] <= ref["q-48_100_7-W8"][1]
    for row in ("s-wide-hi", "s-wide-lo", "s-wide-both"):
        assert sum(int(k - 1).bit_length() for k in bfc.case(row)["ks"]) == 80
    # dead candidates lie before live ones that are taken
    c, (_, choice, _) = bfc.case("s-dead"), bfc.reference("s-dead")
    dead = ((c["cand"] < 0) | (c["cand"] >= np.asarray(c["ks"]))).any(2)
    assert any(dead[j, :choice[j]].any() for j in np.flatnonzero(choice > 0))
    # a NaN never keeps a tuple against a finite error and never wins a candidate against one
    c, (_, choice, _) = bfc.case("s-nan"), bfc.reference("s-nan")
    for g in range(len(c["offsets"]) - 1):
        js = np.arange(c["offsets"][g], c["offsets"][g + 1])
        if np.isfinite(c["err_held"][js]).any():
            assert np.isfinite(c["err_held"][js[choice[js] == -1]]).all()
    # members that are no items take no part, and their groups still have a keeper
    c, (_, choice, _) = bfc.case("s-foreign"), bfc.reference("s-foreign")
    out = (c["members"] < 0) | (c["members"] >= len(c["idx"]))
    assert out.sum() >= 4 and (choice[out] == -1).all()
    assert len(bfc.case("s-large")["members"]) * 8 > 1 << 15                          # past one block of any sort


def test_rounds_are_synchronous(oracle):
    idx, choice, counters = bfc.reference("s-sync")
    assert [tuple(r) for r in idx.tolist()] == bfc.SYNC_WANT["idx"]
    assert choice.tolist() == bfc.SYNC_WANT["choice"] and list(counters) == bfc.SYNC_WANT["counters"]


def test_capture_pair_shares_the_host_side_arguments(oracle):
    a, b = bfc.capture_pair()
    for k in ("ks", "W"):
        assert a[k] == b[k]
    for k in ("idx", "members", "offsets", "err_held", "cand", "cand_err"):
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype
    ra = finish_beam_ref(a["idx"], a["ks"], a["members"], a["offsets"], a["err_held"], a["cand"], a["cand_err"])
    rb = finish_beam_ref(b["idx"], b["ks"], b["members"], b["offsets"], b["err_held"], b["cand"], b["cand_err"])
    assert not np.array_equal(ra[1], rb[1]) and not np.array_equal(ra[0], rb[0]) and ra[2][1] > 0 and rb[2][1] > 0


# ---- the trained F6 model ----------------------------------------------------------------------------------------------------------
def test_f6_behind_the_references_own_rounds_nothing_is_left(oracle):
    z, cbs, greedy, held = bfc.f6_model()
    c = bfc.from_quantiser(z, cbs, held, 8)
    idx, choice, counters = finish_beam_ref(c["idx"], c["ks"], c["members"], c["offsets"], c["err_held"], c["cand"], c["cand_err"])
    print("F6 behind the rounds, W = 8:", counters)
    assert counters[0] == 69 and counters[2] == 0 and colliding_items(idx, c["ks"]) == 0


def test_f6_from_the_greedy_tuples_the_flow_separates_everything_for_less(oracle):
    z, cbs, greedy, _ = bfc.f6_model()
    L = len(cbs)
    flow = bfc.f6_flow(8)
    ks = flow["case"]["ks"]
    err = lambda idx: float(audit_ref(z, cbs, idx)["err"].astype(np.float64).sum())
    alone, _, unresolved = finish_ref(greedy, bfc.prefix_resid(z, cbs, greedy, L - 1), cbs[-1])
    e_greedy, e_beam, e_flow, e_alone = err(greedy), err(flow["idx_beam"]), err(flow["idx_final"]), err(alone)
    print("F6 from greedy, W = 8:", flow["counters"], "then nearest_free (moved, unresolved)", flow["finish"],
          "error sums: greedy", e_greedy, "beam step", e_beam, "flow", e_flow, "nearest_free alone", e_alone)
    assert colliding_items(greedy, ks) == flow["counters"][0] > 0
    assert colliding_items(flow["idx_beam"], ks) == flow["counters"][2]
    assert colliding_items(flow["idx_final"], ks) == 0 and flow["finish"][1] == 0
    assert unresolved == 0 and colliding_items(alone, ks) == 0
    assert e_flow < e_alone
