"""CPU: the host side of the frozen-aware beam finishing pass -- the lcrec_extend_finish_beam entry (declared, exported, bound; its
argument checks return before any launch; its workspace query is lcrec_finish_beam's), the flag of generate and its refusals, the
numpy statement of the rule (tests/extend_beam_ref.py) on every row of the case table against the consequences include/lcrec.h
states, and what the flow does on the F6 split of tests/extend_cases.py."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import beam_finish_cases as bfc
import extend_beam_cases as xbc
import extend_cases as ec
from beam_finish_ref import clamp, colliding_items
from extend_beam_ref import extend_finish_beam_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_entries():
    import lcrec_amd
    text = open(os.path.join(ROOT, "include", "lcrec.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(lcrec_[a-z_0-9]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", lcrec_amd._lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (lcrec_[a-z_0-9]+)", out))
    lib = lcrec_amd._lib.load()                                                       # (loads without a device)
    for name in ("lcrec_extend_finish_beam", "lcrec_extend_finish_beam_workspace"):
        assert name in declared and name in exported and name in lcrec_amd._lib.EXPORTS and hasattr(lib, name)
    f = lib.lcrec_extend_finish_beam
    assert len(f.argtypes) == 18 and f.argtypes[2] is ctypes.c_int64 and f.argtypes[3] is ctypes.c_int and f.argtypes[12] is ctypes.c_int
    assert len(lib.lcrec_finish_beam.argtypes) == 17                                  # the entry it extends keeps its arguments
    q = lib.lcrec_extend_finish_beam_workspace
    assert q.restype is ctypes.c_size_t and len(q.argtypes) == 4
    gen = __import__("lcrec_amd.generate_indices", fromlist=["x"])
    assert callable(lcrec_amd.ops.extend_finish_beam) and callable(gen.extend_beam_collisions)
    assert re.search(r"#define LCREC_ABI_VERSION 3\b", text)


def test_entry_reports_argument_errors_before_any_launch():
    """Each refusal names its argument and the entry and comes back before anything is enqueued, so no device is needed; and the
    workspace query is lcrec_finish_beam_workspace's, refused arguments (0) included."""
    import lcrec_amd
    lib = lcrec_amd._lib.load()
    seen, sizes = [], []

    def calls():
        buf = (ctypes.c_double * 64)()
        p = ctypes.c_void_p((ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15)
        off2, off4 = (ctypes.c_void_p(p.value + o) for o in (2, 4))
        ints = lambda *v: (ctypes.c_int * len(v))(*v)
        f = lib.lcrec_extend_finish_beam

        def call(rc, word, idx=p, n=8, nf=3, L=3, K=ints(48, 100, 7), mem=p, off=p, G=2, M=4, eh=p, cand=p, ce=p, W=4, choice=p, cnt=p,
                 ws=p, ws_bytes=1 << 40):
            seen.append((f(idx, n, nf, L, K, mem, off, G, M, eh, cand, ce, W, choice, cnt, ws, ws_bytes, None), rc, word,
                         lib.lcrec_last_error()))

        call(-1, b"n_frozen=-1", nf=-1)
        call(-1, b"n_frozen=9 (0 .. n=8)", nf=9)
        call(-1, b"n_frozen=3 (0 .. n=0)", n=0)
        call(-1, b"n_frozen=1099511627776", nf=1 << 40)
        for W in (0, 3, 6, 16, -1):
            call(-1, b"width=%d" % W, W=W)
            call(-1, b"width=%d" % W, W=W, nf=8)                                      # n_frozen == n asks for no less
        call(-1, b"L=0", L=0)
        call(-1, b"L=17", L=17)
        call(-1, b"n=-1", n=-1)
        call(-1, b"n=4294967296", n=1 << 32)
        call(-1, b"n_members=-1", M=-1)
        call(-1, b"n_tuple_groups=-1", G=-1)
        call(-1, b"K is NULL", K=None)
        call(-1, b"counters_out is NULL", cnt=None)
        call(-1, b"counters_out is NULL", cnt=None, nf=8)
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
        need = lib.lcrec_extend_finish_beam_workspace(8, 4, 3, 4)
        call(-3, b"workspace of %d bytes, %d needed (lcrec_extend_finish_beam_workspace)" % (need - 1, need), ws_bytes=need - 1)
        call(-3, b"workspace of 0 bytes, %d needed" % need, ws=None)
        for shape in ((8, 4, 3, 4), (1000, 300, 3, 8), (0, 0, 1, 1), (20000, 12000, 3, 8), (300, 200, 16, 2), (8, 4, 0, 4), (8, 4, 17, 4),
                      (8, 4, 3, 3), (-1, 4, 3, 4), (8, -1, 3, 4), (1 << 32, 4, 3, 4)):
            sizes.append((lib.lcrec_extend_finish_beam_workspace(*shape), lib.lcrec_finish_beam_workspace(*shape)))

    ec.in_thread(calls)
    assert len(seen) == 44
    for rc, want, word, text in seen:
        assert rc == want and word in text and b"extend_finish_beam:" in text, (rc, want, word, text)
    assert all(mine == theirs for mine, theirs in sizes) and all(mine > 0 for mine, _ in sizes[:5])
    assert [mine for mine, _ in sizes[5:]] == [0] * 6                                 # refused arguments


def test_generate_takes_the_flag_and_refuses_it_where_it_cannot_run(tmp_path):
    from lcrec_amd import generate_indices as gen
    base = ["--ckpt_path", "c.pth", "--output_dir", "out"]
    a = gen.parse_args(base)
    assert a.extend_finish == "nearest_free" and gen.EXTEND_FINISH_MODES == ("nearest_free", "beam")
    a = gen.parse_args(base + ["--extend", "b.json", "--extend_finish", "beam", "--finish_width", "4", "--spill", "--audit"])
    assert (a.extend, a.extend_finish, a.finish_width, a.spill, a.audit) == ("b.json", "beam", 4, True, True)
    for bad in (["--extend_finish", "beams"], ["--extend_finish", "none"], ["--extend_finish"]):
        with pytest.raises(SystemExit):
            gen.parse_args(base + bad)
    no, out, b = str(tmp_path / "no.pth"), str(tmp_path / "out.json"), str(tmp_path / "base.json")
    # refused before the checkpoint is even opened (none of these files exist)
    with pytest.raises(ValueError, match="--extend_finish beam .*give --extend"):
        gen.generate(no, out, device="cpu", extend_finish="beam")
    with pytest.raises(ValueError, match="extend_finish='beams'"):
        gen.generate(no, out, device="cpu", extend=b, extend_finish="beams")
    with pytest.raises(ValueError, match="--finish_width 3"):
        gen.generate(no, out, device="cpu", extend=b, extend_finish="beam", finish_width=3)
    with pytest.raises(ValueError, match="--finish beam with --extend is not supported.*--extend_finish beam"):
        gen.generate(no, out, device="cpu", finish="beam", extend=b)
    with pytest.raises(ValueError, match="--beam with --extend"):
        gen.generate(no, out, device="cpu", beam=4, extend=b, extend_finish="beam")
    with pytest.raises(ValueError, match="--extend with --recheck_neartie"):
        gen.generate(no, out, device="cpu", extend=b, extend_finish="beam", recheck=True)
    ctx = types.SimpleNamespace(enabled=True, rank=0, world_size=2)
    with pytest.raises(ValueError, match="--extend under torchrun"):
        gen.generate(no, out, device="cpu", ctx=ctx, extend=b, extend_finish="beam")
    with pytest.raises(ValueError, match="extend_finish='x'"):
        gen.generate_extended(no, out, b, device="cpu", extend_finish="x")
    for kw in ({"extend_finish": "beam"}, {"extend_finish": "beam", "finish_width": 2, "spill": True, "audit": True}, {}):
        with pytest.raises(FileNotFoundError):
            gen.generate(no, out, device="cpu", extend=b, **kw)
    assert not os.path.exists(out)


# ---- the rule alone, on every row of the case table ------------------------------------------------------------------------------
@pytest.mark.parametrize("row", xbc.rows())
def test_rule_has_the_consequences_the_header_states(oracle, row):
    c = xbc.case(row)
    idx, choice, counters = xbc.reference(row)
    movers, moved, unresolved, rounds = counters
    ks, W, n, nf = c["ks"], c["W"], len(c["idx"]), c["n_frozen"]
    members = c["members"]
    print(row, "n", n, "n_frozen", nf, "members", len(members), "groups", len(c["offsets"]) - 1, "counters", counters)
    assert movers == moved + unresolved and rounds <= W and (rounds > 0) == (moved > 0)
    assert moved == int((choice >= 0).sum()) and unresolved == int((choice == -2).sum()) and (choice < W).all()
    new = (members >= nf) & (members < n)
    assert (choice[~new] == -1).all()                                                 # frozen and foreign members take no part
    moved_items = members[choice >= 0]
    # rows below n_frozen, and the rows of non-movers, are bit-identical
    assert np.array_equal(idx[:nf], c["idx"][:nf])
    same = np.ones(n, dtype=bool)
    same[moved_items] = False
    assert np.array_equal(idx[same], c["idx"][same]) and len(set(moved_items.tolist())) == moved
    # a moved item holds its chosen candidate, a live one, that nobody held before and no other item holds now
    for j in np.flatnonzero(choice >= 0):
        t = c["cand"][j, choice[j]]
        assert np.array_equal(idx[members[j]], t) and (t >= 0).all() and (t < np.asarray(ks)).all()
    rows_after = [tuple(r) for r in clamp(idx, ks).tolist()]
    count = {}
    for t in rows_after:
        count[t] = count.get(t, 0) + 1
    before = {tuple(r) for r in clamp(c["idx"], ks).tolist()}
    assert all(count[rows_after[i]] == 1 and rows_after[i] not in before for i in moved_items.tolist())
    if xbc.true_groups(row):
        among_frozen = colliding_items(c["idx"][:nf], ks)
        assert colliding_items(c["idx"], ks) == among_frozen + movers and colliding_items(idx, ks) == among_frozen + unresolved
    # per group: a frozen holder leaves no keeper among the new ones; otherwise exactly one new holder stays, the one with the
    # smallest error (a NaN as +inf), the lowest id on a tie; no new holder, no mover
    for g in range(len(c["offsets"]) - 1):
        js = [j for j in range(c["offsets"][g], c["offsets"][g + 1]) if 0 <= members[j] < n]
        fresh = [j for j in js if members[j] >= nf]
        if len(js) < 2 or not fresh:
            assert all(choice[j] == -1 for j in js)
            continue
        keep = [j for j in fresh if choice[j] == -1]
        if len(fresh) < len(js):
            assert not keep
            continue
        assert len(keep) == 1
        err = np.where(np.isnan(c["err_held"][fresh]), np.inf, c["err_held"][fresh])
        assert err[fresh.index(keep[0])] == err.min() and members[keep[0]] == min(members[j] for j, v in zip(fresh, err) if v == err.min())
    # what must never be read is not: the poisoned row gives the clean row's result
    p_idx, p_choice, p_counters = xbc.run_rule(xbc.poisoned(row))
    assert np.array_equal(p_idx, idx) and np.array_equal(p_choice, choice) and p_counters == counters


@pytest.mark.parametrize("row", [r for r in bfc.rows() if r != "s-large"])
def test_without_frozen_items_the_rule_is_finish_beams(oracle, row):
    c = bfc.case(row)
    idx, choice, counters = extend_finish_beam_ref(c["idx"], 0, c["ks"], c["members"], c["offsets"], c["err_held"], c["cand"], c["cand_err"])
    want = bfc.reference(row)
    assert np.array_equal(idx, want[0]) and np.array_equal(choice, want[1]) and tuple(counters) == want[2]


def test_rows_written_by_hand_give_what_they_were_written_for(oracle):
    for row, (_, (idx, choice, counters)) in xbc.HAND.items():
        got = xbc.reference(row)
        assert [tuple(r) for r in got[0].tolist()] == [tuple(t) for t in idx], row
        assert got[1].tolist() == list(choice) and list(got[2]) == list(counters), row
    # the new holder's error IS the smaller one, and the frozen holder keeps the tuple all the same
    c = xbc.case("h-frozen-keeps")
    assert c["err_held"][1] < c["err_held"][0] and c["n_frozen"] == 1
    c = xbc.case("h-sync-f0")
    assert c["err_held"][0] > c["err_held"][1:].max() and xbc.reference("h-sync-f0")[1].tolist() == [-1, 0, 2, 0]
    c = xbc.case("h-last-new")
    assert c["members"][-1] >= c["n_frozen"] > c["members"][-2]
    c = xbc.case("h-cand0-frozen")
    assert tuple(c["cand"][1, 0]) == tuple(c["idx"][0]) and 0 not in c["members"]


def test_rows_cover_what_they_are_there_for(oracle):
    ref = {row: xbc.reference(row)[2] for row in xbc.rows()}
    nf = {row: xbc.case(row)["n_frozen"] for row in xbc.rows()}
    n = {row: len(xbc.case(row)["idx"]) for row in xbc.rows()}
    assert nf["s-dead-nf0"] == 0 and nf["s-dead-nfn"] == n["s-dead-nfn"] and nf["s-dead-nfn1"] == n["s-dead-nfn1"] - 1
    assert ref["s-dead-nf0"] == bfc.reference("s-dead")[2] and ref["s-dead-nfn"] == (0, 0, 0, 0)
    assert ref["s-n1-nf0"] == (0, 0, 0, 0) and ref["s-n1-nfn"] == (0, 0, 0, 0) and ref["h-new-alone"] == (0, 0, 0, 0)
    for row in ("q-48_100_7-W2-f1", "q-48_100_7-W4-f1", "q-48_100_7-W8-f1", "q-48_100_7-W8-f2", "q-8_8_8-W8-f1", "q-8_8_8-W8-f2",
                "q-deep-W8-f1", "q-repeat10-W8-f2", "s-wide-hi-f1", "s-wide-hi-f2", "s-wide-lo-f1", "s-wide-both-f2", "s-dead-f1",
                "s-dead-f2", "s-own-f1", "s-nan-f1", "s-nan-f2", "s-foreign-f1", "s-foreign-f2", "s-n255-f1", "s-n256-f1", "s-n256-f2",
                "s-n257-f2", "s-w1-f1", "s-large-f1"):
        assert ref[row][1] > 0 and 0 < nf[row] < n[row], row
        c = xbc.case(row)
        held = (c["members"] >= 0) & (c["members"] < nf[row])
        assert held.any() and not held.all(), row                                     # frozen and new members side by side
    assert ref["q-48_100_7-W2-f1"][1] <= ref["q-48_100_7-W4-f1"][1] <= ref["q-48_100_7-W8-f1"][1]
    assert {xbc.case(r)["W"] for r in xbc.rows()} == {1, 2, 4, 8}
    for row in ("s-wide-hi-f1", "s-wide-lo-f1", "s-wide-both-f2"):
        assert sum(int(k - 1).bit_length() for k in xbc.case(row)["ks"]) == 80
    assert len(xbc.case("s-large-f1")["members"]) * 8 > 1 << 15                       # past one block of any sort
    # some group has a frozen holder and two or more new ones (all of them move), some has new holders only (one stays)
    c, (_, choice, _) = xbc.case("q-48_100_7-W8-f1"), xbc.reference("q-48_100_7-W8-f1")
    kinds = set()
    for g in range(len(c["offsets"]) - 1):
        m = c["members"][c["offsets"][g]:c["offsets"][g + 1]]
        kinds.add((int((m < c["n_frozen"]).sum()) > 0, int((m >= c["n_frozen"]).sum()) > 1))
    assert kinds >= {(True, True), (False, True), (True, False)}
    # the poison would bite if it were read: with the frozen items taken for new ones the poisoned row gives another result
    p = xbc.poisoned("q-48_100_7-W8-f1")
    wrong = extend_finish_beam_ref(p["idx"], 0, p["ks"], p["members"], p["offsets"], p["err_held"], p["cand"], p["cand_err"])
    assert not np.array_equal(wrong[0], xbc.reference("q-48_100_7-W8-f1")[0])
    assert not np.array_equal(wrong[0][:p["n_frozen"]], p["idx"][:p["n_frozen"]])


def test_capture_pair_shares_the_host_side_arguments(oracle):
    a, b = xbc.capture_pair()
    for k in ("ks", "W", "n_frozen"):
        assert a[k] == b[k]
    for k in ("idx", "members", "offsets", "err_held", "cand", "cand_err"):
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype
    ra, rb = xbc.run_rule(a), xbc.run_rule(b)
    assert not np.array_equal(ra[1], rb[1]) and not np.array_equal(ra[0], rb[0]) and ra[2][1] > 0 and rb[2][1] > 0
    assert 0 < a["n_frozen"] < len(a["idx"]) and np.isnan(b["err_held"]).any()


# ---- the trained F6 model, 2 000 frozen items and 1 000 new ones ---------------------------------------------------------------------
def test_f6_the_flow_places_the_new_items_for_less_than_nearest_free_alone(oracle):
    flow = xbc.f6_flow(2000, "finished", 8)
    ks, n0 = flow["case"]["ks"], 2000
    e = flow["err"]
    print("F6 2000 + 1000, W = 8:", flow["counters"], "then extend_ref (moved, unresolved)", flow["extend"], "error sums of the new items:",
          e, "ratios: flow", e["flow"] / e["greedy"], "extend_ref alone", e["alone"] / e["greedy"])
    assert colliding_items(flow["union"][:n0], ks) == 0 and colliding_items(flow["union"], ks) == 462
    assert tuple(flow["counters"]) == (462, 448, 14, 4)
    assert colliding_items(flow["idx_beam"], ks) == 14
    assert flow["extend"] == (14, 0) and colliding_items(flow["idx_final"], ks) == 0
    assert flow["alone_extend"] == (462, 0) and colliding_items(flow["alone"], ks) == 0
    assert np.array_equal(flow["idx_final"][:n0], flow["union"][:n0]) and np.array_equal(flow["idx_beam"][:n0], flow["union"][:n0])
    assert e["flow"] / e["greedy"] < e["alone"] / e["greedy"]
    assert e["flow"] / e["greedy"] == pytest.approx(0.9860, abs=5e-4) and e["alone"] / e["greedy"] == pytest.approx(1.1816, abs=5e-4)


def test_f6_a_colliding_base_stays_exactly_as_it_is(oracle):
    flow = xbc.f6_flow(2000, "reference", 8)
    ks, n0 = flow["case"]["ks"], 2000
    among = colliding_items(flow["union"][:n0], ks)
    print("F6 reference base:", flow["counters"], flow["extend"], "colliding among the frozen", among)
    assert among == 39 and flow["counters"][0] == 440 and flow["counters"][1] == 435 and flow["extend"] == (5, 0)
    assert np.array_equal(flow["idx_final"][:n0], flow["union"][:n0]) and colliding_items(flow["idx_final"], ks) == among
