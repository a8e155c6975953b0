"""CPU: the host side of --extend -- the lcrec_extend_nearest_free and lcrec_index_json_parse entries (declared, exported, bound;
argument checks return before any launch), the CLI flag, the numpy statement of the rule (tests/extend_ref.py) against
finish_ref and on the F6 fixture split into a frozen base and new items, and the reader of `.index.json`.
Every comparison is of integers; there is no tolerance in this file."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import extend_cases as ec
import finish_cases as fc
import golden_inputs as gi
from extend_ref import extend_ref
from finish_ref import colliding_items, finish_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lcrec_extend_nearest_free", "lcrec_index_json_parse")


def test_header_declares_and_library_exports_both_entries():
    import lcrec_amd
    header = open(os.path.join(ROOT, "include", "lcrec.h")).read()
    assert "#define LCREC_ABI_VERSION 3" in header
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(lcrec_[a-z_0-9]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", lcrec_amd._lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (lcrec_[a-z_0-9]+)", out))
    lib = lcrec_amd._lib.load()
    for name in NEW:
        assert name in declared and name in exported and name in lcrec_amd._lib.EXPORTS and hasattr(lib, name)
    assert lib.lcrec_version() == 3 == lcrec_amd._lib.ABI_VERSION
    assert callable(lcrec_amd.ops.extend_nearest_free) and callable(lcrec_amd.ops.index_json_parse)


def test_extend_entry_reports_argument_errors_before_any_launch():
    """Each refusal names what it is about and comes back before anything is enqueued, so no device is needed."""
    import lcrec_amd
    lib = lcrec_amd._lib.load()
    seen = []

    def calls():
        buf = (ctypes.c_double * 64)()
        base = ctypes.cast(buf, ctypes.c_void_p).value
        p = ctypes.c_void_p((base + 15) & ~15)                       # 16-byte aligned
        off4, off8 = ctypes.c_void_p(p.value + 4), ctypes.c_void_p(p.value + 8)
        ints = lambda *v: (ctypes.c_int * len(v))(*v)
        f = lib.lcrec_extend_nearest_free

        def call(rc, word, idx=p, n=8, nf=2, L=3, K=ints(48, 48, 48), resid=p, e=16, cb=p, mem=p, off=p, nb=1, counters=p):
            seen.append((f(idx, n, nf, L, K, resid, e, cb, mem, off, nb, counters, None), rc, word, lib.lcrec_last_error()))

        call(-1, b"n_frozen=-1", nf=-1)
        call(-1, b"n_frozen=9 (0 .. n=8)", nf=9)
        call(-1, b"resid_last, with 6 new items", resid=None)
        for e in (0, 8, 24, 128):
            call(-2, b"e_dim=%d" % e, e=e)
        call(-1, b"K[2]=0", K=ints(48, 48, 0))
        call(-2, b"level 2 (K=4096, e=64) does not fit", K=ints(48, 48, 4096), e=64)
        call(-2, b"level 0 (K=2048, e=16) does not fit", L=1, K=ints(2048))
        # the frozen-holder counts cost 4 more bytes per code: levels the finishing pass takes and this entry cannot
        call(-2, b"level 1 (K=1900, e=16) does not fit in 160 KB of LDS with the frozen-holder counts", L=2, K=ints(4, 1900))
        call(-2, b"level 1 (K=1080, e=32) does not fit in 160 KB of LDS with the frozen-holder counts", L=2, K=ints(4, 1080), e=32)
        call(-1, b"L=0", L=0)
        call(-1, b"L=17", L=17)
        call(-1, b"n=-1", n=-1, nf=0)
        call(-1, b"n_buckets=-1", nb=-1)
        call(-1, b"resid_last and codebook_last must be 16-byte aligned", resid=off8)
        call(-1, b"resid_last and codebook_last must be 16-byte aligned", cb=off4)
        call(-1, b"must be 8-byte aligned", idx=off4)
        call(-1, b"must be 8-byte aligned", mem=off4)
        call(-1, b"must be 8-byte aligned", off=off4)
        call(-1, b"counters_out is NULL", counters=None)
        call(-1, b"K is NULL", K=None)
        call(-1, b"NULL pointer", mem=None)
        call(-1, b"NULL pointer", cb=None)
        # ... and the same two levels pass the finishing pass's fit check (it goes on to refuse the NULL members)
        g = lib.lcrec_finish_nearest_free
        seen.append((g(p, 8, 2, ints(4, 1900), p, 16, p, None, p, 1, p, None), -1, b"finish_nearest_free: NULL pointer", lib.lcrec_last_error()))
        seen.append((g(p, 8, 2, ints(4, 1080), p, 32, p, None, p, 1, p, None), -1, b"finish_nearest_free: NULL pointer", lib.lcrec_last_error()))

    ec.in_thread(calls)
    assert len(seen) == 27
    for rc, want, word, text in seen:
        assert rc == want and word in text and b"nearest_free" in text, (rc, want, word, text)
    for rc, want, word, text in seen[:-2]:
        assert b"extend_nearest_free" in text


def test_cli_accepts_extend_and_generate_refuses_it_with_recheck(tmp_path):
    from lcrec_amd import generate_indices as gen
    base = ["--ckpt_path", "c.pth", "--output_dir", "out"]
    assert gen.parse_args(base).extend is None
    a = gen.parse_args(base + ["--extend", "Games.index.json", "--finish", "nearest_free"])
    assert a.extend == "Games.index.json"
    assert callable(gen.generate_extended) and callable(gen.extend_collisions) and callable(gen.load_index_json)
    # refused before the checkpoint is even opened (none of these files exist)
    with pytest.raises(ValueError, match="recheck_neartie"):
        gen.generate(str(tmp_path / "no.pth"), str(tmp_path / "out.json"), device="cpu", recheck=True, extend=str(tmp_path / "b.json"))
    import types
    ctx = types.SimpleNamespace(enabled=True, rank=0, world_size=2)
    with pytest.raises(ValueError, match="torchrun"):
        gen.generate(str(tmp_path / "no.pth"), str(tmp_path / "out.json"), device="cpu", ctx=ctx, extend=str(tmp_path / "b.json"))


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def test_without_frozen_items_the_rule_is_the_finishing_pass(oracle):
    """Tuples, the order in which movers are served, and the unresolved count."""
    idx, resid, cb, _ = fc.f6_case()
    cases = [("F6", idx, resid, cb)]
    for K, e, n in ((48, 16, 150), (1, 32, 12), (100, 64, 300)):
        cases.append(((K, e),) + fc.random_case(n, [4, K], e, seed=500 + K))
    cases.append(("L=1",) + fc.random_case(150, [100], 32, seed=501))
    for what, i, r, c in cases:
        want = finish_ref(i, r, c)
        got = extend_ref(i, 0, r, c)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2], what
        assert len(want[1]) > 0, what


@pytest.mark.parametrize("n0,movers_want", [(1500, 789), (2000, 462), (2500, 190), (2900, 24)])
def test_f6_split_into_a_frozen_base_and_new_items(oracle, n0, movers_want):
    """The largest F6 bucket is 41 items on 48 codes and buckets never change (only last codes move), so unresolved == 0 is the
    rule's invariant here: 'unresolved is 0 whenever no touched bucket has more items than K[L-1]'."""
    union, resid_new, cb = ec.f6_split(n0)
    K = cb.shape[0]
    _, sizes = np.unique(union[:, :-1], axis=0, return_counts=True)
    assert sizes.max() == 41 <= K
    assert ec.colliding_among(union, n0) == 0
    new, movers, unresolved = extend_ref(union, n0, resid_new, cb)
    print("N0", n0, "movers", len(movers), "unresolved", unresolved, "colliding after", colliding_items(new))
    assert len(movers) == movers_want and len(set(movers)) == len(movers) and min(movers) >= n0
    assert unresolved == 0
    assert np.array_equal(new[:n0], union[:n0])                                    # frozen rows: bit-identical
    assert colliding_items(new) == 0
    still = np.ones(len(union), dtype=bool)
    still[movers] = False
    assert np.array_equal(new[still], union[still])                                # every non-mover carries its pass-1 tuple
    assert np.array_equal(new[:, :-1], union[:, :-1])
    assert (new[movers, -1] != union[movers, -1]).all() and (new[:, -1] >= 0).all() and (new[:, -1] < K).all()


def test_a_colliding_base_keeps_exactly_its_own_collisions(oracle):
    """The reference's own final tuples as base: 39 of its first 2000 items collide, and nobody may touch them."""
    n0 = 2000
    union, resid_new, cb = ec.f6_split(n0, base="reference")
    before = ec.colliding_among(union, n0)
    assert before == 39
    new, movers, unresolved = extend_ref(union, n0, resid_new, cb)
    assert unresolved == 0 and np.array_equal(new[:n0], union[:n0])
    assert colliding_items(new) == before + unresolved


def test_frozen_precedence_and_untouched_buckets(oracle):
    e, K = 16, 6
    r = gi.rs(7)
    cb = gi.f32(r.standard_normal((K, e)))
    # frozen item 0 and new item 1 hold code 2; the new item sits exactly on code 2 and still has to go
    idx = np.array([[0, 2], [0, 2]], dtype=np.int64)
    new, movers, unres = extend_ref(idx, 1, cb[2:3].copy(), cb)
    assert movers == [1] and unres == 0 and new[0].tolist() == [0, 2] and new[1, 1] != 2
    # {frozen, new, new}: both new items move
    idx = np.array([[0, 2], [0, 2], [0, 2]], dtype=np.int64)
    new, movers, unres = extend_ref(idx, 1, gi.f32(r.standard_normal((2, e))), cb)
    assert movers == [1, 2] and len({2, new[1, 1], new[2, 1]}) == 3
    # two frozen items share a code, the only new item holds another alone: untouched
    idx = np.array([[0, 2], [0, 2], [0, 3]], dtype=np.int64)
    new, movers, unres = extend_ref(idx, 2, gi.f32(r.standard_normal((1, e))), cb)
    assert movers == [] and unres == 0 and np.array_equal(new, idx)
    # a touched bucket: the frozen pair on code 2 stays, the new pair on code 4 is separated, and code 2 counts as occupied
    idx = np.array([[0, 2], [0, 2], [0, 4], [0, 4]], dtype=np.int64)
    new, movers, unres = extend_ref(idx, 2, np.stack([cb[2], cb[2]]), cb)
    assert len(movers) == 1 and new[:2].tolist() == [[0, 2], [0, 2]] and 2 not in new[2:, 1].tolist()
    assert colliding_items(new) == 1
    # K codes all held by frozen items: the new holders have nowhere to go
    idx = np.array([[0, k] for k in range(K)] + [[0, 1], [0, 1]], dtype=np.int64)
    new, movers, unres = extend_ref(idx, K, gi.f32(r.standard_normal((2, e))), cb)
    assert movers == [K, K + 1] and unres == 2 and np.array_equal(new, idx)
    # members out of range take no part
    idx = np.array([[0, 2], [0, 9], [0, 2], [0, -1]], dtype=np.int64)
    new, movers, unres = extend_ref(idx, 1, gi.f32(r.standard_normal((3, e))), cb, buckets=[[-3, 0, 1, 2, 3, 4, 99]])
    assert movers == [2] and np.array_equal(new[[0, 1, 3]], idx[[0, 1, 3]])


# ---- the reader -------------------------------------------------------------------------------------------------------------------
def _text(rows):
    from lcrec_amd import generate_indices as gen
    return json.dumps({str(i): t for i, t in enumerate(gen.tokens_for(np.asarray(rows).tolist()))}).encode() if len(rows) else b"{}"


def test_strict_reader_round_trips_random_tuples():
    import lcrec_amd
    r = gi.rs(11)
    for L in range(1, 27):
        n = int(r.randint(1, 40))
        rows = r.randint(0, 10 ** int(r.randint(1, 10)), size=(n, L)).astype(np.int64)
        rows[0, 0] = 2 ** 63 - 1
        rows[-1, -1] = 0
        got = lcrec_amd.ops.index_json_parse(_text(rows), L)
        assert got.dtype == np.int64 and np.array_equal(got, rows), L
    assert lcrec_amd.ops.index_json_parse(b"{}", 3).shape == (0, 3)
    big = r.randint(0, 256, size=(70000, 4)).astype(np.int64)                      # the formatter's threaded path, and back
    text = b"{" + lcrec_amd.ops.index_json_text(big) + b"}"
    assert np.array_equal(lcrec_amd.ops.index_json_parse(text, 4), big)


def test_reader_gives_the_f6_matrix(tmp_path):
    from lcrec_amd import generate_indices as gen
    import lcrec_amd
    idx, _, _, g = fc.f6_case()
    text = bytes(g["json_text"])
    assert np.array_equal(lcrec_amd.ops.index_json_parse(text, 3), idx)
    path = tmp_path / "F6.index.json"
    path.write_bytes(text)
    assert np.array_equal(gen.load_index_json(str(path), [48, 48, 48]), idx)


def test_other_layouts_go_through_the_fallback(tmp_path):
    from lcrec_amd import generate_indices as gen
    import lcrec_amd
    r = gi.rs(12)
    rows = r.randint(0, 48, size=(37, 3)).astype(np.int64)
    doc = {str(i): t for i, t in enumerate(gen.tokens_for(rows.tolist()))}
    order = [str(i) for i in r.permutation(len(rows))]
    texts = {"shuffled": json.dumps({k: doc[k] for k in order}), "indented": json.dumps(doc, indent=2),
             "compact": json.dumps(doc, separators=(",", ":")), "newline": json.dumps(doc) + "\n"}
    for what, text in texts.items():
        path = tmp_path / (what + ".index.json")
        path.write_text(text)
        with pytest.raises(lcrec_amd.LcrecError, match="byte "):
            ec.in_thread(lcrec_amd.ops.index_json_parse, text.encode(), 3)
        assert np.array_equal(ec.in_thread(gen.load_index_json, str(path), [48, 48, 48]), rows), what


def test_malformed_files_raise_value_error_naming_item_and_level(tmp_path):
    from lcrec_amd import generate_indices as gen
    good = {"0": ["<a_1>", "<b_2>", "<c_3>"], "1": ["<a_4>", "<b_5>", "<c_6>"], "2": ["<a_7>", "<b_8>", "<c_9>"]}

    def refuse(text, match, ks=(48, 48, 48)):
        path = tmp_path / "bad.index.json"
        path.write_text(text if isinstance(text, str) else json.dumps(text))
        with pytest.raises(ValueError, match=match):
            ec.in_thread(gen.load_index_json, str(path), list(ks))

    refuse(dict(good, **{"1": ["<a_4>", "<b_5>"]}), "item 1: 2 tokens")                      # a wrong level count
    refuse(dict(good, **{"2": ["<a_7>", "<b_8>", "<c_9>", "<d_1>"]}), "item 2: 4 tokens")
    refuse(good, "item 0: 3 tokens, the checkpoint has 2 levels", ks=(48, 48))
    refuse(dict(good, **{"1": ["<a_4>", "<c_5>", "<c_6>"]}), "item 1, level 1")                # a wrong prefix letter
    refuse(dict(good, **{"1": ["<a_4>", "<b_-5>", "<c_6>"]}), "item 1, level 1")
    refuse(dict(good, **{"2": ["<a_7>", "<b_8>", "<c_48>"]}), "item 2, level 2: code 48 .* 48 codes")   # a code >= K_l
    refuse(good, "item 2, level 1: code 8 .* 8 codes", ks=(48, 8, 48))
    refuse({"0": good["0"], "1": good["1"], "3": good["2"]}, "no item 2 .*'3'")              # a missing key
    refuse({"0": good["0"], "01": good["1"], "2": good["2"]}, "no item 1 .*'01'")
    refuse('{"0": ["<a_1>", "<b_2>", "<c_3>"], "0": ["<a_1>", "<b_2>", "<c_4>"]}', "duplicate key '0'")
    refuse('[["<a_1>"]]', "not an index file")
    refuse('{"0": ["<a_1>", "<b_2>", "<c_3>"]', "not an index file")
    refuse(dict(good, **{"1": "tokens"}), "item 1: no tokens")
