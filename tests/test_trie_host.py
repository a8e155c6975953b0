"""CPU: the host side of the index trie -- the four lcrec_index_trie_* entries (declared, exported, bound; every argument check
returns before any launch), the numpy statement of the three rules (tests/trie_ref.py) against a brute-force dict of tuples on every
row of the case table, what the reference's per-position sets admit on F6 against what the trie admits, the query command's
refusals and its report's arithmetic."""
import argparse
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import extend_cases as ec
import trie_cases as tc
from trie_ref import (NEG_INF_BITS, allowed_ref, brute_force, build_ref, clamp, exact_only, find_ref, mask_ref, span_ref, stats_ref,
                      walk_table)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("lcrec_index_trie_build_workspace", "lcrec_index_trie_build", "lcrec_index_trie_find", "lcrec_index_trie_mask_logits")


@pytest.fixture(autouse=True, scope="module")
def trie_entries():
    """Every test here is about the index trie: without its entries in the library and its class in the package there is nothing
    for the rules below to pin."""
    import lcrec_amd
    lib = lcrec_amd._lib.load()
    assert all(hasattr(lib, name) for name in ENTRIES) and hasattr(lcrec_amd, "IndexTrie") and hasattr(lcrec_amd.ops, "trie_build")


def test_header_still_says_abi_3_and_the_library_exports_the_trie_entries():
    import lcrec_amd
    header = open(os.path.join(ROOT, "include", "lcrec.h")).read()
    assert "#define LCREC_ABI_VERSION 3" in header
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(lcrec_[a-z_0-9]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", lcrec_amd._lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (lcrec_[a-z_0-9]+)", out))
    lib = lcrec_amd._lib.load()
    assert lib.lcrec_version() == 3
    for name in ENTRIES:
        assert name in declared and name in exported and name in lcrec_amd._lib.EXPORTS and hasattr(lib, name), name
    v, i64 = ctypes.c_void_p, ctypes.c_int64
    assert lib.lcrec_index_trie_build_workspace.restype is ctypes.c_size_t and lib.lcrec_index_trie_build_workspace.argtypes == [i64, ctypes.c_int]
    assert lib.lcrec_index_trie_build.argtypes == [v, i64, i64, ctypes.c_int, v, v, v, ctypes.c_size_t, v]
    assert lib.lcrec_index_trie_find.argtypes == [v, v, i64, i64, ctypes.c_int, v, v, v]
    assert lib.lcrec_index_trie_mask_logits.argtypes == [v, v, i64, ctypes.c_int, v, ctypes.c_int, v, i64, i64, v]
    assert [f for f, _ in lcrec_amd._lib.IndexTrie._fields_] == ["n", "L", "K", "order", "counts", "child", "code", "first"]
    for name in ("trie_build", "trie_find", "trie_mask_logits_"):
        assert callable(getattr(lcrec_amd.ops, name)), name
    for name in ("from_indices", "from_file", "find", "mask_logits_", "lookup", "span", "stats", "prefix_allowed_tokens_fn"):
        assert callable(getattr(lcrec_amd.IndexTrie, name)), name
    assert "trie.hip" in open(os.path.join(ROOT, "lc-rec_amd", "csrc", "Makefile")).read()


def test_entries_report_argument_errors_before_any_launch():
    """Each refusal names its argument and comes back before anything is enqueued, so no device is needed.  (In a thread of its own:
    the library's last-error text is per thread, and other tests expect this thread's to be empty.)"""
    import lcrec_amd
    lib = lcrec_amd._lib.load()
    seen, sizes = [], []

    def calls():
        buf = (ctypes.c_double * 64)()
        base = ctypes.cast(buf, ctypes.c_void_p).value
        p = ctypes.c_void_p((base + 15) & ~15)
        off2, off4, off8 = (ctypes.c_void_p(p.value + k) for k in (2, 4, 8))
        ints = lambda *v: (ctypes.c_int * len(v))(*v)

        def record(n=8, L=3, K=(48, 100, 7), **over):
            t = lcrec_amd._lib.IndexTrie()
            t.n, t.L = n, L
            for l, k in enumerate(K):
                t.K[l] = k
            for name in ("order", "counts", "child", "code", "first"):
                setattr(t, name, over.get(name, p).value if over.get(name, p) is not None else None)
            return t

        def build(rc, word, idx=p, stride=0, n=8, L=3, K=ints(48, 100, 7), trie="fresh", ws=p, ws_bytes=1 << 40):
            t = record(0, 0, ()) if trie == "fresh" else trie
            got = lib.lcrec_index_trie_build(idx, stride, n, L, K, None if t is None else ctypes.addressof(t), ws, ws_bytes, None)
            seen.append((got, rc, word, b"trie_build", lib.lcrec_last_error()))

        def find(rc, word, trie="built", prefix=p, stride=0, B=4, depth=3, node=p, dout=p):
            t = record() if trie == "built" else trie
            got = lib.lcrec_index_trie_find(None if t is None else ctypes.addressof(t), prefix, stride, B, depth, node, dout, None)
            seen.append((got, rc, word, b"trie_find", lib.lcrec_last_error()))

        def mask(rc, word, trie="built", node=p, B=4, depth=1, tokens=p, eos=2, logits=p, ld=100, V=100):
            t = record() if trie == "built" else trie
            got = lib.lcrec_index_trie_mask_logits(None if t is None else ctypes.addressof(t), node, B, depth, tokens, eos, logits, ld, V, None)
            seen.append((got, rc, word, b"trie_mask", lib.lcrec_last_error()))

        build(-1, b"K is NULL", K=None)
        build(-1, b"L=0", L=0)
        build(-1, b"L=17", L=17, K=ints(*[4] * 17))
        build(-1, b"n=-1", n=-1)
        build(-1, b"K[1]=0", K=ints(48, 0, 7))
        build(-1, b"144 key bits (> 128)", L=16, K=ints(*[512] * 16))
        build(-1, b"idx_stride=2 < L=3", stride=2)
        build(-1, b"idx_stride=-1", stride=-1)
        build(-1, b"idx is NULL", idx=None)
        build(-1, b"idx must be 8-byte aligned", idx=off4)
        build(-1, b"trie is NULL", trie=None)
        for name in ("order", "counts", "child", "code", "first"):
            build(-1, b"trie->" + name.encode() + b" is NULL", trie=record(0, 0, (), **{name: None}))
        build(-1, b"must be 8-byte aligned", trie=record(0, 0, (), first=off4))
        build(-1, b"trie->code must be 4-byte aligned", trie=record(0, 0, (), code=off2))
        build(-1, b"workspace must be 16-byte aligned", ws=off8)
        need = lib.lcrec_index_trie_build_workspace(8, 3)
        build(-3, b"workspace of %d bytes, %d needed" % (need - 1, need), ws_bytes=need - 1)
        build(-3, b"workspace of 0 bytes, %d needed" % need, ws=None)
        sizes.extend([need, lib.lcrec_index_trie_build_workspace(0, 3), lib.lcrec_index_trie_build_workspace(-1, 3),
                      lib.lcrec_index_trie_build_workspace(8, 0), lib.lcrec_index_trie_build_workspace(8, 17)])

        find(-1, b"trie is NULL", trie=None)
        find(-1, b"L=0", trie=record(L=0), depth=0)
        find(-1, b"n=-2", trie=record(n=-2))
        find(-1, b"K[2]=0", trie=record(K=(48, 100, 0)))
        find(-1, b"trie->child is NULL", trie=record(child=None))
        find(-1, b"B=-1", B=-1)
        find(-1, b"depth=-1 outside [0, L=3]", depth=-1)
        find(-1, b"depth=4 outside [0, L=3]", depth=4)
        find(-1, b"prefix_stride=2 < depth=3", stride=2)
        find(-1, b"prefix is NULL", prefix=None)
        find(-1, b"node_out is NULL", node=None)
        find(-1, b"must be 8-byte aligned", prefix=off4)
        find(-1, b"depth_out must be 4-byte aligned", dout=off2)
        find(0, b"", B=0)
        find(0, b"", B=0, prefix=None, node=None, dout=None)

        mask(-1, b"trie is NULL", trie=None)
        mask(-1, b"L=17", trie=record(L=17))
        mask(-1, b"K[0]=-1", trie=record(K=(-1, 100, 7)))
        mask(-1, b"trie->counts is NULL", trie=record(counts=None))
        mask(-1, b"B=-1", B=-1)
        mask(-1, b"depth=-1 outside [0, L=3]", depth=-1)
        mask(-1, b"depth=4 outside [0, L=3]", depth=4)
        mask(-1, b"V=0", V=0)
        mask(-1, b"ld=99 < V=100", ld=99)
        mask(-1, b"node is NULL", node=None)
        mask(-1, b"logits is NULL", logits=None)
        mask(-1, b"node must be 8-byte aligned", node=off4)
        mask(-1, b"must be 4-byte aligned", logits=off2)
        mask(-1, b"must be 4-byte aligned", tokens=off2)
        mask(0, b"", B=0)
        mask(0, b"", B=0, node=None, logits=None, tokens=None, depth=3)

    ec.in_thread(calls)
    for rc, want, word, who, text in seen:
        assert rc == want and (rc == 0 or (word in text and who in text)), (rc, want, word, text)
    assert len(seen) == 52
    assert sizes[0] >= 11 * 256 and sizes[0] % 256 == 0 and sizes[1:] == [0, 0, 0, 0]


def test_the_binding_refuses_what_is_not_on_a_device():
    """... before the library is called: no last-error text is left in this thread."""
    import lcrec_amd
    before = lcrec_amd._lib.load().lcrec_last_error()
    with pytest.raises(lcrec_amd.LcrecError, match="HIP device"):
        lcrec_amd.ops.trie_build(torch.zeros((4, 2), dtype=torch.int64), [4, 4])
    assert lcrec_amd._lib.load().lcrec_last_error() == before


# ---- the numpy rule against a brute-force dict of tuples -----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tc.BUILD))
def test_build_rule_numbers_the_sorted_distinct_prefixes(name):
    idx, ks, _, trie = tc.build_case(name)
    n, L = len(idx), len(ks)
    nodes, holders = brute_force(idx, ks)
    c = clamp(idx, ks)
    assert trie["counts"].tolist() == [len(nodes[d]) for d in range(L + 1)] and trie["counts"][0] == 1
    assert sorted(trie["order"].tolist()) == list(range(n))
    keys = [tuple(int(v) for v in c[i]) + (int(i),) for i in trie["order"]]
    assert keys == sorted(keys)                                              # by key ascending, then id ascending
    if n == 0:
        assert [r.tolist() for r in trie["child"]] == [[0]] * L and trie["first"].tolist() == [0]
        return
    inverse = [{j: p for p, j in nodes[d].items()} for d in range(L + 1)]
    for d in range(L):
        kids = trie["child"][d]
        assert len(kids) == trie["counts"][d] + 1 and kids[-1] == trie["counts"][d + 1] and len(trie["code"][d]) == trie["counts"][d + 1]
        for j in range(int(trie["counts"][d])):
            mine = [inverse[d + 1][k] for k in range(int(kids[j]), int(kids[j + 1]))]
            want = sorted(p for p in nodes[d + 1] if p[:d] == inverse[d][j]) if n <= 5000 else None
            assert mine and all(p[:d] == inverse[d][j] for p in mine) and mine == sorted(mine)
            assert want is None or mine == want
            assert [p[-1] for p in mine] == trie["code"][d][int(kids[j]):int(kids[j + 1])].tolist()
    first = trie["first"]
    assert len(first) == trie["counts"][L] + 1 and first[-1] == n
    for j, p in inverse[L].items():
        assert trie["order"][int(first[j]):int(first[j + 1])].tolist() == holders[p]


def test_f6_counts_and_what_the_reference_admits():
    """On F6 the reference's per-position sets (data.py:67-89) admit 48 * 48 * 47 tuples; the trie admits the 2 931 the file holds."""
    idx, ks, _, trie = tc.build_case("f6")
    assert trie["counts"].tolist() == tc.F6_COUNTS == [1, 48, 521, 2931]
    st = stats_ref(trie)
    assert st["largest_leaf"] == 4 and st["nodes"] == tc.F6_COUNTS and st["max_children"][0] == 48
    per_position = [set(idx[:, l].tolist()) for l in range(3)]
    assert int(np.prod([len(s) for s in per_position])) == 48 * 48 * 47 == 108288
    table = walk_table(trie)
    admitted = 0
    stack = [(0, 0)]
    while stack:                                                             # every path the allowed sets let a generation take
        d, node = stack.pop()
        if d == 3:
            admitted += 1
            continue
        stack.extend((d + 1, table[(d, node, c)]) for c in allowed_ref(trie, node, d, None, -1))
    assert admitted == 2931 == len({tuple(r) for r in idx.tolist()})
    assert 1.0 - admitted / 108288 > 0.97


@pytest.mark.parametrize("name", tc.SMALL)
def test_find_rule_on_every_depth_and_batch(name):
    idx, ks, _, trie = tc.build_case(name)
    nodes, holders = brute_force(idx, ks)
    table = tc.table_of(name)
    L = len(ks)
    for depth in range(L + 1):
        for B in (1, 65):
            q = tc.find_queries(name, depth, B)
            got, reached = find_ref(trie, q, depth, table)
            for b in range(B):
                row = [int(v) for v in q[b]]
                want = 0
                while want < depth and 0 <= row[want] < ks[want] and tuple(row[:want + 1]) in nodes[want + 1]:
                    want += 1
                assert reached[b] == want and got[b] == nodes[want][tuple(row[:want])], (depth, b, row)
            assert np.array_equal(exact_only(got, reached, depth) >= 0, reached == depth)
    if len(idx):                                                             # every held tuple is found, under its clamped codes
        c = clamp(idx, ks)
        got, reached = find_ref(trie, c, L, table)
        assert (reached == L).all()
        for i in range(len(idx)):
            assert i in trie["order"][int(trie["first"][got[i]]):int(trie["first"][got[i] + 1])]
            assert span_ref(trie, got[i], L) == (int(trie["first"][got[i]]), int(trie["first"][got[i] + 1]))
        assert span_ref(trie, 0, 0) == (0, len(idx))
        raw_out = np.flatnonzero(((idx < 0) | (idx >= np.array(ks))).any(1))   # out-of-range query codes are absent, not clamped
        if raw_out.size:
            _, reached = find_ref(trie, idx[raw_out], L, table)
            assert (reached < L).all()


@pytest.mark.parametrize("name", [r[0] for r in tc.MASK])
def test_mask_rule_is_set_membership(name):
    build, depth, V, ld, off, B, token_ids, eos, node, bits = tc.mask_case(name)
    trie = tc.build_case(build)[3]
    before = bits[off:].reshape(B, ld)
    after = mask_ref(trie, node, depth, token_ids, eos, before, V)
    assert np.array_equal(after[:, V:], before[:, V:])
    for b in range(B):
        allowed = {t for t in allowed_ref(trie, int(node[b]), depth, token_ids, eos) if 0 <= t < V}
        kept = set(np.flatnonzero(after[b, :V] != NEG_INF_BITS).tolist())
        assert kept == allowed and all(after[b, t] == before[b, t] for t in kept)
        if depth == trie["L"] or not 0 <= node[b] < trie["counts"][depth]:
            assert allowed == ({eos} if 0 <= eos < V else set())
    assert (before != NEG_INF_BITS).all() and np.isnan(before.view(np.float32)).all()


def test_mask_table_covers_what_it_should():
    names = {r[0]: r for r in tc.MASK}
    assert {r[3] for r in tc.MASK} >= {1, 3, 4, 5, 4097, 3 * tc.MASK_CHUNK + 1}
    assert {(r[5] + b * (r[3] + r[4])) % 4 for r in tc.MASK for b in range(r[6])} == {0, 1, 2, 3}      # every row alignment mod 16 bytes
    assert any(r[4] == 0 for r in tc.MASK) and any((r[3] + r[4]) % 2 == 1 and r[4] > 0 for r in tc.MASK)
    assert {names["odd_ld_small"][8], names["V4097"][8], names["three_chunks_ld_V"][8], names["one_child"][8]} == {0, 4096, -1}
    assert names["V5"][8] == names["V5"][3] - 1 and names["B0"][6] == 0
    case = tc.mask_case("three_chunks_ld_V")
    assert len(set(case[6].tolist())) < len(case[6]) and (case[6] < 0).any() and (case[6] >= case[2]).any()
    one = tc.build_case("one_tuple")[3]
    assert [np.diff(r).tolist() for r in one["child"]] == [[1], [1], [1]]
    full = tc.build_case("distinct")[3]
    assert np.diff(full["child"][0]).tolist() == [4] and (np.diff(full["child"][1]) == 4).all()


# ---- the query command -----------------------------------------------------------------------------------------------------------
def test_report_is_a_plain_function_of_the_exact_arrays():
    from lcrec_amd import query_indices as qi
    idx, ks, _, trie = tc.build_case("f6")
    table = tc.table_of("f6")
    rs = np.random.RandomState(5)
    q, W, L = 40, 4, 3
    tuples = idx[rs.randint(0, len(idx), (q, W))].copy()
    tuples[::3, 1, 2] = (tuples[::3, 1, 2] + 1 + rs.randint(0, 40, len(tuples[::3]))) % 48      # some miss at the last level
    tuples[::5, 2, 0] = 47 - tuples[::5, 2, 0]
    tuples[1::7, 3] = -1                                                                        # beams past the live count
    err = rs.rand(q, W).astype(np.float32)
    node, depth = find_ref(trie, tuples.reshape(-1, L), L, table)
    spans = np.array([span_ref(trie, node[i], int(depth[i])) for i in range(q * W)], dtype=np.int64).reshape(q, W, 2)
    rep = qi.build_query_report(tuples, err, depth.reshape(q, W), spans[..., 0], spans[..., 1], trie["order"], L)
    holders = brute_force(idx, ks)[1]
    live = tuples[:, :, 0] >= 0
    exact = np.array([[live[i, w] and tuple(tuples[i, w].tolist()) in holders for w in range(W)] for i in range(q)])
    assert (rep["queries"], rep["beam"], rep["levels"], rep["items"]) == (q, W, L, 3000)
    assert rep["exact_beam0"] == int(exact[:, 0].sum()) and rep["exact_any"] == int(exact.any(1).sum()) and 0 < rep["exact_any"] < q * W
    assert rep["mean_depth"] == pytest.approx(depth.reshape(q, W)[live].astype(np.float64).mean(), rel=1e-12)
    for i, beams in enumerate(rep["results"]):
        assert [b["beam"] for b in beams] == [w for w in range(W) if live[i, w]]
        for b in beams:
            t = tuple(tuples[i, b["beam"]].tolist())
            assert b["tuple"] == list(t) and b["err"] == float(err[i, b["beam"]])
            if t in holders:
                assert b["items"] == holders[t] and b["depth"] == L and "items_under_prefix" not in b
            else:
                under = int((idx[:, :b["depth"]] == np.array(t[:b["depth"]])).all(1).sum())
                assert b["items_under_prefix"] == under > 0 and b["depth"] < L and "items" not in b
    assert json.loads(json.dumps(rep)) == rep and len(qi.summary(rep)) == 2
    empty = qi.build_query_report(tuples[:0], err[:0], depth[:0].reshape(0, W), spans[:0, :, 0], spans[:0, :, 1], trie["order"], L)
    assert (empty["queries"], empty["exact_any"], empty["mean_depth"], empty["results"]) == (0, 0, 0.0, [])


def test_query_command_refuses_what_it_cannot_do(tmp_path, monkeypatch):
    from lcrec_amd import generate_indices as gen
    from lcrec_amd import query_indices as qi
    a = qi.parse_args(["--ckpt_path", "c.pth", "--index_file", "x.json", "--queries", "q.npy"])
    assert (a.index_file, a.queries, a.beam, a.report, a.device, a.trust_checkpoint) == ("x.json", "q.npy", 4, None, "cuda:0", False)
    assert qi.parse_args(["--ckpt_path", "c", "--index_file", "x", "--queries", "q", "--beam", "8", "--report", "r.json"]).beam == 8
    no, out = str(tmp_path / "no.pth"), str(tmp_path / "out.json")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="single process"):                            # before the checkpoint is opened
        qi.query(no, out, no, device="cpu")
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(ValueError, match="--beam 3"):
        qi.query(no, out, no, beam=3, device="cpu")
    with pytest.raises(FileNotFoundError):
        qi.query(no, out, no, device="cpu")
    args = argparse.Namespace(data_path="none.npy", num_emb_list=[8, 8], e_dim=16, layers=[32], dropout_prob=0.0, bn=False, loss_type="mse",
                              quant_loss_weight=1.0, kmeans_init=False, kmeans_iters=10, sk_epsilons=[0.0, 0.0], sk_iters=50)
    model = gen.build_model_from_args(args, 24)
    ckpt = str(tmp_path / "toy.pth")
    torch.save({"args": args, "epoch": 0, "state_dict": model.state_dict(), "optimizer": {}}, ckpt, pickle_protocol=4)
    good, narrow, flat, f64 = (str(tmp_path / f"{k}.npy") for k in ("good", "narrow", "flat", "f64"))
    np.save(good, np.zeros((5, 24), dtype=np.float32))
    np.save(narrow, np.zeros((5, 23), dtype=np.float32))
    np.save(flat, np.zeros(24, dtype=np.float32))
    np.save(f64, np.zeros((5, 24), dtype=np.float64))
    index = str(tmp_path / "four.index.json")
    gen.dump_index_json(np.zeros((4, 2), dtype=np.int64), index)
    with pytest.raises(ValueError, match=r"shape \(5, 23\) but the checkpoint's encoder takes rows of 24 floats"):
        qi.query(ckpt, index, narrow)
    with pytest.raises(ValueError, match=r"shape \(24,\)"):
        qi.query(ckpt, index, flat)
    with pytest.raises(ValueError, match="float64, not float32"):
        qi.query(ckpt, index, f64)
    three = str(tmp_path / "three.index.json")
    gen.dump_index_json(np.zeros((4, 3), dtype=np.int64), three)
    with pytest.raises(ValueError):                                                    # load_index_json's: 3 levels, the checkpoint has 2
        qi.query(ckpt, three, good)
    big = str(tmp_path / "big.index.json")
    gen.dump_index_json(np.array([[0, 8]], dtype=np.int64), big)
    with pytest.raises(ValueError, match="code 8 but the checkpoint's level 1 has 8 codes"):
        qi.query(ckpt, big, good)
    shim = open(os.path.join(ROOT, "index", "query_indices.py")).read()
    assert "from lcrec_amd.query_indices import main" in shim and len(shim.splitlines()) == 11
