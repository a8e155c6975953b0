"""MI355X: the index trie (lcrec_index_trie_build / _find / _mask_logits, ops.trie_*, IndexTrie, query_indices.main).

Everything is integer-exact or bit-exact against tests/trie_ref.py: there is no tolerance in this file.  Outputs lie between guard
bands in garbage-filled buffers and are compared WHOLE, so an element the rule does not write must still hold the garbage; the build's
workspace is exactly the queried size and filled with 0xFF; every row is called twice, the second time on the then dirty buffers.
For the mask the whole [B][ld] buffer -- the pad columns, the floats before the first row -- is compared as uint32."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

import finish_cases as fc
import golden_inputs as gi
import trie_cases as tc
from trie_ref import brute_force, clamp, exact_only, find_ref, mask_ref, span_ref, stats_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAND = 256                                                  # bytes on either side of every buffer the calls write
BAND_BYTE = 0x5A
GARBAGE = 0x7FC12345                                        # as int32; a NaN as a float
GARBAGE64 = GARBAGE | (GARBAGE << 32)
NP = {torch.int64: np.int64, torch.int32: np.int32, torch.float32: np.uint32, torch.uint8: np.uint8}


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)             # (a copy: the shared inputs are read-only arrays)


class Banded:
    """`count` elements of `dtype` as a view into a larger byte buffer: BAND bytes of BAND_BYTE, the elements, BAND bytes more."""

    def __init__(self, dtype, count):
        self.dtype, self.count = dtype, int(count)
        self.nbytes = self.count * torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full((BAND + self.nbytes + BAND,), BAND_BYTE, dtype=torch.uint8, device=DEV)
        self.bytes = self.raw[BAND:BAND + self.nbytes]
        self.view = self.bytes.view(dtype)
        assert self.view.data_ptr() % 16 == 0
        self.garbage()

    def garbage(self):
        if self.dtype == torch.uint8:
            self.bytes.fill_(0xFF)
        else:
            self.bytes.view(torch.int32).fill_(GARBAGE)

    def load(self, bits):
        self.bytes.view(torch.int32).copy_(torch.from_numpy(np.array(bits).view(np.int32)))

    def result(self):
        """the elements as numpy (floats as their uint32 bits), after checking the bands"""
        torch.cuda.synchronize()
        assert bool((self.raw[:BAND] == BAND_BYTE).all()) and bool((self.raw[BAND + self.nbytes:] == BAND_BYTE).all()), "written outside"
        host = self.bytes.cpu().numpy().copy()
        return host.view(NP[self.dtype])


_tries = {}


def trie_of(hip, name):
    """the row's trie on the device, built once (plain buffers) and shared by the find and mask rows"""
    if name not in _tries:
        idx, ks, _, _ = tc.build_case(name)
        _tries[name] = hip.ops.trie_build(dev(idx), ks)
    return _tries[name]


def image(ref, sizes):
    """what the five arrays must hold after a build into garbage: the rule's prefixes, garbage everywhere else"""
    n, L = ref["n"], ref["L"]
    want = {k: np.full(sizes[k], GARBAGE if k == "code" else GARBAGE64, dtype=np.int32 if k == "code" else np.int64) for k in sizes}
    want["order"][:n] = ref["order"]
    want["counts"][:L + 1] = ref["counts"]
    for d in range(L):
        want["child"][d * (n + 1):d * (n + 1) + len(ref["child"][d])] = ref["child"][d]
        want["code"][d * n:d * n + len(ref["code"][d])] = ref["code"][d]
    want["first"][:len(ref["first"])] = ref["first"]
    return want


# ---- build -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tc.BUILD))
def test_build_matches_the_rule(hip, name):
    idx, ks, stride, ref = tc.build_case(name)
    n, L = idx.shape
    lib = hip._lib.load()
    source = dev(tc.wide(idx, stride)) if stride else dev(idx)
    src = source[:, :L]
    before = source.clone()
    sizes = hip.ops.trie_array_sizes(n, L)
    bufs = {k: Banded(dtype, sizes[k]) for k, dtype in hip.ops.TRIE_ARRAYS}
    need = lib.lcrec_index_trie_build_workspace(n, L)
    assert (need > 0) == (n > 0)
    ws = Banded(torch.uint8, need)
    want = image(ref, sizes)
    for call in ("first", "second, on the dirty buffers and workspace"):
        trie = hip.ops.trie_build(src, ks, arrays={k: b.view for k, b in bufs.items()}, workspace=ws.view)
        assert (trie.n, trie.L, trie.ks, list(trie.record.K)[:L]) == (n, L, ks, ks)
        for k, b in bufs.items():
            got = b.result()
            if not np.array_equal(got, want[k]):
                bad = np.flatnonzero(got != want[k])
                raise AssertionError((name, call, k, len(bad), bad[:8], got[bad[:8]], want[k][bad[:8]]))
        ws.result()                                                                      # its bands
    assert torch.equal(source, before)                                                   # idx is never written
    if stride:
        assert src.stride(0) == stride > L


def test_build_refuses_a_small_workspace_through_the_binding(hip):
    idx, ks, _, _ = tc.build_case("n65")
    need = hip._lib.load().lcrec_index_trie_build_workspace(65, 3)
    with pytest.raises(hip.LcrecError, match=f"workspace of {need - 1} bytes, {need} needed"):
        hip.ops.trie_build(dev(idx), ks, workspace=torch.zeros(need - 1, dtype=torch.uint8, device=DEV))


# ---- find --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tc.BUILD))
def test_find_matches_the_rule(hip, name):
    idx, ks, _, ref = tc.build_case(name)
    trie, table, L = trie_of(hip, name), tc.table_of(name), len(ks)
    for depth in range(L + 1):
        batches = tc.FIND_BATCHES if L <= 4 or depth in (1, L) else tc.FIND_BATCHES[:3]
        for B in batches:
            q = tc.find_queries(name, depth, B)
            nodes, reached = find_ref(ref, q, depth, table)
            layouts = [("adjacent", dev(q))]
            if B == 65 and depth:                                                        # prefix_stride > depth
                spread = torch.full((B, depth + 2), 1 << 40, dtype=torch.int64, device=DEV)
                spread[:, :depth] = dev(q)
                layouts.append(("strided", spread[:, :depth]))
            for layout, qd in layouts:
                node_out, depth_out = Banded(torch.int64, B), Banded(torch.int32, B)
                for call in ("first", "second"):
                    hip.ops.trie_find(trie, qd, depth, longest=True, node_out=node_out.view, depth_out=depth_out.view)
                    assert np.array_equal(node_out.result(), nodes) and np.array_equal(depth_out.result(), reached), (name, depth, B, layout, call)
                hip.ops.trie_find(trie, qd, depth, node_out=node_out.view)               # without depth_out: -1 unless the full depth
                assert np.array_equal(node_out.result(), exact_only(nodes, reached, depth)), (name, depth, B, layout)
                assert np.array_equal(depth_out.result(), reached)                       # ... and depth_out was not touched
    got = hip.ops.trie_find(trie, None, 0, rows=5)
    assert got.tolist() == [0] * 5
    if len(idx):                                                                         # every held tuple, under its clamped codes
        c = clamp(idx, ks)
        leaf = hip.ops.trie_find(trie, dev(c), L).cpu().numpy()
        nodes, reached = find_ref(ref, c, L, table) if len(idx) <= 5000 else (leaf, np.full(len(idx), L))
        assert (leaf >= 0).all() and np.array_equal(leaf, nodes) and (reached == L).all()
        first, order = ref["first"], ref["order"]
        pos = np.empty(len(idx), dtype=np.int64)
        pos[order] = np.arange(len(idx))
        assert ((first[leaf] <= pos) & (pos < first[leaf + 1])).all()                    # item i lies in the leaf its tuple leads to


# ---- mask --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [r[0] for r in tc.MASK])
def test_mask_matches_the_rule_bit_for_bit(hip, name):
    build, depth, V, ld, off, B, token_ids, eos, node, bits = tc.mask_case(name)
    ref = tc.build_case(build)[3]
    trie = trie_of(hip, build)
    buf = Banded(torch.float32, off + B * ld)
    buf.load(bits)
    want = np.array(bits, copy=True)
    want[off:] = mask_ref(ref, node, depth, token_ids, eos, bits[off:].reshape(B, ld), V).reshape(-1)
    view = buf.view[off:].view(B, ld)[:, :V]
    if B:
        assert (view.data_ptr() // 4) % 4 == (buf.view.data_ptr() // 4 + off) % 4 and buf.view.data_ptr() % 16 == 0
    tok = None if token_ids is None else dev(token_ids)
    for call in ("first", "second, on the masked buffer"):
        hip.ops.trie_mask_logits_(trie, view, dev(node), depth, tok, eos)
        got = buf.result()
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            raise AssertionError((name, call, len(bad), bad[:8], got[bad[:8]], want[bad[:8]]))
    if B:
        assert (want[off:].reshape(B, ld)[:, :V] == 0xFF800000).any()


def test_index_trie_refuses_other_dtypes_and_devices(hip):
    t = hip.IndexTrie(trie_of(hip, "k48"))
    nodes = torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="float16"):
        t.mask_logits_(torch.zeros((2, 8), dtype=torch.float16, device=DEV), nodes, 1)
    with pytest.raises(ValueError, match="cpu"):
        t.mask_logits_(torch.zeros((2, 8), dtype=torch.float32), nodes, 1)
    with pytest.raises(ValueError, match="int32"):
        t.find(torch.zeros((2, 3), dtype=torch.int32))


# ---- find, then mask: recorded once, replayed on other inputs --------------------------------------------------------------------------
def test_find_then_mask_is_recorded_once_and_replayed_on_other_inputs(hip):
    _, ks, _, ref = tc.build_case("k48")
    trie, table = trie_of(hip, "k48"), tc.table_of("k48")
    depth, B, V, pad, eos = 2, 65, tc.MASK_CHUNK + 37, 3, 11
    ld = V + pad
    rs = np.random.RandomState(3)
    token_ids = rs.permutation(V)[:ks[depth]].astype(np.int32)
    sets = {}
    qa = tc.find_queries("k48", depth, B)
    for which, q in (("A", qa), ("B", np.roll(qa, 7, axis=0))):
        bits = (np.uint32(0x7FC00000) | rs.randint(1, 1 << 22, B * ld).astype(np.uint32)).astype(np.uint32)
        nodes, reached = find_ref(ref, q, depth, table)
        found = exact_only(nodes, reached, depth)
        sets[which] = (q, bits, found, mask_ref(ref, found, depth, token_ids, eos, bits.reshape(B, ld), V).reshape(-1))
    assert not np.array_equal(sets["A"][2], sets["B"][2]) and (sets["A"][2] < 0).any() and (sets["A"][2] >= 0).any()
    prefix = torch.empty((B, depth), dtype=torch.int64, device=DEV)
    node_out, logits = Banded(torch.int64, B), Banded(torch.float32, B * ld)
    tok = dev(token_ids)
    view = logits.view.view(B, ld)[:, :V]

    def call():
        hip.ops.trie_find(trie, prefix, depth, node_out=node_out.view)
        hip.ops.trie_mask_logits_(trie, view, node_out.view, depth, tok, eos)

    def load(which):
        prefix.copy_(torch.from_numpy(np.array(sets[which][0])))
        logits.load(sets[which][1])
        node_out.garbage()

    def check(which, what):
        side.synchronize()
        assert np.array_equal(node_out.result(), sets[which][2]), (what, "nodes")
        assert np.array_equal(logits.result(), sets[which][3]), (what, "logits")

    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(side):
            load("A")
            call()
            check("A", "eager call on A, on a side stream")
            load("A")
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                call()
            side.synchronize()
            assert np.array_equal(logits.result(), sets["A"][1]), "the capture itself ran something"
            load("B")
            graph.replay()
            check("B", "first replay, on B")
            load("A")
            graph.replay()
            check("A", "second replay, on A")
            load("B")
            graph.replay()
            check("B", "third replay, on B")
    finally:
        torch.cuda.synchronize()


# ---- F6: the class and the command ---------------------------------------------------------------------------------------------------
def _f6_trie(hip, tmp_path):
    idx, ks, _, ref = tc.build_case("f6")
    path = str(tmp_path / "F6.index.json")
    open(path, "wb").write(bytes(fc.f6_case()[3]["json_text"]))
    return hip.IndexTrie.from_file(path, ks, DEV), idx, ks, ref, path


def test_index_trie_from_file_on_f6(hip, tmp_path):
    t, idx, ks, ref, _ = _f6_trie(hip, tmp_path)
    assert t.nodes == tc.F6_COUNTS and (t.n, t.L, t.ks) == (3000, 3, ks)
    st = t.stats()
    assert st == stats_ref(ref) and st["largest_leaf"] == 4
    h = t.host()
    assert np.array_equal(h["order"], ref["order"]) and np.array_equal(h["first"], ref["first"])
    for d in range(3):
        assert np.array_equal(h["child"][d], ref["child"][d]) and np.array_equal(h["code"][d], ref["code"][d])
    # lookup: every item's own tuple returns that item among its holders, ascending
    items, offsets = (a.cpu().numpy() for a in t.lookup(dev(idx)))
    holders = brute_force(idx, ks)[1]
    assert offsets[0] == 0 and len(offsets) == 3001 and offsets[-1] == len(items)
    for i in range(3000):
        row = items[offsets[i]:offsets[i + 1]].tolist()
        assert i in row and row == holders[tuple(idx[i].tolist())]
    # the holders of a shared tuple are collision_groups' group for that tuple
    groups = hip.ops.collision_groups(dev(idx), ks)["groups"]
    assert len(groups) == sum(len(v) > 1 for v in holders.values()) > 0
    for g in groups:
        assert items[offsets[g[0]]:offsets[g[0] + 1]].tolist() == g
    # absent and out-of-range tuples hold nothing; an empty batch
    absent = np.array([[0, 0, 48], [-1, 3, 3], [47, 47, 47]], dtype=np.int64)
    absent = absent[[tuple(r) not in holders for r in absent.tolist()]]
    items2, offsets2 = t.lookup(dev(absent))
    assert items2.numel() == 0 and offsets2.tolist() == [0] * (len(absent) + 1)
    assert t.lookup(torch.zeros((0, 3), dtype=torch.int64))[1].tolist() == [0]
    # span: down the child chain
    for depth in range(4):
        nodes = np.arange(tc.F6_COUNTS[depth])
        lo, hi = (a.cpu().numpy() for a in t.span(dev(nodes), depth))
        want = np.array([span_ref(ref, j, depth) for j in nodes])
        assert np.array_equal(lo, want[:, 0]) and np.array_equal(hi, want[:, 1])
    node, reached = t.find(dev(idx[:7, :2]), longest=True)
    assert reached.tolist() == [2] * 7 and node.dtype == torch.int64 and reached.dtype == torch.int32


def test_prefix_allowed_tokens_fn_against_a_brute_force_walk(hip, tmp_path):
    t, idx, ks, ref, _ = _f6_trie(hip, tmp_path)
    rs = np.random.RandomState(11)
    tables = [32000 + 100 * l + rs.permutation(48) for l in range(3)]
    eos, sep = 2, [13, 29871, 13]
    fn = t.prefix_allowed_tokens_fn(tables, eos, sep)
    seen = set()
    for k in range(50):
        i = k % 4                                                                        # codes after the separator
        codes = idx[rs.randint(0, 3000)][:i].copy()
        if k % 5 == 4 and i:
            codes[-1] = (codes[-1] + 1 + rs.randint(0, 46)) % 48                         # maybe a prefix no item holds
        prompt = rs.randint(100, 30000, rs.randint(0, 9)).tolist()
        sentence = torch.tensor(prompt + sep + [int(tables[l][c]) for l, c in enumerate(codes)], dtype=torch.int64)
        under = idx[(idx[:, :i] == codes).all(1)] if i else idx
        if i == 3:
            want = [eos]
        elif len(under) == 0:
            want = [eos]
        else:
            want = sorted(int(tables[i][c]) for c in set(under[:, i].tolist()))
        got = fn(k, sentence)
        assert sorted(got) == want and len(set(got)) == len(got), (k, codes, got, want)
        seen.add((i, len(under) == 0))
    assert seen >= {(0, False), (1, False), (2, False), (3, False)} and any(absent for _, absent in seen)
    assert fn(0, torch.tensor([5, 6, 7], dtype=torch.int64)) is None                     # no separator: the reference's answer
    per_position = [sorted(int(tables[l][c]) for c in set(idx[:, l].tolist())) for l in range(3)]
    first = idx[0]
    narrowed = fn(0, torch.tensor(sep + [int(tables[0][first[0]])], dtype=torch.int64))
    assert set(narrowed) < set(per_position[1])                                          # fewer than the per-position set admits


def _checkpoint(tmp_path, g, meta):
    kw = {k: v for k, v in meta["model"].items() if k != "in_dim"}
    sd = {k[4:]: torch.from_numpy(g[k].copy()) for k in g.files if k.startswith("sd__")}
    args = argparse.Namespace(data_path=str(tmp_path / "none.npy"), num_workers=0, **kw)
    ckpt = str(tmp_path / "toy.pth")
    torch.save({"args": args, "epoch": 0, "best_loss": 0.0, "best_collision_rate": 0.0, "state_dict": sd, "optimizer": {}}, ckpt,
               pickle_protocol=4)
    return ckpt


def test_query_indices_on_f6(hip, oracle, tmp_path):
    from lcrec_amd import query_indices as qi
    t, idx, ks, ref, path = _f6_trie(hip, tmp_path)
    g = fc.f6_case()[3]
    meta = json.load(open(os.path.join(fc.GOLD, "manifest.json")))["fixtures"]["f6_generate.npz"]
    names = gi.state_dict_names(len(meta["model"]["layers"]) + 1, meta["model"]["bn"], len(meta["model"]["num_emb_list"]))
    cbs = [gi.f32(g["sd__" + n]) for n in names["codebooks"]]
    items = gi.toy_items(meta["seed"])[:64]
    greedy = oracle.encode_assign(items, [g["sd__" + n + ".weight"] for n in names["encoder"]],
                                  [g["sd__" + n + ".bias"] for n in names["encoder"]], cbs)["idx"].astype(np.int64)
    ckpt = _checkpoint(tmp_path, g, meta)
    qnpy, report = str(tmp_path / "Q.npy"), str(tmp_path / "r" / "query.json")
    np.save(qnpy, items)
    holders = brute_force(idx, ks)[1]

    def consistent(rep, W):
        assert (rep["queries"], rep["beam"], rep["levels"], rep["items"]) == (64, W, 3, 3000)
        exact0 = exact_any = 0
        depths = []
        for beams in rep["results"]:
            assert [b["beam"] for b in beams] == list(range(len(beams))) and 1 <= len(beams) <= W
            hits = []
            for b in beams:
                tup = tuple(b["tuple"])
                d = 0
                while d < 3 and (idx[:, :d + 1] == np.array(tup[:d + 1])).all(1).any():
                    d += 1
                assert b["depth"] == d
                depths.append(d)
                hits.append(d == 3)
                if d == 3:
                    assert b["items"] == holders[tup]
                else:
                    assert b["items_under_prefix"] == int((idx[:, :d] == np.array(tup[:d])).all(1).sum())
            exact0 += hits[0]
            exact_any += any(hits)
        assert (rep["exact_beam0"], rep["exact_any"]) == (exact0, exact_any)
        assert rep["mean_depth"] == pytest.approx(np.mean(depths), rel=1e-12)

    rep4 = qi.main(["--ckpt_path", ckpt, "--index_file", path, "--queries", qnpy, "--beam", "4", "--device", DEV, "--report", report])
    consistent(rep4, 4)
    assert json.load(open(report)) == rep4 and rep4["exact_any"] >= rep4["exact_beam0"] > 0
    rep1 = qi.main(["--ckpt_path", ckpt, "--index_file", path, "--queries", qnpy, "--beam", "1", "--device", DEV])
    consistent(rep1, 1)
    listed = 0
    for i, beams in enumerate(rep1["results"]):
        assert beams[0]["tuple"] == greedy[i].tolist()                                   # W = 1: beam 0 is the greedy tuple
        if (greedy[i] == idx[i]).all():
            assert i in beams[0]["items"]                                                # ... and where the file holds it, the item is listed
            listed += 1
    assert listed == int((greedy == idx[:64]).all(1).sum()) > 0                          # (the fixture's own count: the file's tuples come from a later round)
