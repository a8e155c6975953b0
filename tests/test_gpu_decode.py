"""MI355X: the decode pass (lcrec_decode_tuples, ops.decode_tuples, RQVAE.decode_indices, decode_indices.main, audit_indices --recon).

Every per-item comparison is exact: the kernels and tests/decode_ref.py evaluate the same fp32 operations in the same order -- the
gather's adds in level order, the layers' fma chains (lcrec_linear_forward against oracle.linear), one error chain per row -- so xq,
out, err (both losses) and flags must agree bit for bit (where the rule gives a NaN, any NaN counts).  Report floats are compared to
float64 aggregates of the reference arrays at 1e-12 relative, as tests/test_gpu_audit.py compares its report: fp64 rounding, 1.1e-16,
times at most a few thousand summands, whatever the order of summation; report integers exactly.
Outputs sit between guard bands and are pre-filled with garbage; the workspace is exactly the queried size and filled with NaN; every
row is called twice, the second time (for the other loss) on the then dirty buffers and workspace."""
import argparse
import itertools
import json
import os

import numpy as np
import pytest
import torch

import audit_cases as ac
import decode_cases as dc
import extend_cases as ec
import finish_cases as fc
import golden_inputs as gi
from decode_ref import decode_ref, recon_report_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64                                                  # elements on either side of every output
BAND, GARBAGE = 0x5A5A5A5A, 0x7FC12345                      # (as int32; GARBAGE is a NaN as a float)
REL = 1e-12
NAMES = ("xq", "out", "err", "flags")


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)             # (a copy: the shared inputs are read-only arrays)


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return False
    if got.dtype.kind != "f":
        return np.array_equal(got.astype(np.int64), want.astype(np.int64))
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].astype(np.float32).view(np.uint32))


class Guarded:
    """The outputs of one call as views into larger buffers: GUARD elements of BAND, the output filled with GARBAGE, GUARD of BAND."""

    def __init__(self, n, e, w, names):
        self.shape = {"xq": (n, e), "out": (n, w), "err": (n,), "flags": (n,)}
        self.raw, self.into, self.need = {}, {}, {}
        for name in names:
            need = int(np.prod(self.shape[name]))
            raw = torch.full((GUARD + need + GUARD,), BAND, dtype=torch.int32, device=DEV)
            raw[GUARD:GUARD + need] = GARBAGE
            self.raw[name], self.need[name] = raw, need
            self.into[name] = raw[GUARD:].view(torch.int32 if name == "flags" else torch.float32)   # the far band lies inside it

    def result(self):
        out = {}
        for name, raw in self.raw.items():
            need = self.need[name]
            assert bool((raw[:GUARD] == BAND).all()) and bool((raw[GUARD + need:] == BAND).all()), f"{name}: written outside its rows"
            out[name] = self.into[name][:need].cpu().numpy().reshape(self.shape[name]).copy()
        return out


def run(hip, idx, cbs, decoder, x, names=NAMES, chunk_rows=0, idx_dev=None):
    """ops.decode_tuples into guarded buffers with an exactly sized, NaN-filled workspace: once for the squared error and once more,
    on the dirty buffers and workspace, for the L1 error.  -> dict of numpy arrays (err_l1 beside err)"""
    dims, Ws, bs, scs, shs = decoder
    flat, ks = hip.ops.flatten_codebooks([dev(c) for c in cbs])
    held = dev(idx) if idx_dev is None else idx_dev
    n = held.shape[0]
    dW, db = [dev(w) for w in Ws], [dev(b) for b in bs]
    dsc = None if scs is None else [None if s is None else dev(s) for s in scs]
    dsh = None if shs is None else [None if s is None else dev(s) for s in shs]
    xd = dev(x) if "err" in names else None
    g = Guarded(n, dims[0], dims[-1], names)
    lib = hip._lib.load()
    ints = lambda v: (__import__("ctypes").c_int * len(v))(*[int(k) for k in v])
    size = lib.lcrec_debug_decode_tuples_workspace(n, ints(dims), len(dims) - 1, ints(ks), len(ks), int("out" in names), int(chunk_rows))
    assert size > 0
    ws = torch.full((size,), 0xFF, dtype=torch.uint8, device=DEV)                      # every float of it a NaN
    kw = dict(bn_scales=dsc, bn_shifts=dsh, x=xd, chunk_rows=chunk_rows, into=g.into, workspace=ws)
    hip.ops.decode_tuples(held, flat, ks, dW, db, l1=False, **kw)
    first = g.result()
    hip.ops.decode_tuples(held, flat, ks, dW, db, l1=True, **kw)
    second = g.result()
    for name in first:
        if name != "err":
            assert same_bits(second[name], first[name]), f"{name}: the second call on the dirty buffers differs"
    if "err" in first:
        first["err_l1"] = second["err"]
    return first


def check(got, want, what=""):
    for name in got:
        w = want[name]
        if not same_bits(got[name], w):
            bad = np.flatnonzero((np.asarray(got[name]).reshape(len(w), -1) != np.asarray(w).reshape(len(w), -1)).any(1))
            raise AssertionError((what, name, len(bad), bad[:8], np.asarray(got[name])[bad[:4]], np.asarray(w)[bad[:4]]))


# ---- the table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", dc.rows(), ids=dc.row_id)
def test_kernels_match_the_rule_on_greedy_and_random_tuples(hip, oracle, row):
    e, ks, n, form, w = row
    _, cbs, greedy, _, rand = ac.inputs(e, ks, n)
    for which, idx in (("greedy", greedy), ("random", rand)):
        got = run(hip, idx, cbs, dc.decoder(e, form, w), dc.embeddings(n, w))
        assert set(got) == {"xq", "out", "err", "err_l1", "flags"}
        check(got, dc.reference(e, ks, n, form, w, which), (row, which))


@pytest.mark.parametrize("row", dc.LOOPING, ids=lambda r: f"{r[0]}-n{r[3]}")
def test_item_loops_make_more_than_one_trip(hip, oracle, row):
    """More items than the grid covers at once (dc.LOOPING says why these sizes): the second trip of each kernel's loop, its stride
    and the ragged tail of the last trip."""
    _, e, ks, n = row
    cbs, idx, decoder, x = dc.looping_inputs(e, ks, n)
    got = run(hip, idx, cbs, decoder, x)
    check(got, decode_ref(idx, cbs, decoder[1], decoder[2], None, None, x), row)


@pytest.mark.parametrize("L", [1, 3, ac.MAX_LEVELS])
def test_out_of_range_codes_are_clamped_and_flagged(hip, oracle, L):
    cbs, idx, level, K, decoder, x = dc.out_of_range_case(L)
    got = run(hip, idx, cbs, decoder, x)
    check(got, decode_ref(idx, cbs, decoder[1], decoder[2], decoder[3], decoder[4], x), ("out of range", L))
    assert np.array_equal(got["flags"], np.where(np.arange(len(idx)) % 4 == 3, 0, 1 << level))
    clamped = idx.copy()
    clamped[:, level] = np.resize(np.array([0, K - 1, K - 1, min(5, K - 1)]), len(idx))
    again = run(hip, clamped, cbs, decoder, x)
    for name in ("xq", "out", "err", "err_l1"):
        assert same_bits(got[name], again[name]), name
    assert (again["flags"] == 0).all()


def test_nan_and_inf_come_out_where_the_rule_puts_them(hip, oracle):
    cbs, idx, decoder, x = dc.nan_case()
    got = run(hip, idx, cbs, decoder, x)
    check(got, decode_ref(idx, cbs, decoder[1], decoder[2], None, None, x), "nan")
    assert np.isnan(got["out"][:3]).all() and np.isnan(got["err"][:4]).all() and np.isnan(got["err_l1"][:4]).all()
    assert np.isposinf(got["err"][5]) and np.isposinf(got["err_l1"][5]) and np.isfinite(got["err"][6:]).all()


def test_tuples_as_columns_of_a_wider_matrix(hip, oracle):
    e, ks, n, form, w = 32, (48, 100, 7), 257, "hidden_bn", 100
    _, cbs, _, _, rand = ac.inputs(e, ks, n)
    L = len(ks)
    wide = gi.rs(6400).randint(-9, 1 << 20, size=(n, L + 5)).astype(np.int64)
    wide[:, 2:2 + L] = rand
    wide_dev = dev(wide)
    got = run(hip, None, cbs, dc.decoder(e, form, w), dc.embeddings(n, w), idx_dev=wide_dev[:, 2:2 + L])
    check(got, dc.reference(e, ks, n, form, w, "random"), "strided")
    assert np.array_equal(wide_dev.cpu().numpy(), wide)                              # idx is never written
    with pytest.raises(hip.LcrecError, match="column block"):
        flat, kl = hip.ops.flatten_codebooks([dev(c) for c in cbs])
        hip.ops.decode_tuples(wide_dev[:, 0:2 * L:2], flat, kl, [dev(v) for v in dc.decoder(e, form, w)[1]], [None, None])


@pytest.mark.parametrize("form,w", [("hidden_bn", 100), ("single", 33), ("hidden", 772)])
def test_every_chunking_gives_the_bits_of_the_unchunked_call(hip, oracle, form, w):
    e, ks, n = 32, (48, 100, 7), 257
    _, cbs, _, _, rand = ac.inputs(e, ks, n)
    whole = run(hip, rand, cbs, dc.decoder(e, form, w), dc.embeddings(n, w))
    check(whole, dc.reference(e, ks, n, form, w, "random"), "unchunked")
    for chunk_rows in dc.CHUNKINGS(n)[1:]:
        got = run(hip, rand, cbs, dc.decoder(e, form, w), dc.embeddings(n, w), chunk_rows=chunk_rows)
        for name in whole:
            assert same_bits(got[name], whole[name]), (chunk_rows, name)


def test_every_combination_of_optional_outputs(hip, oracle):
    e, ks, n, form, w = 16, (48, 100, 7), 65, "hidden", 100
    _, cbs, _, _, rand = ac.inputs(e, ks, n)
    decoder, x = dc.decoder(e, form, w), dc.embeddings(n, w)
    full = run(hip, rand, cbs, decoder, x)
    check(full, dc.reference(e, ks, n, form, w, "random"), "full")
    for k in (1, 2, 3):
        for main in itertools.combinations(("xq", "out", "err"), k):
            for names in (main, main + ("flags",)):
                part = run(hip, rand, cbs, decoder, x, names=names, chunk_rows=30)
                assert set(part) == set(names) | ({"err_l1"} if "err" in names else set())
                for name in part:
                    assert same_bits(part[name], full[name]), (names, name)
    # ... and the tensors the binding allocates itself
    flat, kl = hip.ops.flatten_codebooks([dev(c) for c in cbs])
    dW, db = [dev(v) for v in decoder[1]], [dev(v) for v in decoder[2]]
    res = hip.ops.decode_tuples(dev(rand), flat, kl, dW, db)
    assert res["xq"] is None and res["err"] is None and res["flags"].dtype == torch.int32
    assert same_bits(res["out"].cpu().numpy(), full["out"]) and same_bits(res["flags"].cpu().numpy(), full["flags"])
    res = hip.ops.decode_tuples(dev(rand), flat, kl, dW, db, x=dev(x), l1=True, want_out=False, want_xq=True)
    assert res["out"] is None and same_bits(res["xq"].cpu().numpy(), full["xq"]) and same_bits(res["err"].cpu().numpy(), full["err_l1"])
    empty = hip.ops.decode_tuples(torch.zeros((0, 3), dtype=torch.int64, device=DEV), flat, kl, dW, db, x=torch.zeros((0, w), device=DEV))
    assert empty["out"].shape == (0, w) and empty["err"].shape == (0,)


def test_refusals_launch_nothing_and_every_chunk_is_traced(hip, oracle):
    e, ks, n, form, w = 16, (48, 100, 7), 257, "hidden", 100
    _, cbs, _, _, rand = ac.inputs(e, ks, n)
    dims, Ws, bs, _, _ = dc.decoder(e, form, w)
    flat, kl = hip.ops.flatten_codebooks([dev(c) for c in cbs])
    dW, db, held, xd = [dev(v) for v in Ws], [dev(v) for v in bs], dev(rand), dev(dc.embeddings(n, w))
    f = hip.ops.decode_tuples

    def refused(match, *args, **kw):
        with pytest.raises(hip.LcrecError, match=match):
            ec.in_thread(f, *args, **kw)                                               # (the last-error text stays in that thread)

    hip.ops.trace_enable(True)
    try:
        refused("e_dim=24", held, torch.zeros(155 * 24, device=DEV), kl, [torch.zeros((40, 24), device=DEV), dW[1]], db)
        bad = [dW[0], torch.zeros((44, 40), device=DEV), torch.zeros((w, 44), device=DEV)]
        refused(r"layer 2 \(in_dim=44, out_dim=100", held, flat, kl, bad, [db[0], None, db[1]])    # the LAST layer: nothing ran before it
        refused("no output asked for", held, flat, kl, dW, db, want_out=False)
        refused("16-byte aligned", held, flat, kl, dW, db, x=torch.zeros(n * w + 4, device=DEV)[1:1 + n * w].view(n, w))
        refused("workspace of 256 bytes", held, flat, kl, dW, db, workspace=torch.zeros(256, dtype=torch.uint8, device=DEV))
        refused("idx must be an int64", held.to(torch.int32), flat, kl, dW, db)                            # what the binding itself refuses
        refused("codebooks hold", held, flat, [48, 100], dW, db)
        refused("does not chain", held, flat, kl, [dW[0], dW[0]], db)
        torch.cuda.synchronize()
        assert hip.ops.trace_collect() == {}
        f(held, flat, kl, dW, db, x=xd, chunk_rows=100)                                # 3 chunks
        torch.cuda.synchronize()
        traced = hip.ops.trace_collect()
        assert traced["rq_decode_gather"][0] == 3 and traced["recon_row_error"][0] == 3
        assert sum(v[0] for k, v in traced.items() if k.startswith("linear_fwd")) == 3 * 2
        f(held, flat, kl, dW, db, want_out=False, want_xq=True, chunk_rows=64)        # xq alone: 5 gathers and nothing else
        torch.cuda.synchronize()
        assert {k: v[0] for k, v in hip.ops.trace_collect().items()} == {"rq_decode_gather": 5}
        f(held, flat, kl, dW, db)                                                      # out alone: no error kernel
        torch.cuda.synchronize()
        traced = hip.ops.trace_collect()
        assert traced["rq_decode_gather"][0] == 1 and "recon_row_error" not in traced
    finally:
        hip.ops.trace_enable(False)


def test_the_call_is_capturable(hip, oracle):
    """No allocation and no host synchronisation: the pass is recorded into a graph and replayed on new tuples."""
    e, ks, n, form, w = 32, (48, 100, 7), 257, "hidden_bn", 100
    _, cbs, greedy, _, rand = ac.inputs(e, ks, n)
    dims, Ws, bs, scs, shs = dc.decoder(e, form, w)
    flat, kl = hip.ops.flatten_codebooks([dev(c) for c in cbs])
    dW, db, dsc, dsh = [dev(v) for v in Ws], [dev(v) for v in bs], [None if s is None else dev(s) for s in scs], [None if s is None else dev(s) for s in shs]
    held, xd = dev(greedy), dev(dc.embeddings(n, w))
    into = {"out": torch.empty((n, w), device=DEV), "err": torch.empty(n, device=DEV), "flags": torch.empty(n, dtype=torch.int32, device=DEV)}
    ws = torch.empty(hip.ops.decode_plan(n, dims, kl, want_out=True, chunk_rows=100)["total_bytes"], dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip.ops.decode_tuples(held, flat, kl, dW, db, dsc, dsh, x=xd, chunk_rows=100, into=into, workspace=ws)   # warm-up, eagerly
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.ops.decode_tuples(held, flat, kl, dW, db, dsc, dsh, x=xd, chunk_rows=100, into=into, workspace=ws)
    held.copy_(dev(rand))
    graph.replay()
    torch.cuda.synchronize()
    want = dc.reference(e, ks, n, form, w, "random")
    assert same_bits(into["out"].cpu().numpy(), want["out"]) and same_bits(into["err"].cpu().numpy(), want["err"])


# ---- end to end on F6 ------------------------------------------------------------------------------------------------------------
def _checkpoint(tmp_path, g, meta):
    npy = str(tmp_path / "Toy.emb.npy")
    np.save(npy, gi.toy_items(meta["seed"]))
    kw = {k: v for k, v in meta["model"].items() if k != "in_dim"}
    sd = {k[4:]: torch.from_numpy(g[k].copy()) for k in g.files if k.startswith("sd__")}
    args = argparse.Namespace(data_path=npy, num_workers=0, **kw)
    ckpt = str(tmp_path / "toy.pth")
    torch.save({"args": args, "epoch": 0, "best_loss": 0.0, "best_collision_rate": 0.0, "state_dict": sd, "optimizer": {}}, ckpt,
               pickle_protocol=4)
    return ckpt


_f6 = {}


def _f6_model(oracle):
    """(items, codebooks, pass-1 tuples, decoder weights, decoder biases, fixture, meta) of the F6 model on the oracle, once"""
    if not _f6:
        g = fc.f6_case()[3]
        meta = json.load(open(os.path.join(fc.GOLD, "manifest.json")))["fixtures"]["f6_generate.npz"]
        names = gi.state_dict_names(len(meta["model"]["layers"]) + 1, meta["model"]["bn"], len(meta["model"]["num_emb_list"]))
        cbs = [gi.f32(g["sd__" + n]) for n in names["codebooks"]]
        items = gi.toy_items(meta["seed"])
        enc = oracle.encode_assign(items, [g["sd__" + n + ".weight"] for n in names["encoder"]],
                                   [g["sd__" + n + ".bias"] for n in names["encoder"]], cbs)
        Ws = [gi.f32(g["sd__" + n + ".weight"]) for n in names["decoder"]]
        bs = [gi.f32(g["sd__" + n + ".bias"]) for n in names["decoder"]]
        _f6["model"] = (items, cbs, enc["idx"].astype(np.int64), Ws, bs, g, meta)
    return _f6["model"]


def _compare_recon(rep, mine, theirs, held, greedy):
    want = recon_report_ref(mine["err"], theirs["err"], held, greedy, mine["flags"], 128, "mse")
    assert set(rep) == set(want)
    for key, w in want.items():
        print(key, rep[key], w)
        if isinstance(w, float):
            assert rep[key] == pytest.approx(w, rel=REL, abs=0.0), key
        else:
            assert rep[key] == w, key
    assert json.loads(json.dumps(rep)) == rep                                        # plain numbers and lists: it goes into a JSON file


@pytest.mark.parametrize("source", ["finish_nearest_free", "the_references_own_file"])
def test_decode_indices_on_f6(hip, oracle, tmp_path, source):
    from lcrec_amd import audit_indices as ai
    from lcrec_amd import decode_indices as di
    from lcrec_amd import generate_indices as gen
    items, cbs, pass1, Ws, bs, g, meta = _f6_model(oracle)
    ckpt = _checkpoint(tmp_path, g, meta)
    ks = [c.shape[0] for c in cbs]
    path = str(tmp_path / "Toy.index.json")
    if source == "finish_nearest_free":
        gen.generate(ckpt, path, device=DEV, verbose=False, finish="nearest_free")
    else:
        open(path, "wb").write(bytes(g["json_text"]))
    held = gen.load_index_json(path, ks)
    mine, theirs = decode_ref(held, cbs, Ws, bs, x=items), decode_ref(pass1, cbs, Ws, bs, x=items)
    npy, report = str(tmp_path / "o" / "Recon.npy"), str(tmp_path / "r" / "recon.json")
    rep = di.main(["--ckpt_path", ckpt, "--index_file", path, "--device", DEV, "--output", npy, "--report", report])
    _compare_recon(rep, mine, theirs, held, pass1)
    assert json.load(open(report)) == rep
    assert rep["moved_items"] == int((held != pass1).any(1).sum()) > 0 and rep["recon_file"] > 0 and rep["recon_greedy"] > 0
    recon = np.load(npy)
    assert recon.dtype == np.float32 and same_bits(recon, mine["out"])              # the .npy holds the reference's bits
    # --no_data: the same reconstruction, no error figures
    npy2 = str(tmp_path / "Recon2.npy")
    bare = di.main(["--ckpt_path", ckpt, "--index_file", path, "--device", DEV, "--output", npy2, "--no_data"])
    assert bare == {"items": 3000, "in_dim": 128, "loss_type": "mse", "clamped_items": 0} and same_bits(np.load(npy2), mine["out"])
    # the model's own method
    model = gen.build_model_from_args(torch.load(ckpt, weights_only=False)["args"], 128)
    model.load_state_dict({k[4:]: torch.from_numpy(g[k].copy()) for k in g.files if k.startswith("sd__")})
    model = model.to(DEV).eval()
    out, err = model.decode_indices(dev(held), dev(items))
    assert same_bits(out.cpu().numpy(), mine["out"]) and same_bits(err.cpu().numpy(), mine["err"])
    assert same_bits(model.decode_indices(dev(held)).cpu().numpy(), mine["out"])
    # audit_indices --recon: the old report plus `recon`; without the flag exactly the old report
    old = ai.main(["--ckpt_path", ckpt, "--index_file", path, "--device", DEV])
    assert "recon" not in old and old["items"] == 3000
    new = ai.main(["--ckpt_path", ckpt, "--index_file", path, "--device", DEV, "--recon"])
    assert new["recon"] == rep and {k: v for k, v in new.items() if k != "recon"} == old
