"""CPU: the host side of the decode pass -- the lcrec_decode_tuples entries (declared, exported, bound; every argument check returns
before any launch), the plan of its chunk walk, the numpy statement of its rule (tests/decode_ref.py) on every row of the case table,
the link between the sum of the codes and the quantiser's own straight-through sum, the report's arithmetic and the commands'
refusals."""
import argparse
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import audit_cases as ac
import decode_cases as dc
import extend_cases as ec
import finish_cases as fc
import golden_inputs as gi
from decode_ref import decode_ref, gather_ref, recon_report_ref, row_error_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("lcrec_decode_tuples", "lcrec_decode_tuples_workspace", "lcrec_decode_tuples_chunk_rows", "lcrec_debug_decode_tuples",
           "lcrec_debug_decode_tuples_plan", "lcrec_debug_decode_tuples_workspace")


def test_header_still_says_abi_3_and_the_library_exports_the_decode_entries():
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
    assert len(lib.lcrec_decode_tuples.argtypes) == 21 and len(lib.lcrec_debug_decode_tuples.argtypes) == 22
    assert lib.lcrec_decode_tuples.argtypes[:3] == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64]
    assert lib.lcrec_decode_tuples_workspace.restype is ctypes.c_size_t and lib.lcrec_decode_tuples_chunk_rows.restype is ctypes.c_int64
    assert [f for f, _ in lcrec_amd._lib.DecodePlan._fields_] == ["n", "chunk_rows", "n_chunks", "last_chunk_rows", "widest", "act_bytes",
                                                                  "act_offset", "q_offset", "q_bytes", "total_bytes"]
    assert callable(lcrec_amd.ops.decode_tuples) and callable(lcrec_amd.RQVAE.decode_indices)


# ---- the plan of the chunk walk ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want_out", [0, 1])
@pytest.mark.parametrize("dims", [[16, 40, 100], [32, 772], [64, 128, 512, 36]], ids=lambda d: "x".join(map(str, d)))
def test_plan_cuts_the_rows_and_lays_out_disjoint_buffers(dims, want_out):
    import lcrec_amd
    lib = lcrec_amd._lib.load()
    n, ks = 1000, [48, 100, 7]
    e, hidden, w = dims[0], dims[1:-1], dims[-1]
    for chunk_rows in dc.CHUNKINGS(n):
        p = lcrec_amd.ops.decode_plan(n, dims, ks, want_out=want_out, chunk_rows=chunk_rows)
        rows = min(chunk_rows or lib.lcrec_decode_tuples_chunk_rows(), n)
        assert (p["n"], p["chunk_rows"], p["n_chunks"]) == (n, rows, -(-n // rows))
        assert p["last_chunk_rows"] == n - (p["n_chunks"] - 1) * rows and 1 <= p["last_chunk_rows"] <= rows
        assert p["widest"] == max(hidden + ([] if want_out else [w]), default=0)
        assert p["act_bytes"] == -(-rows * p["widest"] * 4 // 256) * 256
        assert p["act_offset"] == [0, p["act_bytes"]] and p["q_offset"] == 2 * p["act_bytes"]
        assert p["q_bytes"] == -(-rows * e * 4 // 256) * 256 and p["total_bytes"] == p["q_offset"] + p["q_bytes"]
        ints = lambda v: (ctypes.c_int * len(v))(*v)
        assert lib.lcrec_debug_decode_tuples_workspace(n, ints(dims), len(dims) - 1, ints(ks), 3, want_out, chunk_rows) == p["total_bytes"]
        if chunk_rows == 0:
            assert lib.lcrec_decode_tuples_workspace(n, ints(dims), len(dims) - 1, ints(ks), 3, want_out) == p["total_bytes"]
    assert lib.lcrec_decode_tuples_chunk_rows() == 524288
    empty = lcrec_amd.ops.decode_plan(0, dims, ks, want_out=want_out)
    assert (empty["n_chunks"], empty["last_chunk_rows"], empty["chunk_rows"]) == (0, 0, 1)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_entry_reports_argument_errors_before_any_launch():
    """Each refusal names its argument (a layer's by its number) and comes back before anything is enqueued, so no device is needed.
    (In a thread of its own: the library's last-error text is per thread, and other tests expect this thread's to be empty.)"""
    import lcrec_amd
    lib = lcrec_amd._lib.load()
    seen, sizes = [], []

    def calls():
        buf = (ctypes.c_double * 64)()
        base = ctypes.cast(buf, ctypes.c_void_p).value
        p = ctypes.c_void_p((base + 15) & ~15)                       # 16-byte aligned
        off2, off4, off8 = (ctypes.c_void_p(p.value + k) for k in (2, 4, 8))
        ints = lambda *v: (ctypes.c_int * len(v))(*v)
        ptrs = lambda *v: (ctypes.c_void_p * len(v))(*v)
        both = ptrs(p.value, p.value)

        def call(rc, word, idx=p, stride=0, n=8, cb=p, K=ints(48, 100, 7), L=3, dims=ints(16, 40, 100), nl=2, W=both, b=both, sc=None,
                 sh=None, xq=p, out=p, x=p, l1=0, err=p, flags=p, ws=p, ws_bytes=1 << 40, chunk=None):
            args = (idx, stride, n, cb, K, L, dims, nl, W, b, sc, sh, xq, out, x, l1, err, flags, ws, ws_bytes, None)
            got = lib.lcrec_decode_tuples(*args) if chunk is None else lib.lcrec_debug_decode_tuples(*args, chunk)
            seen.append((got, rc, word, lib.lcrec_last_error()))

        call(-1, b"K is NULL", K=None)
        call(-1, b"dims is NULL", dims=None)
        call(-1, b"L=0", L=0)
        call(-1, b"L=17", L=17)
        call(-1, b"n_layers=0", nl=0)
        call(-1, b"n_layers=17", nl=17)
        call(-1, b"n=-1", n=-1)
        call(-1, b"chunk_rows=-4", chunk=-4)
        for e in (0, 8, 24, 128):
            call(-1, b"e_dim=%d" % e, dims=ints(e, 40, 100))
        call(-1, b"K[1]=0", K=ints(48, 0, 7))
        call(-1, b"layer 1: dims[2]=0", dims=ints(16, 40, 0))
        call(-2, b"layer 1 (in_dim=44, out_dim=100", dims=ints(16, 44, 100))   # lcrec_linear_forward's refusal, and its code
        call(-1, b"idx_stride=2 < L=3", stride=2)
        call(-1, b"idx is NULL", idx=None)
        call(-1, b"codebooks is NULL", cb=None)
        call(-1, b"no output asked for", xq=None, out=None, x=None, err=None)
        call(-1, b"x and err_out are given together", x=None)
        call(-1, b"x and err_out are given together", err=None)
        call(-1, b"W is NULL", W=None)
        call(-1, b"b is NULL", b=None)
        call(-1, b"layer 1: W[1] is NULL", W=ptrs(p.value, None))
        call(-1, b"layer 0: bn_scale and bn_shift", sc=both, sh=ptrs(None, p.value))
        call(-1, b"layer 1: W[1] must be 16-byte aligned", W=ptrs(p.value, off8.value))
        for name in ("cb", "xq", "out", "x", "err", "ws"):
            call(-1, b"must be 16-byte aligned", **{name: off8})
        call(-1, b"idx must be 8-byte aligned", idx=off4)
        call(-1, b"flags_out must be 4-byte aligned", flags=off2)
        call(-3, b"workspace of 256 bytes, 3072 needed", ws_bytes=256)          # 2 x (8 x 40 floats) + 8 x 16 floats
        call(-3, b"workspace of 0 bytes, 7168 needed", ws=None, out=None)      # the last layer in the workspace: 2 x (8 x 100 floats -> 3328)
        call(0, b"", n=0)                                                      # past every check, no launch
        call(0, b"", n=0, xq=None, flags=None, b=ptrs(None, None))
        call(0, b"", n=0, out=None, x=None, err=None, W=None, b=None, ws=None, ws_bytes=0)   # xq alone: no layer, no workspace
        sizes.extend([lib.lcrec_decode_tuples_workspace(8, ints(16, 40, 100), 2, ints(48, 100, 7), 3, 1),
                      lib.lcrec_decode_tuples_workspace(8, ints(16, 40, 100), 2, ints(48, 100, 7), 3, 0),
                      lib.lcrec_decode_tuples_workspace(8, ints(24, 40, 100), 2, ints(48, 100, 7), 3, 1),
                      lib.lcrec_decode_tuples_workspace(8, ints(16, 44, 100), 2, ints(48, 100, 7), 3, 1),
                      lib.lcrec_decode_tuples_workspace(8, ints(16, 40, 100), 2, None, 3, 1),
                      lib.lcrec_debug_decode_tuples_workspace(8, ints(16, 40, 100), 2, ints(48, 100, 7), 3, 1, -1)])

    ec.in_thread(calls)
    for rc, want, word, text in seen:
        assert rc == want and (rc == 0 or (word in text and b"decode_tuples" in text)), (rc, want, word, text)
    assert len(seen) == 39
    assert sizes == [2 * 1280 + 512, 2 * 3328 + 512, 0, 0, 0, 0]


def test_the_binding_refuses_what_is_not_on_a_device():
    """... before the library is called: no last-error text is left in this thread."""
    import lcrec_amd
    idx, cb = torch.zeros((4, 1), dtype=torch.int64), torch.zeros((48, 16))
    with pytest.raises(lcrec_amd.LcrecError, match="HIP device"):
        lcrec_amd.ops.decode_tuples(idx, cb, [48], [torch.zeros((8, 16))], [None])
    assert lcrec_amd._lib.load().lcrec_last_error() == b""


# ---- the reference alone, on every row of the case table -----------------------------------------------------------------------
@pytest.mark.parametrize("row", dc.rows(), ids=dc.row_id)
def test_reference_on_greedy_and_random_tuples(oracle, row):
    e, ks, n, form, w = row
    _, cbs, greedy, _, rand = ac.inputs(e, ks, n)
    dims, Ws, bs, scs, shs = dc.decoder(e, form, w)
    x = dc.embeddings(n, w)
    for which, idx in (("greedy", greedy), ("random", rand)):
        ref = dc.reference(e, ks, n, form, w, which)
        assert ref["xq"].shape == (n, e) and ref["out"].shape == (n, w) and ref["err"].shape == (n,) and (ref["flags"] == 0).all()
        # rule 2 item by item: fp32 adds in level order (a plain copy for the first level)
        for i in (0, n // 2, n - 1):
            q = cbs[0][idx[i, 0]].copy()
            for l in range(1, len(ks)):
                q = (q + cbs[l][idx[i, l]]).astype(np.float32)
            assert np.array_equal(ref["xq"][i], q)
        # rules 3 and 4 against float64 on the same q: a chain of k fp32 fmas is within k * 2^-24 of the exact sum of magnitudes
        h = ref["xq"].astype(np.float64)
        for l, W in enumerate(Ws):
            mag = np.abs(h) @ np.abs(W.astype(np.float64)).T + np.abs(bs[l].astype(np.float64))
            h = h @ W.astype(np.float64).T + bs[l].astype(np.float64)
            if scs is not None and scs[l] is not None:
                mag = mag * np.abs(scs[l].astype(np.float64)) + np.abs(shs[l].astype(np.float64))
                h = h * scs[l].astype(np.float64) + shs[l].astype(np.float64)
            if l != len(Ws) - 1:
                h = np.maximum(h, 0.0)
        assert np.abs(ref["out"] - h).max() <= 64 * (max(dims) + 4) * 2.0 ** -24 * mag.max()
        d = (ref["out"] - x).astype(np.float64)
        assert np.allclose(ref["err"], (d * d).sum(1), rtol=(w + 2) * 2.0 ** -23, atol=0.0)
        assert np.allclose(ref["err_l1"], np.abs(d).sum(1), rtol=(w + 2) * 2.0 ** -23, atol=0.0)
        # one chain per row: the rows of a reference do not depend on the other rows
        some = slice(n // 3, n // 3 + 5)
        part = decode_ref(idx[some], cbs, Ws, bs, scs, shs, x[some])
        for k in ("xq", "out", "err", "err_l1"):
            assert np.array_equal(part[k], ref[k][some]), k


@pytest.mark.parametrize("e", ac.ES)
def test_sum_of_the_codes_is_the_straight_through_sum_up_to_rounding_and_not_bit_equal(oracle, e):
    """The greedy-path link.  q of the oracle's greedy tuples against the oracle's own xq (the straight-through sum): per level
    |fl(r + fl(c - r)) - c| <= 2^-24 (|c - r| + |s|), plus the roundings of the adds on either side; with M the largest magnitude among
    residuals, code rows and xq that is within L * 2^-21 * M.  And the two are NOT the same bits: 30 to 39 % of the elements
    differ (measured with these inputs on the CPU: 1235 of 4112 at e = 16, max difference 4.8e-7 against a bound of 5.8e-6; 3014 of 8224
    at e = 32, 6.0e-7 against 7.8e-6; 6357 of 16448 at e = 64, 4.8e-7 against 5.9e-6)."""
    ks, n = ac.KS_FOR_ALL_N[e], 257
    _, cbs, greedy, _, _ = ac.inputs(e, ks, n)
    rq = dc.greedy_path(e, ks, n)
    assert np.array_equal(rq["idx"], greedy)
    q, flags = gather_ref(cbs, greedy)
    M = max(np.abs(rq["resid"]).max(), max(np.abs(c).max() for c in cbs), np.abs(rq["xq"]).max())
    bound = len(ks) * 2.0 ** -21 * M
    diff = np.abs(q.astype(np.float64) - rq["xq"].astype(np.float64))
    differing = int((q != rq["xq"]).sum())
    print(e, ks, "elements differing", differing, "of", q.size, "max difference", diff.max(), "bound", bound)
    assert diff.max() <= bound and (flags == 0).all()
    if len(ks) > 1 and ks[0] > 1:
        assert differing > q.size // 8
    else:
        assert differing > 0 or len(ks) == 1


def test_reference_clamps_and_flags_out_of_range_codes(oracle):
    for L in (1, 3, ac.MAX_LEVELS):
        cbs, idx, level, K, (dims, Ws, bs, scs, shs), x = dc.out_of_range_case(L)
        ref = decode_ref(idx, cbs, Ws, bs, scs, shs, x)
        want = np.where(np.arange(len(idx)) % 4 == 3, 0, 1 << level)
        assert np.array_equal(ref["flags"], want.astype(np.uint32))
        clamped = idx.copy()
        clamped[:, level] = np.resize(np.array([0, K - 1, K - 1, min(5, K - 1)]), len(idx))
        same = decode_ref(clamped, cbs, Ws, bs, scs, shs, x)
        assert (same["flags"] == 0).all()
        for k in ("xq", "out", "err", "err_l1"):
            assert np.array_equal(ref[k], same[k]), k


def test_reference_on_nan_and_inf(oracle):
    cbs, idx, (dims, Ws, bs, scs, shs), x = dc.nan_case()
    ref = decode_ref(idx, cbs, Ws, bs, scs, shs, x)
    assert np.isnan(ref["xq"][:3, 4]).all() and int(np.isnan(ref["xq"]).sum()) == 3
    assert np.isnan(ref["err"][:4]).all() and np.isnan(ref["err_l1"][:4]).all()       # the NaN code row, and the all-NaN row of x
    assert np.isposinf(ref["err"][5]) and np.isposinf(ref["err_l1"][5])               # fma(-inf, -inf, err) = +inf; err + |-inf| = +inf
    rest = np.ones(len(idx), dtype=bool)
    rest[[0, 1, 2, 3, 5]] = False
    assert np.isfinite(ref["err"][rest]).all() and np.isfinite(ref["out"][3:]).all() and np.isnan(ref["out"][:3]).all()
    assert np.array_equal(row_error_ref(ref["out"][rest], x[rest]), ref["err"][rest])


def test_reference_on_the_looping_rows(oracle):
    for name, e, ks, n in dc.LOOPING:
        cbs, idx, (dims, Ws, bs, scs, shs), x = dc.looping_inputs(e, ks, n)
        assert dims == [16, 8] and idx.shape == (n, len(ks))
    assert dc.LOOPING[0][3] == 1024 * 256 // (16 // 4) + 65 and dc.LOOPING[1][3] == 1024 * 128 + 65


# ---- the report's arithmetic and the commands' refusals ------------------------------------------------------------------------
def f6_model(oracle):
    """(items, codebooks, pass-1 tuples, decoder weights, decoder biases, the reference's own tuples, fixture, meta) of F6"""
    held, _, _, g = fc.f6_case()
    meta = json.load(open(os.path.join(fc.GOLD, "manifest.json")))["fixtures"]["f6_generate.npz"]
    names = gi.state_dict_names(len(meta["model"]["layers"]) + 1, meta["model"]["bn"], len(meta["model"]["num_emb_list"]))
    cbs = [gi.f32(g["sd__" + n]) for n in names["codebooks"]]
    items = gi.toy_items(meta["seed"])
    enc = oracle.encode_assign(items, [g["sd__" + n + ".weight"] for n in names["encoder"]],
                               [g["sd__" + n + ".bias"] for n in names["encoder"]], cbs)
    Ws = [gi.f32(g["sd__" + n + ".weight"]) for n in names["decoder"]]
    bs = [gi.f32(g["sd__" + n + ".bias"]) for n in names["decoder"]]
    return items, cbs, enc["idx"].astype(np.int64), Ws, bs, held, g, meta


def test_report_is_a_plain_function_of_the_per_item_arrays(oracle):
    from lcrec_amd import decode_indices as di
    items, cbs, greedy, Ws, bs, held, _, meta = f6_model(oracle)
    assert Ws[0].shape[1] == 16 and Ws[-1].shape[0] == items.shape[1] == 128           # the F6 fixture holds the decoder
    mine, theirs = decode_ref(held, cbs, Ws, bs, x=items), decode_ref(greedy, cbs, Ws, bs, x=items)
    for key, loss in (("err", "mse"), ("err_l1", "l1")):
        rep = di.build_recon_report(mine[key], theirs[key], held, greedy, mine["flags"], 128, loss)
        want = recon_report_ref(mine[key], theirs[key], held, greedy, mine["flags"], 128, loss)
        assert rep["worst"] == want["worst"] and len(rep["worst"]) == 10
        for k in ("items", "in_dim", "loss_type", "moved_items", "clamped_items"):
            assert rep[k] == want[k], k
        for k in ("recon_file", "recon_greedy", "recon_added_rel"):
            assert rep[k] == pytest.approx(want[k], rel=1e-12, abs=0.0), k
        n = len(held)
        assert rep["items"] == n == 3000 and rep["clamped_items"] == 0
        assert rep["recon_file"] == pytest.approx(mine[key].astype(np.float64).sum() / (n * 128), rel=1e-12)
        assert rep["moved_items"] == int((held != greedy).any(1).sum()) > 0
        assert rep["recon_added_rel"] == pytest.approx(rep["recon_file"] / rep["recon_greedy"] - 1.0, rel=1e-9)
        added = mine[key].astype(np.float64) - theirs[key].astype(np.float64)
        assert [w["item"] for w in rep["worst"]] == sorted(range(n), key=lambda i: (-added[i], i))[:10]
        assert json.loads(json.dumps(rep)) == rep and di.summary(rep)
    # the file's own tuples as "greedy": nothing moved, nothing added
    rep0 = di.build_recon_report(mine["err"], mine["err"], held, held, mine["flags"], 128, "mse")
    assert rep0["moved_items"] == 0 and rep0["recon_added_rel"] == 0.0 and [w["item"] for w in rep0["worst"]] == list(range(10))
    empty = di.build_recon_report(np.zeros(0, np.float32), np.zeros(0, np.float32), held[:0], held[:0], np.zeros(0, np.int32), 128, "mse")
    assert empty["items"] == 0 and empty["worst"] == [] and empty["recon_file"] == 0.0


def test_commands_refuse_what_they_cannot_do(tmp_path, monkeypatch):
    from lcrec_amd import audit_indices as ai
    from lcrec_amd import decode_indices as di
    from lcrec_amd import generate_indices as gen
    a = di.parse_args(["--ckpt_path", "c.pth", "--index_file", "x.json", "--output", "r.npy", "--report", "r.json"])
    assert (a.index_file, a.output, a.report, a.device, a.no_data, a.data_path) == ("x.json", "r.npy", "r.json", "cuda:0", False, None)
    assert di.parse_args(["--ckpt_path", "c.pth", "--index_file", "x.json", "--no_data"]).no_data is True
    base = ["--ckpt_path", "c.pth", "--index_file", "x.json"]
    assert ai.parse_args(base).recon is False and ai.parse_args(base + ["--recon"]).recon is True
    no, out = str(tmp_path / "no.pth"), str(tmp_path / "out.json")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="single process"):                            # before the checkpoint is opened
        di.decode(no, out, device="cpu")
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(FileNotFoundError):
        di.decode(no, out, device="cpu")
    npy = str(tmp_path / "items.npy")
    np.save(npy, np.zeros((5, 24), dtype=np.float32))
    args = argparse.Namespace(data_path=npy, num_emb_list=[8, 8], e_dim=16, layers=[32], dropout_prob=0.0, bn=False, loss_type="mse",
                              quant_loss_weight=1.0, kmeans_init=False, kmeans_iters=10, sk_epsilons=[0.0, 0.0], sk_iters=50)
    model = gen.build_model_from_args(args, 24)
    ckpt = str(tmp_path / "toy.pth")
    torch.save({"args": args, "epoch": 0, "state_dict": model.state_dict(), "optimizer": {}}, ckpt, pickle_protocol=4)
    index = str(tmp_path / "four.index.json")
    gen.dump_index_json(np.zeros((4, 2), dtype=np.int64), index)
    with pytest.raises(ValueError, match=r"holds 4 items but the data file 5 rows"):    # both counts, before the device is touched
        di.decode(ckpt, index, device="cuda:0")
