"""MI355X: the beam-search quantiser (lcrec_rq_beam, ops.rq_beam, RQVAE.get_indices_beam, generate(beam=W)).

Every per-item comparison is exact: the kernel and tests/beam_ref.py evaluate the same fp32 fma chains and every tie is defined, so
tuples, score, err and resid must agree bit for bit (a NaN, which only err and resid can hold, must be a NaN on both sides).  The
float statistics of generate() are compared to float64 aggregates of the reference arrays at 1e-12 relative: fp64 rounding, 1.1e-16,
times at most a few thousand summands, whatever the order of summation; its integers exactly.
Outputs sit between guard bands and are pre-filled with garbage; the workspace has exactly the size the query states and is filled
with NaNs; every call is made a second time on the then dirty buffers and workspace."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

import beam_cases as bc
import finish_cases as fc
import golden_inputs as gi
from audit_ref import audit_ref
from beam_ref import beam_ref, choose_ref, stats_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64                                                  # elements on either side of every output
BAND, GARBAGE = 0x5A5A5A5A, 0x7FC12345                      # (as int32; GARBAGE is a NaN as a float and a large code as an integer)
REL = 1e-12
NAMES = ("tuples", "score", "err", "resid")


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
    """The outputs of one shape as views into larger buffers: GUARD elements of BAND, the output filled with GARBAGE, GUARD of BAND."""

    def __init__(self, n, W, L, e, names=NAMES):
        sizes = {"tuples": (torch.int64, n * W * L), "score": (torch.float32, n * W), "err": (torch.float32, n * W),
                 "resid": (torch.float32, n * W * e)}
        self.shape = {"tuples": (n, W, L), "score": (n, W), "err": (n, W), "resid": (n, W, e)}
        self.raw, self.into, self.need = {}, {}, {}
        for name in names:
            dtype, need = sizes[name]
            raw_t = torch.int64 if dtype == torch.int64 else torch.int32
            raw = torch.full((GUARD + need + GUARD,), BAND, dtype=raw_t, device=DEV)
            raw[GUARD:GUARD + need] = GARBAGE
            self.raw[name], self.need[name] = raw, need
            self.into[name] = raw[GUARD:].view(dtype)        # larger than the call needs: the far band lies inside it

    def result(self):
        out = {}
        for name, raw in self.raw.items():
            need = self.need[name]
            assert bool((raw[:GUARD] == BAND).all()) and bool((raw[GUARD + need:] == BAND).all()), f"{name}: written outside its rows"
            out[name] = self.into[name][:need].cpu().numpy().reshape(self.shape[name]).copy()
        return out


def run(hip, z, cbs, W, names=NAMES):
    """ops.rq_beam_into guarded buffers with an exactly sized, NaN-filled workspace, twice; the second call, on the dirty buffers and
    workspace, must give the first's bits.  -> dict of numpy arrays"""
    n, e = z.shape
    flat, ks = hip.ops.flatten_codebooks([dev(c) for c in cbs])
    zd = dev(z)
    lib = hip._lib.load()
    need = lib.lcrec_rq_beam_workspace(n, e, hip.ops._ints(ks), len(ks), W)
    assert (need == 0) == (len(ks) == 1)
    raw = torch.full((GUARD + need // 4 + GUARD,), BAND, dtype=torch.int32, device=DEV)
    raw[GUARD:GUARD + need // 4] = GARBAGE
    ws = raw[GUARD:GUARD + need // 4].view(torch.uint8)
    assert ws.numel() == need and ws.data_ptr() % 16 == 0
    g = Guarded(n, W, len(ks), e, names)
    hip.ops.rq_beam_into(zd, flat, ks, W, g.into, workspace=ws)
    first = g.result()
    hip.ops.rq_beam_into(zd, flat, ks, W, g.into, workspace=ws)
    second = g.result()
    assert bool((raw[:GUARD] == BAND).all()) and bool((raw[GUARD + need // 4:] == BAND).all()), "written outside the workspace"
    for name in first:
        assert same_bits(second[name], first[name]), f"{name}: the second call on the dirty buffers differs"
    return first


def check(got, want, what=""):
    for name in got:
        w = want[name]
        if not same_bits(got[name], w):
            bad = np.flatnonzero((np.asarray(got[name]).reshape(len(w), -1) != np.asarray(w).reshape(len(w), -1)).any(1))
            raise AssertionError((what, name, bad[:8], np.asarray(got[name])[bad[:4]], np.asarray(w)[bad[:4]]))


# ---- the grid of shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", bc.shapes(), ids=bc.shape_id)
def test_kernel_matches_the_rule(hip, oracle, row):
    e, ks, W, n = row
    z, cbs, greedy = bc.inputs(e, ks, n)
    got = run(hip, z, cbs, W)
    check(got, bc.reference(e, ks, W, n), row)
    if W == 1:
        assert np.array_equal(got["tuples"][:, 0], greedy)


@pytest.mark.parametrize("row", bc.LOOPING, ids=bc.shape_id)
def test_item_loop_makes_more_than_one_trip(hip, oracle, row):
    """More items than the grid covers at once (bc.LOOPING says why these sizes): the second trip of the item loop, its stride and the
    tail of the last trip."""
    e, ks, W, n = row
    z, cbs, _ = bc.inputs(e, ks, n)
    check(run(hip, z, cbs, W), bc.reference(e, ks, W, n), (row, "looping"))


def _admits(hip, e, K, W):
    """whether lcrec_rq_beam takes a lone level of K codes: a call at n = 0, past every check and launching nothing.  (The library
    itself is called: the binding never passes an empty tensor on.)"""
    import ctypes
    import extend_cases as ec
    lib = hip._lib.load()
    p = ctypes.c_void_p(torch.zeros(64, device=DEV).data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        hip._lib.check(lib.lcrec_rq_beam(p, 0, e, p, hip.ops._ints([K]), 1, W, p, p, p, p, None, 0, stream), "lcrec_rq_beam")
    try:
        ec.in_thread(call)                                                           # (the last-error text stays in that thread)
        return True
    except hip.LcrecError as refusal:
        assert f"level 0 (K={K}, e={e}) does not fit" in str(refusal), str(refusal)
        return False


@pytest.mark.parametrize("e", bc.ES)
def test_the_largest_level_of_the_table_is_the_largest_the_entry_admits(hip, e):
    """audit_cases.LARGEST, derived from the LDS formula, against the entry itself at the widest beam: K is admitted, K + 1 refused as
    not fitting (the width plays no part: the narrowest beam draws the same line)."""
    import audit_cases as ac
    found = ac.largest_admitted(lambda K: _admits(hip, e, K, 8))
    print("rq_beam e", e, "largest admitted K", found, "(derived:", ac.LARGEST[e], ")")
    assert found == ac.LARGEST[e] == ac.largest_level(e) and not _admits(hip, e, found + 1, 8)
    assert _admits(hip, e, found, 1) and not _admits(hip, e, found + 1, 1)
    assert all((e, (found,), W, bc.N_FOR_ALL_KS) in bc.shapes() for W in bc.WS_LARGEST)   # ... and the grid above runs it


def test_exact_ties_go_by_parent_then_code(hip, oracle):
    z, cbs = bc.tie_case()
    got = run(hip, z, cbs, 4)
    check(got, beam_ref(z, cbs, 4), "ties")
    for i in range(4):
        assert got["tuples"][i].tolist() == bc.TIE_BEAMS_OF_ROW_7


@pytest.mark.parametrize("W", [1, 2, 8])
def test_nan_and_inf_count_as_plus_infinity(hip, oracle, W):
    z, cbs = bc.nan_case()
    got = run(hip, z, cbs, W)
    check(got, beam_ref(z, cbs, W), ("nan", W))
    assert not np.isnan(got["score"]).any() and got["tuples"][3].tolist() == [[0, k] for k in range(W)]


def test_every_beam_agrees_with_the_audit_on_the_device(hip, oracle):
    e, ks, W, n = 32, (48, 100, 7), 8, 257
    z, cbs, _ = bc.inputs(e, ks, n)
    flat, kl = hip.ops.flatten_codebooks([dev(c) for c in cbs])
    zd = dev(z)
    out = hip.ops.rq_beam(zd, flat, kl, W, want_resid=True)
    assert set(out) == set(NAMES) and out["tuples"].shape == (n, W, 3) and out["tuples"].dtype == torch.int64
    check({k: v.cpu().numpy() for k, v in out.items()}, bc.reference(e, ks, W, n), "allocating binding")
    for b in range(W):
        aud = hip.ops.rq_audit(zd, flat, kl, out["tuples"][:, b, :].contiguous(), want_resid=True)
        assert same_bits(aud["err"].cpu().numpy(), out["err"][:, b].cpu().numpy())
        assert same_bits(aud["d_held"][:, 2].cpu().numpy(), out["score"][:, b].cpu().numpy())
        assert same_bits(aud["resid"].cpu().numpy(), out["resid"][:, b].cpu().numpy())
    part = hip.ops.rq_beam(zd, flat, kl, W)
    assert set(part) == {"tuples", "score", "err"} and torch.equal(part["tuples"], out["tuples"])
    empty = hip.ops.rq_beam(torch.zeros((0, e), device=DEV), flat, kl, W)
    assert empty["tuples"].shape == (0, W, 3) and empty["err"].shape == (0, W)


def test_the_chunk_walk_gives_the_bits_of_one_call(hip, oracle, monkeypatch):
    e, ks, W, n = 16, (48, 100, 7), 4, 257
    z, cbs, _ = bc.inputs(e, ks, n)
    flat, kl = hip.ops.flatten_codebooks([dev(c) for c in cbs])
    monkeypatch.setattr(hip.ops, "BEAM_WORKSPACE_BOUND", 64 * 1024)
    rows = hip.ops.beam_chunk_rows(e, 3, W)
    assert 1 < rows < n and hip._lib.load().lcrec_rq_beam_workspace(rows, e, hip.ops._ints(kl), 3, W) <= 64 * 1024
    out = hip.ops.rq_beam(dev(z), flat, kl, W, want_resid=True)
    check({k: v.cpu().numpy() for k, v in out.items()}, bc.reference(e, ks, W, n), "chunked")


def test_refusals_launch_nothing_and_the_call_is_traced_once(hip):
    n, e = 64, 16
    z = torch.zeros((n, e), device=DEV)
    cb = torch.zeros((48 * e,), device=DEV)
    f = hip.ops.rq_beam
    hip.ops.trace_enable(True)
    try:
        with pytest.raises(hip.LcrecError, match="e_dim=24"):
            f(torch.zeros((n, 24), device=DEV), torch.zeros((48 * 24,), device=DEV), [48], 4)
        with pytest.raises(hip.LcrecError, match=r"level 0 \(K=4096, e=64\) does not fit"):
            f(torch.zeros((n, 64), device=DEV), torch.zeros((4096 * 64,), device=DEV), [4096], 4)
        with pytest.raises(hip.LcrecError, match="width=3"):
            f(z, cb, [48], 3)
        flat = torch.zeros(n * e + 4, device=DEV)
        with pytest.raises(hip.LcrecError, match="16-byte aligned"):
            f(flat[1:1 + n * e].view(n, e), cb, [48], 4)
        with pytest.raises(hip.LcrecError):                                          # what the binding itself refuses
            f(z, cb, [48, 48], 4)
        with pytest.raises(hip.LcrecError):
            hip.ops.rq_beam_into(z, cb, [48], 4, {"score": torch.zeros(n * 4, device=DEV)})
        with pytest.raises(hip.LcrecError, match="workspace of 256 bytes"):
            out = {"tuples": torch.zeros(n * 8, dtype=torch.int64, device=DEV), "score": torch.zeros(n * 4, device=DEV),
                   "err": torch.zeros(n * 4, device=DEV)}
            hip.ops.rq_beam_into(z, torch.zeros(96 * e, device=DEV), [48, 48], 4, out,
                                 workspace=torch.zeros(256, dtype=torch.uint8, device=DEV))
        torch.cuda.synchronize()
        assert hip.ops.trace_collect() == {}
        f(z, torch.zeros((48 + 100 + 7) * e, device=DEV), [48, 100, 7], 4)
        torch.cuda.synchronize()
        traced = hip.ops.trace_collect()
        assert set(traced) == {"rq_beam"} and traced["rq_beam"][0] == 1               # one bracket per call, whatever L
    finally:
        hip.ops.trace_enable(False)


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
    return ckpt, args, sd


_f6 = {}


def _f6_model(oracle):
    """(latents, codebooks, pass-1 greedy tuples, their audit_ref, the fixture, its manifest entry) of the F6 model on the oracle, once"""
    if not _f6:
        g = fc.f6_case()[3]
        meta = json.load(open(os.path.join(fc.GOLD, "manifest.json")))["fixtures"]["f6_generate.npz"]
        names = gi.state_dict_names(len(meta["model"]["layers"]) + 1, meta["model"]["bn"], len(meta["model"]["num_emb_list"]))
        cbs = [gi.f32(g["sd__" + n]) for n in names["codebooks"]]
        enc = oracle.encode_assign(gi.toy_items(meta["seed"]), [g["sd__" + n + ".weight"] for n in names["encoder"]],
                                   [g["sd__" + n + ".bias"] for n in names["encoder"]], cbs)
        greedy = enc["idx"].astype(np.int64)
        _f6["model"] = (enc["latent"], cbs, greedy, audit_ref(enc["latent"], cbs, greedy), g, meta)
    return _f6["model"]


def _f6_rqvae(hip, tmp_path, g, meta):
    from lcrec_amd import generate_indices as gen
    ckpt, args, sd = _checkpoint(tmp_path, g, meta)
    model = gen.build_model_from_args(args, gi.toy_items(meta["seed"]).shape[1])
    model.load_state_dict(sd)
    return ckpt, model.to(DEV).eval()


def test_get_indices_beam_width_1_is_get_indices_and_width_4_follows_the_rule(hip, oracle, tmp_path):
    latent, cbs, greedy, aud, g, meta = _f6_model(oracle)
    _, model = _f6_rqvae(hip, tmp_path, g, meta)
    xs = dev(gi.toy_items(meta["seed"]))
    plain = model.get_indices(xs)
    assert np.array_equal(plain.cpu().numpy(), greedy)
    one = model.get_indices_beam(xs, 1)
    assert one.dtype == torch.int64 and torch.equal(one, plain)
    chosen, beams = model.get_indices_beam(xs, 4, return_all=True)
    ref = beam_ref(latent, cbs, 4)
    check({k: beams[k].cpu().numpy() for k in ("tuples", "score", "err")}, ref, "F6 beams")
    want, err_c, keep = choose_ref(ref, greedy, aud["err"])
    assert np.array_equal(chosen.cpu().numpy(), want) and torch.equal(model.get_indices_beam(xs, 4), chosen)
    print("F6, width 4:", stats_ref(want, err_c, greedy, aud["err"], keep, 4))
    assert (err_c <= aud["err"]).all()
    with pytest.raises(ValueError, match="width=3"):
        model.get_indices_beam(xs, 3)
    model.train()
    with pytest.raises(hip.LcrecError, match="eval mode"):
        model.get_indices_beam(xs, 4)


def test_generate_with_beam_finish_and_audit(hip, oracle, tmp_path):
    from lcrec_amd import generate_indices as gen
    latent, cbs, greedy, aud, g, meta = _f6_model(oracle)
    ckpt, _, _ = _checkpoint(tmp_path, g, meta)
    ks = [c.shape[0] for c in cbs]
    L = len(ks)
    out = str(tmp_path / "Beam.index.json")
    stats = gen.generate(ckpt, out, device=DEV, verbose=False, finish="nearest_free", audit=True, beam=4)
    held = gen.load_index_json(out, ks)                                              # the file parses
    assert held.shape == greedy.shape
    ref = beam_ref(latent, cbs, 4)
    chosen, err_c, keep = choose_ref(ref, greedy, aud["err"])
    want = stats_ref(chosen, err_c, greedy, aud["err"], keep, 4)
    print({k: stats[k] for k in want}, want)
    for key, w in want.items():
        if isinstance(w, float):
            assert stats[key] == pytest.approx(w, rel=REL, abs=0.0), key
        else:
            assert stats[key] == w, key
    assert stats["beam_err_ratio"] <= 1.0 and stats["beam_changed"] > 0
    # the rounds and the finishing pass only ever touch the last level: the chosen prefixes are in the file
    assert np.array_equal(held[:, :L - 1], chosen[:, :L - 1]) and stats["collision_rate"] == stats["audit"]["collision_rate"]
    assert stats["finish_unresolved"] > 0 or stats["collision_rate"] == 0.0
    # the report's greedy side stays pass 1's greedy tuples; its file side is the file
    rep = stats["audit"]
    mine = audit_ref(latent, cbs, held)
    assert rep["err_greedy_mean"] == pytest.approx(aud["err"].astype(np.float64).sum() / len(held), rel=REL)
    assert rep["err_file_mean"] == pytest.approx(mine["err"].astype(np.float64).sum() / len(held), rel=REL)
    assert rep["greedy_items"] == int((mine["rank"] == 0).all(1).sum())
    # --beam 1 is the path without the flag: the same statistics, the same bytes
    one_file, plain_file = str(tmp_path / "One.index.json"), str(tmp_path / "Plain.index.json")
    one = gen.generate(ckpt, one_file, device=DEV, verbose=False, finish="nearest_free", audit=True, beam=1)
    plain = gen.generate(ckpt, plain_file, device=DEV, verbose=False, finish="nearest_free", audit=True)
    assert one == plain and "beam_width" not in plain
    assert open(one_file, "rb").read() == open(plain_file, "rb").read()
    assert open(out, "rb").read() != open(plain_file, "rb").read()


def test_generate_with_beam_and_spill_uses_the_chosen_tuples_residuals(hip, oracle, tmp_path):
    """assign_all(beam=4, want_prev=True): the residuals entering levels L-1 and L-2 are those of the CHOSEN tuples."""
    from lcrec_amd import generate_indices as gen
    latent, cbs, greedy, aud, g, meta = _f6_model(oracle)
    _, model = _f6_rqvae(hip, tmp_path, g, meta)
    info = {}
    idx, last, ks, prev = gen.assign_all(model, dev(gi.toy_items(meta["seed"])), chunk_rows=1024, want_prev=True, beam=4, beam_info=info)
    chosen, err_c, keep = choose_ref(beam_ref(latent, cbs, 4), greedy, aud["err"])
    L = len(ks)
    assert np.array_equal(idx.cpu().numpy(), chosen) and np.array_equal(torch.cat(info["greedy"]).cpu().numpy(), greedy)
    assert same_bits(last.cpu().numpy(), audit_ref(latent, cbs[:L - 1], chosen[:, :L - 1])["resid"])
    assert same_bits(prev.cpu().numpy(), audit_ref(latent, cbs[:L - 2], chosen[:, :L - 2])["resid"] if L > 2 else latent)
    assert info["kept_greedy"] == int(keep.sum()) and info["changed"] == int((chosen != greedy).any(1).sum())
