"""MI355X: the index audit (lcrec_rq_audit, ops.rq_audit, audit_indices.audit, generate(audit=True)).

Every per-item comparison is exact: the kernel and tests/audit_ref.py evaluate the same fp32 fma chains and every tie is defined,
so d_held, d_best, rank, best, err, resid and flags must agree bit for bit (a NaN, which only err and resid can hold, must be a NaN
on both sides).  Report floats are compared to this file's own float64 aggregates of the reference arrays at 1e-12 relative: fp64
rounding, 1.1e-16, times at most a few thousand summands, whatever the order of summation; report integers exactly.
Outputs sit between guard bands and are pre-filled with garbage; every call is made twice on the then dirty buffers."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

import audit_cases as ac
import finish_cases as fc
import golden_inputs as gi
import spill_cases as sc
from audit_ref import audit_ref, report_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64                                                  # elements on either side of every output
BAND, GARBAGE = 0x5A5A5A5A, 0x7FC12345                      # (as int32; GARBAGE is a NaN as a float and a large code as an integer)
REL = 1e-12
NAMES = ("d_held", "d_best", "rank", "best", "err", "resid", "flags")


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

    def __init__(self, n, L, e, names=NAMES):
        sizes = {"d_held": (torch.float32, n * L), "d_best": (torch.float32, n * L), "rank": (torch.int32, n * L),
                 "best": (torch.int64, n * L), "err": (torch.float32, n), "resid": (torch.float32, n * e), "flags": (torch.int32, n)}
        self.shape = {"d_held": (n, L), "d_best": (n, L), "rank": (n, L), "best": (n, L), "err": (n,), "resid": (n, e), "flags": (n,)}
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


def run(hip, z, cbs, idx, names=NAMES, idx_dev=None):
    """ops.rq_audit_into guarded buffers, twice; the second call's bits must be the first's.  -> dict of numpy arrays"""
    n, e = z.shape
    flat, ks = hip.ops.flatten_codebooks([dev(c) for c in cbs])
    zd = dev(z)
    held = dev(idx) if idx_dev is None else idx_dev
    g = Guarded(n, len(ks), e, names)
    hip.ops.rq_audit_into(zd, flat, ks, held, g.into)
    first = g.result()
    hip.ops.rq_audit_into(zd, flat, ks, held, g.into)
    second = g.result()
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
@pytest.mark.parametrize("row", ac.shapes(), ids=ac.shape_id)
def test_kernel_matches_the_rule_on_greedy_and_random_tuples(hip, oracle, row):
    e, ks, n = row
    z, cbs, greedy, resid, rand = ac.inputs(e, ks, n)
    got = run(hip, z, cbs, greedy)
    check(got, ac.reference(e, ks, n, "greedy"), (row, "greedy"))
    assert (got["rank"] == 0).all() and same_bits(got["d_held"], got["d_best"]) and same_bits(got["resid"], resid[len(ks)])
    got = run(hip, z, cbs, rand)
    want = ac.reference(e, ks, n, "random")
    check(got, want, (row, "random"))
    print(row, "largest rank per level", got["rank"].max(0).tolist(), "of", list(ks))


@pytest.mark.parametrize("row", ac.LOOPING, ids=ac.shape_id)
def test_item_loop_makes_more_than_one_trip(hip, oracle, row):
    """More items than the grid covers at once (ac.LOOPING says why these sizes): the second trip of the item loop, its stride and
    the tail of the last trip, at the register-bound grid and at the LDS-bound one."""
    e, ks, n = row
    z, cbs, _, _, rand = ac.inputs(e, ks, n)
    got = run(hip, z, cbs, rand)
    check(got, ac.reference(e, ks, n, "random"), (row, "looping"))


def _admits(hip, e, K):
    """whether lcrec_rq_audit takes a lone level of K codes: a call at n = 0, past every check and launching nothing.  (The library
    itself is called: the binding never passes an empty tensor on.)"""
    import ctypes
    import extend_cases as ec
    lib = hip._lib.load()
    p = ctypes.c_void_p(torch.zeros(64, device=DEV).data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        hip._lib.check(lib.lcrec_rq_audit(p, 0, e, p, hip.ops._ints([K]), 1, p, 0, p, p, p, p, p, p, p, None, 0, stream), "lcrec_rq_audit")
    try:
        ec.in_thread(call)                                                           # (the last-error text stays in that thread)
        return True
    except hip.LcrecError as refusal:
        assert f"level 0 (K={K}, e={e}) does not fit" in str(refusal), str(refusal)
        return False


@pytest.mark.parametrize("e", ac.ES)
def test_the_largest_level_of_the_table_is_the_largest_the_entry_admits(hip, e):
    """ac.LARGEST, derived from the LDS formula, against the entry itself: K is admitted, K + 1 refused as not fitting."""
    found = ac.largest_admitted(lambda K: _admits(hip, e, K))
    print("rq_audit e", e, "largest admitted K", found, "(derived:", ac.LARGEST[e], ")")
    assert found == ac.LARGEST[e] == ac.largest_level(e) and not _admits(hip, e, found + 1)
    assert (e, (found,), ac.N_FOR_ALL_KS) in ac.shapes()                              # ... and the grid above runs it


def test_exact_ties_rank_by_code_order(hip, oracle):
    z, cbs, idx = ac.tie_case()
    got = run(hip, z, cbs, idx)
    check(got, audit_ref(z, cbs, idx), "ties")
    assert got["rank"][:4, 0].tolist() == [2, 2, 2, 2] and got["best"][:4, 0].tolist() == [7, 7, 7, 7]
    assert (got["d_held"][:4, 0] == 0).all() and (got["d_best"][:4, 0] == 0).all()


@pytest.mark.parametrize("L", [1, 3, ac.MAX_LEVELS])
def test_out_of_range_codes_are_clamped_and_flagged(hip, oracle, L):
    z, cbs, idx, level, K = ac.out_of_range_case(L)
    got = run(hip, z, cbs, idx)
    check(got, audit_ref(z, cbs, idx), ("out of range", L))
    assert np.array_equal(got["flags"], np.where(np.arange(len(z)) % 4 == 3, 0, 1 << level))
    clamped = idx.copy()
    clamped[:, level] = np.resize(np.array([0, K - 1, K - 1, min(5, K - 1)]), len(z))
    again = run(hip, z, cbs, clamped)
    for name in ("d_held", "d_best", "rank", "best", "err", "resid"):                 # the residual followed the clamped code
        assert same_bits(got[name], again[name]), name
    assert (again["flags"] == 0).all()


def test_nan_and_inf_count_as_plus_infinity(hip, oracle):
    z, cbs, idx = ac.nan_case()
    got = run(hip, z, cbs, idx)
    check(got, audit_ref(z, cbs, idx), "nan")
    assert not np.isnan(got["d_held"]).any() and not np.isnan(got["d_best"]).any()
    assert np.isinf(got["d_held"][:3, 0]).all() and (got["rank"][:3, 0] == 47).all()
    assert (got["best"][3] == 0).all() and np.array_equal(got["rank"][3], idx[3])


def test_tuples_as_columns_of_a_wider_matrix(hip, oracle):
    e, ks, n = 32, (48, 100, 7), 257
    z, cbs, greedy, _, rand = ac.inputs(e, ks, n)
    L = len(ks)
    wide = gi.rs(5200).randint(-9, 1 << 20, size=(n, L + 5)).astype(np.int64)
    wide[:, 2:2 + L] = rand
    wide_dev = dev(wide)
    got = run(hip, z, cbs, None, idx_dev=wide_dev[:, 2:2 + L])
    check(got, ac.reference(e, ks, n, "random"), "strided")
    assert np.array_equal(wide_dev.cpu().numpy(), wide)                              # idx is never written
    with pytest.raises(hip.LcrecError, match="column block"):
        hip.ops.rq_audit(dev(z), *hip.ops.flatten_codebooks([dev(c) for c in cbs]),
                         wide_dev[:, 0:2 * L:2])


def test_best_and_resid_are_optional(hip, oracle):
    e, ks, n = 16, (48, 100, 7), 65
    z, cbs, _, _, rand = ac.inputs(e, ks, n)
    full = run(hip, z, cbs, rand)
    for names in (("d_held", "d_best", "rank", "err", "flags"), ("d_held", "d_best", "rank", "err", "flags", "best"),
                  ("d_held", "d_best", "rank", "err", "flags", "resid")):
        part = run(hip, z, cbs, rand, names=names)
        assert set(part) == set(names)
        for name in names:
            assert same_bits(part[name], full[name]), (names, name)
    # ... and the tensors the binding allocates itself
    flat, kl = hip.ops.flatten_codebooks([dev(c) for c in cbs])
    out = hip.ops.rq_audit(dev(z), flat, kl, dev(rand))
    assert set(out) == {"d_held", "d_best", "rank", "err", "flags"} and out["rank"].dtype == torch.int32
    out = hip.ops.rq_audit(dev(z), flat, kl, dev(rand), want_best=True, want_resid=True)
    for name in NAMES:
        assert same_bits(out[name].cpu().numpy(), full[name]), name
    empty = hip.ops.rq_audit(torch.zeros((0, e), device=DEV), flat, kl, torch.zeros((0, 3), dtype=torch.int64, device=DEV))
    assert empty["rank"].shape == (0, 3) and empty["err"].shape == (0,)


@pytest.mark.parametrize("e,ks,n", [(32, (256, 256, 256, 256), 1000), (64, (576,), 257), (16, (48, 100, 7), 65)])
def test_the_production_quantiser_is_on_rank_zero(hip, oracle, e, ks, n):
    """ops.rq_assign on the device, then ops.rq_audit of its output: rank 0 everywhere, and the last residual bit for bit."""
    z, cbs, _, _, _ = ac.inputs(e, ks, n)
    flat, kl = hip.ops.flatten_codebooks([dev(c) for c in cbs])
    zd = dev(z)
    idx, _, _, resid = hip.ops.rq_assign(zd, flat, kl, want_resid=True)
    out = hip.ops.rq_audit(zd, flat, kl, idx, want_best=True, want_resid=True)
    assert int(out["rank"].abs().sum()) == 0 and int(out["flags"].abs().sum()) == 0
    assert torch.equal(out["best"], idx) and torch.equal(out["d_held"], out["d_best"])
    assert same_bits(out["resid"].cpu().numpy(), resid[len(ks)].cpu().numpy())


def test_refusals_launch_nothing_and_the_call_is_traced_once(hip):
    n, e = 64, 16
    z = torch.zeros((n, e), device=DEV)
    cb = torch.zeros((48 * e,), device=DEV)
    idx = torch.zeros((n, 1), dtype=torch.int64, device=DEV)
    f = hip.ops.rq_audit
    hip.ops.trace_enable(True)
    try:
        with pytest.raises(hip.LcrecError, match="e_dim=24"):
            f(torch.zeros((n, 24), device=DEV), torch.zeros((48 * 24,), device=DEV), [48], idx)
        with pytest.raises(hip.LcrecError, match=r"level 0 \(K=4096, e=64\) does not fit"):
            f(torch.zeros((n, 64), device=DEV), torch.zeros((4096 * 64,), device=DEV), [4096], idx)
        flat = torch.zeros(n * e + 4, device=DEV)
        with pytest.raises(hip.LcrecError, match="16-byte aligned"):
            f(flat[1:1 + n * e].view(n, e), cb, [48], idx)
        with pytest.raises(hip.LcrecError):                                          # what the binding itself refuses
            f(z, cb, [48, 48], idx)
        with pytest.raises(hip.LcrecError):
            f(z, cb, [48], idx.to(torch.int32))
        with pytest.raises(hip.LcrecError):
            f(z, cb, [48], idx.cpu())
        with pytest.raises(hip.LcrecError):
            hip.ops.rq_audit_into(z, cb, [48], idx, {"rank": torch.zeros(n, dtype=torch.int32, device=DEV)})
        torch.cuda.synchronize()
        assert hip.ops.trace_collect() == {}
        f(z, torch.zeros((48 + 100 + 7) * e, device=DEV), [48, 100, 7], torch.zeros((n, 3), dtype=torch.int64, device=DEV))
        torch.cuda.synchronize()
        traced = hip.ops.trace_collect()
        assert set(traced) == {"rq_audit"} and traced["rq_audit"][0] == 1              # one bracket per call, whatever L
    finally:
        hip.ops.trace_enable(False)


# ---- end to end on F6 ------------------------------------------------------------------------------------------------------------
def _checkpoint(tmp_path, g, meta, cut=None):
    npy = str(tmp_path / "Toy.emb.npy")
    np.save(npy, gi.toy_items(meta["seed"]))
    kw = {k: v for k, v in meta["model"].items() if k != "in_dim"}
    sd = {k[4:]: torch.from_numpy(g[k].copy()) for k in g.files if k.startswith("sd__")}
    if cut is not None:
        kw["num_emb_list"] = [48, 48, sc.F6_CUT]
        sd[cut[4:]] = sd[cut[4:]][:sc.F6_CUT].clone()
    args = argparse.Namespace(data_path=npy, num_workers=0, **kw)
    ckpt = str(tmp_path / "toy.pth")
    torch.save({"args": args, "epoch": 0, "best_loss": 0.0, "best_collision_rate": 0.0, "state_dict": sd, "optimizer": {}}, ckpt,
               pickle_protocol=4)
    return ckpt


_f6 = {}


def _f6_model(oracle):
    """(latents, codebooks, pass-1 tuples) of the F6 model on the oracle, once"""
    if not _f6:
        g = fc.f6_case()[3]
        meta = json.load(open(os.path.join(fc.GOLD, "manifest.json")))["fixtures"]["f6_generate.npz"]
        names = gi.state_dict_names(len(meta["model"]["layers"]) + 1, meta["model"]["bn"], len(meta["model"]["num_emb_list"]))
        cbs = [gi.f32(g["sd__" + n]) for n in names["codebooks"]]
        enc = oracle.encode_assign(gi.toy_items(meta["seed"]), [g["sd__" + n + ".weight"] for n in names["encoder"]],
                                   [g["sd__" + n + ".bias"] for n in names["encoder"]], cbs)
        _f6["model"] = (enc["latent"], cbs, enc["idx"].astype(np.int64), g, meta)
    return _f6["model"]


def _compare_report(rep, latent, cbs, held, greedy, first=0):
    ks = [c.shape[0] for c in cbs]
    mine, theirs = audit_ref(latent, cbs, held), audit_ref(latent, cbs, greedy)
    want = report_ref(mine, theirs, held, ks)
    for key, w in want.items():
        print(key, rep[key], w)
        if isinstance(w, float) or (isinstance(w, list) and w and isinstance(w[0], float)):
            assert rep[key] == pytest.approx(w, rel=REL, abs=0.0), key
        else:
            assert rep[key] == w, key
    assert 0 <= rep["early_divergence_neartie"] <= rep["early_divergence"]
    added = mine["err"].astype(np.float64) - theirs["err"].astype(np.float64)
    worst = sorted(range(len(held)), key=lambda i: (-added[i], i))[:10]
    assert [w["item"] - first for w in rep["worst"]] == worst
    for w in rep["worst"]:
        i = w["item"] - first
        assert w["tuple"] == held[i].tolist() and w["greedy_tuple"] == greedy[i].tolist() and w["ranks"] == mine["rank"][i].tolist()
        assert w["err_file"] == float(mine["err"][i]) and w["err_greedy"] == float(theirs["err"][i])


def test_generate_with_audit_reports_what_the_finishing_pass_cost(hip, oracle, tmp_path):
    from lcrec_amd import audit_indices as ai
    from lcrec_amd import generate_indices as gen
    latent, cbs, pass1, g, meta = _f6_model(oracle)
    ckpt = _checkpoint(tmp_path, g, meta)
    ks = [c.shape[0] for c in cbs]
    L = len(ks)
    out = str(tmp_path / "Toy.index.json")
    stats = gen.generate(ckpt, out, device=DEV, verbose=False, finish="nearest_free", audit=True)
    rep = stats["audit"]
    held = gen.load_index_json(out, ks)
    assert rep["items"] == 3000 and rep["colliding_items"] == 0 and rep["levels"] == L and rep["codes"] == ks
    assert rep["first_divergence"][:L - 1] == [0] * (L - 1)
    assert rep["first_divergence"][L - 1] == int((held[:, L - 1] != pass1[:, L - 1]).sum()) > 0
    assert np.array_equal(held[:, :L - 1], pass1[:, :L - 1])
    _compare_report(rep, latent, cbs, held, pass1)
    assert rep["early_divergence"] == 0 and rep["clamped_items"] == 0
    assert json.loads(json.dumps(rep)) == rep                                        # plain numbers and lists: it goes into a JSON file
    # the command on that file returns the same report
    again = ai.audit(ckpt, out, device=DEV)
    assert again == rep
    report = str(tmp_path / "r" / "report.json")
    assert ai.main(["--ckpt_path", ckpt, "--index_file", out, "--device", DEV, "--report", report]) == rep
    assert json.load(open(report)) == rep
    # without the flag: no `audit` key, the same statistics otherwise and the same bytes
    plain_file = str(tmp_path / "Plain.index.json")
    plain = gen.generate(ckpt, plain_file, device=DEV, verbose=False, finish="nearest_free")
    assert "audit" not in plain and plain == {k: v for k, v in stats.items() if k != "audit"}
    assert open(plain_file, "rb").read() == open(out, "rb").read()


def test_the_references_own_f6_file_still_collides_on_69_items(hip, oracle, tmp_path, caplog):
    from lcrec_amd import audit_indices as ai
    latent, cbs, pass1, g, meta = _f6_model(oracle)
    ckpt = _checkpoint(tmp_path, g, meta)
    ks = [c.shape[0] for c in cbs]
    path = str(tmp_path / "Ref.index.json")
    open(path, "wb").write(bytes(g["json_text"]))
    with caplog.at_level("WARNING", logger=ai.log.name):
        rep = ai.audit(ckpt, path, device=DEV)
    held = fc.f6_case()[0]
    assert rep["colliding_items"] == 69 == fc.movers_by_count(held)
    _compare_report(rep, latent, cbs, held, pass1)
    assert rep["early_divergence"] == 0 and "not written from this checkpoint" not in caplog.text
    # a file whose level-0 column is rotated by one code was not written from this checkpoint
    rotated = held.copy()
    rotated[:, 0] = (rotated[:, 0] + 1) % ks[0]
    from lcrec_amd import generate_indices as gen
    path2 = str(tmp_path / "Rotated.index.json")
    gen.dump_index_json(rotated, path2)
    with caplog.at_level("WARNING", logger=ai.log.name):
        rep2 = ai.audit(ckpt, path2, device=DEV)
    assert rep2["early_divergence"] - rep2["early_divergence_neartie"] > 0
    assert "not written from this checkpoint" in caplog.text
    assert rep2["first_divergence"] == report_ref(audit_ref(latent, cbs, rotated), audit_ref(latent, cbs, pass1), rotated, ks)["first_divergence"]


def test_generate_with_spill_and_audit_counts_the_spilled_items_one_level_up(hip, oracle, tmp_path):
    from lcrec_amd import generate_indices as gen
    f = sc.f6_cut()
    ckpt = _checkpoint(tmp_path, f["fixture"], f["meta"], cut=f["last_name"])
    ks = [48, 48, sc.F6_CUT]
    out = str(tmp_path / "Cut.index.json")
    stats = gen.generate(ckpt, out, device=DEV, verbose=False, finish="nearest_free", spill=True, audit=True)
    rep = stats["audit"]
    assert stats["spill_moved"] > 0 and rep["first_divergence"][len(ks) - 2] == stats["spill_moved"]
    assert rep["first_divergence"][0] == 0 and rep["colliding_items"] == 0 and rep["codes"] == ks
    held = gen.load_index_json(out, ks)
    _compare_report(rep, f["resid"][0], f["cbs"], held, f["idx"])                  # (the residual entering level 0 is the latent)


def test_generate_extend_with_audit_covers_the_new_rows_only(hip, oracle, tmp_path):
    """2000 F6 items indexed with --finish nearest_free are the base; --extend --audit over all 3000 reports the 1000 new rows."""
    from lcrec_amd import generate_indices as gen
    latent, cbs, pass1, g, meta = _f6_model(oracle)
    ckpt = _checkpoint(tmp_path, g, meta)
    ks = [c.shape[0] for c in cbs]
    L, n0 = len(ks), 2000
    npy0 = str(tmp_path / "Base.emb.npy")
    np.save(npy0, gi.toy_items(meta["seed"])[:n0])
    base_file, out, plain_file = (str(tmp_path / name) for name in ("Base.index.json", "All.index.json", "Plain.index.json"))
    gen.generate(ckpt, base_file, device=DEV, data_path=npy0, verbose=False, finish="nearest_free")
    stats = gen.generate(ckpt, out, device=DEV, verbose=False, extend=base_file, audit=True)
    rep = stats["audit"]
    held = gen.load_index_json(out, ks)[n0:]
    assert rep["items"] == 1000 == stats["new_items"] and rep["first_divergence"][:L - 1] == [0] * (L - 1)
    assert rep["first_divergence"][L - 1] == int((held[:, L - 1] != pass1[n0:, L - 1]).sum()) == stats["extend_moved"] > 0
    _compare_report(rep, np.ascontiguousarray(latent[n0:]), cbs, held, pass1[n0:], first=n0)
    plain = gen.generate(ckpt, plain_file, device=DEV, verbose=False, extend=base_file)
    assert "audit" not in plain and plain == {k: v for k, v in stats.items() if k != "audit"}
    assert open(plain_file, "rb").read() == open(out, "rb").read()
