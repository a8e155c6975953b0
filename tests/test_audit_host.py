"""CPU: the host side of the index audit -- the lcrec_rq_audit entry (declared, exported, bound; its argument checks return before any
launch), the numpy statement of its rule (tests/audit_ref.py) on every row of the case table and against the finishing pass's own
reference, the report's arithmetic, and the refusals of the two commands."""
import argparse
import ctypes
import os
import re
import subprocess
import threading
import types

import numpy as np
import pytest
import torch

import audit_cases as ac
import extend_cases as ec
from audit_ref import audit_ref, first_divergence
from finish_ref import finish_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_audit_entries():
    import lcrec_amd
    header = open(os.path.join(ROOT, "include", "lcrec.h")).read()
    assert "#define LCREC_ABI_VERSION 3" in header
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(lcrec_[a-z_0-9]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", lcrec_amd._lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (lcrec_[a-z_0-9]+)", out))
    lib = lcrec_amd._lib.load()
    for name in ("lcrec_rq_audit", "lcrec_rq_audit_workspace"):
        assert name in declared and name in exported and name in lcrec_amd._lib.EXPORTS and hasattr(lib, name)
    assert lib.lcrec_rq_audit.argtypes[6:8] == [ctypes.c_void_p, ctypes.c_int64] and len(lib.lcrec_rq_audit.argtypes) == 18
    assert lib.lcrec_rq_audit_workspace.restype is ctypes.c_size_t
    assert callable(lcrec_amd.ops.rq_audit)


def test_audit_entry_reports_argument_errors_before_any_launch():
    """Each refusal names its argument and comes back before anything is enqueued, so no device is needed.  (In a thread of its own:
    the library's last-error text is per thread, and other tests expect this thread's to be empty.)"""
    import lcrec_amd
    lib = lcrec_amd._lib.load()
    seen, sizes = [], []

    def calls():
        buf = (ctypes.c_double * 64)()
        base = ctypes.cast(buf, ctypes.c_void_p).value
        p = ctypes.c_void_p((base + 15) & ~15)                       # 16-byte aligned
        off4, off8 = ctypes.c_void_p(p.value + 4), ctypes.c_void_p(p.value + 8)
        ints = lambda *v: (ctypes.c_int * len(v))(*v)
        f = lib.lcrec_rq_audit

        def call(rc, word, z=p, n=8, e=16, cb=p, K=ints(48, 100, 7), L=3, idx=p, stride=0, dh=p, db=p, rank=p, best=p, err=p, resid=p,
                 flags=p, ws=p, ws_bytes=1 << 40):
            seen.append((f(z, n, e, cb, K, L, idx, stride, dh, db, rank, best, err, resid, flags, ws, ws_bytes, None), rc, word,
                         lib.lcrec_last_error()))

        for e in (0, 8, 24, 128):
            call(-1, b"e_dim=%d" % e, e=e)
        call(-1, b"L=0", L=0)
        call(-1, b"L=17", L=17)
        call(-1, b"n=-1", n=-1)
        call(-1, b"K is NULL", K=None)
        call(-1, b"K[1]=0", K=ints(48, 0, 7))
        call(-1, b"idx_stride=2 < L=3", stride=2)
        for name in ("z", "cb", "idx", "dh", "db", "rank", "err", "flags"):
            word = {"cb": "codebooks", "dh": "d_held_out", "db": "d_best_out", "rank": "rank_out", "err": "err_out", "flags": "flags_out"}
            call(-1, (word.get(name, name) + " is NULL").encode(), **{name: None})
        for name in ("z", "cb", "dh", "db", "err", "resid", "ws"):
            call(-1, b"must be 16-byte aligned", **{name: off8})
        call(-1, b"idx and best_out must be 8-byte aligned", idx=off4)
        call(-1, b"idx and best_out must be 8-byte aligned", best=off4)
        call(-2, b"level 1 (K=4096, e=64) does not fit", K=ints(48, 4096, 7), e=64)    # lcrec_rq_assign refuses it too
        call(-2, b"level 3 (K=577, e=64) does not fit", K=ints(256, 256, 256, 577), L=4, e=64)
        call(-3, b"workspace of 256 bytes, 512 needed", ws_bytes=256)
        call(-3, b"workspace of 0 bytes, 512 needed", ws=None)
        call(0, b"", K=ints(256, 256, 256, 576), L=4, e=64, n=0)                      # the largest level: past every check, no launch
        call(0, b"", n=0, best=None, resid=None)
        sizes.extend([lib.lcrec_rq_audit_workspace(8, 16, ints(48, 100, 7), 3), lib.lcrec_rq_audit_workspace(1000, 64, ints(300), 1),
                      lib.lcrec_rq_audit_workspace(1000, 32, ints(48, 100, 7), 3), lib.lcrec_rq_audit_workspace(8, 24, ints(48), 1)])

    worker = threading.Thread(target=calls)
    worker.start()
    worker.join()
    assert len(seen) == 33
    for rc, want, word, text in seen:
        assert rc == want and (rc == 0 or (word in text and b"rq_audit" in text)), (rc, want, word, text)
    assert sizes == [512, 0, 128000, 0]


@pytest.mark.parametrize("e", ac.ES)
def test_the_tables_largest_level_follows_from_the_lds_formula_and_the_entry_draws_the_same_line(e):
    """ac.LARGEST against its own derivation and against the entry's admission check (calls at n = 0: nothing is launched, so no
    device is needed); the kernel's dynamic LDS at that level, K * (4 e + 20) bytes, is within the CU's 160 KB."""
    import lcrec_amd
    lib = lcrec_amd._lib.load()
    buf = (ctypes.c_double * 8)()
    p = ctypes.c_void_p((ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15)

    def admits(K):
        def call():
            rc = lib.lcrec_rq_audit(p, 0, e, p, (ctypes.c_int * 1)(K), 1, p, 0, p, p, p, p, p, p, p, None, 0, None)
            return rc, lib.lcrec_last_error()
        rc, text = ec.in_thread(call)
        assert rc == 0 or (rc == -2 and b"level 0 (K=%d, e=%d) does not fit" % (K, e) in text), (rc, text)
        return rc == 0

    K = ac.LARGEST[e]
    assert ac.largest_level(e) == K == ac.largest_admitted(admits) and K % 32 == 0
    assert K * (4 * e + 20) == {16: 161280, 32: 161024, 64: 158976}[e] <= ac.LDS_PER_CU
    assert (e, (K,), ac.N_FOR_ALL_KS) in ac.shapes() and (ac.DEEP_E, ac.KS_DEEP, ac.N_FOR_ALL_KS) in ac.shapes()
    assert len(ac.KS_DEEP) == ac.MAX_LEVELS == lcrec_amd._lib.MAX_LEVELS


def test_the_binding_refuses_what_is_not_on_a_device():
    """... before the library is called: no last-error text is left in this thread."""
    import lcrec_amd
    z, cb = torch.zeros((4, 16)), torch.zeros((48, 16))
    with pytest.raises(lcrec_amd.LcrecError, match="HIP device"):
        lcrec_amd.ops.rq_audit(z, cb, [48], torch.zeros((4, 1), dtype=torch.int64))


# ---- the reference alone, on every row of the case table -----------------------------------------------------------------------
@pytest.mark.parametrize("row", ac.shapes(), ids=ac.shape_id)
def test_reference_on_greedy_and_random_tuples(oracle, row):
    e, ks, n = row
    z, cbs, greedy, resid, rand = ac.inputs(e, ks, n)
    ref = ac.reference(e, ks, n, "greedy")
    assert (ref["rank"] == 0).all() and np.array_equal(ref["d_held"], ref["d_best"]) and np.array_equal(ref["best"], greedy)
    assert np.array_equal(ref["resid"], resid[len(ks)]) and (ref["flags"] == 0).all()
    assert np.array_equal(ref["err"], oracle.distances(resid[len(ks)], np.zeros((1, e), np.float32))[:, 0])
    rnd = ac.reference(e, ks, n, "random")
    assert (rnd["rank"] >= 0).all() and (rnd["rank"] < np.asarray(ks)[None, :]).all() and (rnd["flags"] == 0).all()
    assert np.array_equal(rnd["rank"] == 0, rand == rnd["best"])                     # rank 0 <=> held == best
    assert (rnd["d_held"] >= rnd["d_best"]).all()
    assert np.array_equal(rnd["best"][:, 0], greedy[:, 0])                           # level 0 sees the same residual whatever is held


@pytest.mark.parametrize("e", ac.ES)
@pytest.mark.parametrize("ks", ac.KS)
def test_random_tuples_reach_the_far_end_of_the_ranking(oracle, e, ks):
    """At n = 321 uniformly random tuples reach rank >= K / 2 at every level with K >= 48 (measured with the rule: K - 3 or more)."""
    rnd = ac.reference(e, ks, ac.N_RANK_SPREAD, "random")
    for l, K in enumerate(ks):
        if K >= 48:
            assert rnd["rank"][:, l].max() >= K // 2, (l, K, rnd["rank"][:, l].max())


def test_reference_on_exact_ties(oracle):
    z, cbs, idx = ac.tie_case()
    ref = audit_ref(z, cbs, idx)
    assert ref["rank"][:4, 0].tolist() == [2, 2, 2, 2] and ref["best"][:4, 0].tolist() == [7, 7, 7, 7]
    assert (ref["d_held"][:4, 0] == 0).all() and (ref["d_best"][:4, 0] == 0).all()
    assert (ref["rank"][:, 0] >= 2).all()                                            # rows 7 and 40 always precede 41 on a tie


@pytest.mark.parametrize("L", [1, 3, ac.MAX_LEVELS])
def test_reference_clamps_and_flags_out_of_range_codes(oracle, L):
    z, cbs, idx, level, K = ac.out_of_range_case(L)
    ref = audit_ref(z, cbs, idx)
    want = np.where(np.arange(len(z)) % 4 == 3, 0, 1 << level)
    assert np.array_equal(ref["flags"], want.astype(np.uint32))
    clamped = idx.copy()
    clamped[:, level] = np.resize(np.array([0, K - 1, K - 1, min(5, K - 1)]), len(z))
    same = audit_ref(z, cbs, clamped)
    for k in ("d_held", "d_best", "rank", "best", "err", "resid"):
        assert np.array_equal(ref[k], same[k]), k                                    # the residual followed the clamped code


def test_reference_on_nan_and_inf(oracle):
    z, cbs, idx = ac.nan_case()
    ref = audit_ref(z, cbs, idx)
    assert not np.isnan(ref["d_held"]).any() and not np.isnan(ref["d_best"]).any()
    assert np.isinf(ref["d_held"][:3, 0]).all() and (ref["rank"][:3, 0] == 47).all()  # the NaN row: +inf, behind every finite code
    assert (ref["best"][3] == 0).all() and np.array_equal(ref["rank"][3], idx[3]) and np.isinf(ref["d_best"][3]).all()
    assert (ref["best"][:3, 1] == 0).all() and np.array_equal(ref["rank"][:3, 1], idx[:3, 1])   # ... and their residual is NaN after it
    assert (ref["best"][5] == 0).all() and np.array_equal(ref["rank"][5], idx[5])


def test_finishing_pass_moves_show_at_the_last_level_only(oracle):
    """The oracle's greedy tuples at ks = [4, 48] with more items per bucket than distinct nearest codes; finish_ref; then every
    mover that moved has last-level rank >= 1 and rank 0 before it, everybody else rank 0 throughout."""
    z, cbs, greedy, resid = ac.collide_case()
    new, movers, unresolved = finish_ref(greedy, resid[1], cbs[1])
    moved = [i for i in movers if new[i, 1] != greedy[i, 1]]
    assert len(moved) == len(movers) - unresolved and len(moved) > 20
    ref = audit_ref(z, cbs, new)
    assert (ref["rank"][moved, 1] >= 1).all() and (ref["rank"][moved, 0] == 0).all()
    others = np.ones(len(z), dtype=bool)
    others[moved] = False
    assert (ref["rank"][others] == 0).all()
    assert first_divergence(ref["rank"]) == [0, len(moved)]


# ---- the report's arithmetic and the commands' refusals ------------------------------------------------------------------------
def test_report_is_a_plain_function_of_the_per_item_arrays(oracle):
    from lcrec_amd import audit_indices as ai
    e, ks, n = 32, (48, 100, 7), 257
    z, cbs, greedy, _, rand = ac.inputs(e, ks, n)
    held = greedy.copy()
    held[::3] = rand[::3]
    held[1] = held[0]                                                                  # one colliding pair
    mine, theirs = audit_ref(z, cbs, held), ac.reference(e, ks, n, "greedy")
    per = {"rank": mine["rank"], "d_held": mine["d_held"], "d_best": mine["d_best"], "flags": mine["flags"].astype(np.int32),
           "err_file": mine["err"], "err_greedy": theirs["err"]}
    neartie = np.zeros(n, dtype=np.int32)
    off = mine["rank"] > 0
    early = np.flatnonzero(off[:, 0])
    neartie[early[:5]] = 1                                                             # five early leavers are near-ties of level 0
    neartie[early[5]] = 2                                                              # ... one is a near-tie of ANOTHER level: no excuse
    unique = len({tuple(r) for r in held.tolist()})
    rep = ai.build_report(per, ks, held, greedy, neartie, unique, 2)
    assert (rep["items"], rep["levels"], rep["codes"]) == (n, 3, [48, 100, 7])
    assert rep["distinct_tuples"] == unique and rep["colliding_items"] == n - unique >= 1 and rep["max_conflicts"] == 2
    assert rep["collision_rate"] == (n - unique) / n and rep["clamped_items"] == 0
    assert rep["first_divergence"] == first_divergence(mine["rank"]) and sum(rep["first_divergence"]) == n - rep["greedy_items"]
    assert rep["early_divergence"] == rep["first_divergence"][0] == len(early) and rep["early_divergence_neartie"] == 5
    rank = mine["rank"].astype(np.float64)
    diff = mine["err"].astype(np.float64) - theirs["err"].astype(np.float64)
    for l in range(3):
        assert rep["rank0_items"][l] == int((mine["rank"][:, l] == 0).sum()) and rep["rank_max"][l] == int(mine["rank"][:, l].max())
        assert rep["rank_mean"][l] == pytest.approx(rank[:, l].sum() / n, rel=1e-12)
        regret = (mine["d_held"][:, l].astype(np.float64) - mine["d_best"][:, l].astype(np.float64)).sum() / n
        assert rep["regret_mean"][l] == pytest.approx(regret, rel=1e-12)
        assert rep["codes_used"][l] == len(set(held[:, l].tolist()))
    assert rep["err_file_mean"] == pytest.approx(mine["err"].astype(np.float64).sum() / n, rel=1e-12)
    assert rep["err_greedy_mean"] == pytest.approx(theirs["err"].astype(np.float64).sum() / n, rel=1e-12)
    assert rep["err_added_mean_diverged"] == pytest.approx(diff[off.any(1)].sum() / off.any(1).sum(), rel=1e-12)
    order = sorted(range(n), key=lambda i: (-diff[i], i))[:10]
    assert [w["item"] for w in rep["worst"]] == order
    w = rep["worst"][0]
    assert w["tuple"] == held[order[0]].tolist() and w["greedy_tuple"] == greedy[order[0]].tolist()
    assert w["ranks"] == mine["rank"][order[0]].tolist() and w["err_file"] == float(mine["err"][order[0]])
    assert ai.summary(rep) and all(isinstance(line, str) for line in ai.summary(rep))
    # all greedy: nothing diverges, the added error is 0.0
    per0 = {"rank": theirs["rank"], "d_held": theirs["d_held"], "d_best": theirs["d_best"], "flags": theirs["flags"].astype(np.int32),
            "err_file": theirs["err"], "err_greedy": theirs["err"]}
    rep0 = ai.build_report(per0, ks, greedy, greedy, neartie, n, 1)
    assert rep0["greedy_items"] == n and rep0["first_divergence"] == [0, 0, 0] and rep0["err_added_mean_diverged"] == 0.0
    assert rep0["early_divergence"] == 0 and rep0["regret_mean"] == [0.0, 0.0, 0.0]


def test_the_warning_is_a_condition_not_a_threshold(caplog):
    from lcrec_amd import audit_indices as ai
    with caplog.at_level("WARNING", logger=ai.log.name):
        assert ai.warn_if_foreign({"early_divergence": 7, "early_divergence_neartie": 7}) == 0
        assert not caplog.records
        assert ai.warn_if_foreign({"early_divergence": 7, "early_divergence_neartie": 6}) == 1
    assert "1 items leave the model's own path before the last two levels" in caplog.text
    assert "probably not written from this checkpoint" in caplog.text


def test_commands_refuse_what_they_cannot_do(tmp_path, monkeypatch):
    from lcrec_amd import audit_indices as ai
    from lcrec_amd import generate_indices as gen
    base = ["--ckpt_path", "c.pth", "--output_dir", "out"]
    assert gen.parse_args(base).audit is False and gen.parse_args(base + ["--audit"]).audit is True
    a = ai.parse_args(["--ckpt_path", "c.pth", "--index_file", "x.json", "--report", "r.json"])
    assert (a.index_file, a.report, a.device, a.trust_checkpoint) == ("x.json", "r.json", "cuda:0", False)
    no, out = str(tmp_path / "no.pth"), str(tmp_path / "out.json")
    # generate --audit: refused before the checkpoint is even opened (none of these files exist)
    with pytest.raises(ValueError, match="--audit with --recheck_neartie"):
        gen.generate(no, out, device="cpu", recheck=True, audit=True)
    ctx = types.SimpleNamespace(enabled=True, rank=0, world_size=2)
    with pytest.raises(ValueError, match="--audit under torchrun"):
        gen.generate(no, out, device="cpu", ctx=ctx, audit=True)
    with pytest.raises(FileNotFoundError):
        gen.generate(no, out, device="cpu", audit=True)
    # audit_indices under torchrun, before the checkpoint is opened
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="single process"):
        ai.audit(no, out, device="cpu")
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(FileNotFoundError):
        ai.audit(no, out, device="cpu")
    # an item count that is not the data's row count: both counts named, before the device is touched
    npy = str(tmp_path / "items.npy")
    np.save(npy, np.zeros((5, 24), dtype=np.float32))
    args = argparse.Namespace(data_path=npy, num_emb_list=[8, 8], e_dim=16, layers=[32], dropout_prob=0.0, bn=False, loss_type="mse",
                              quant_loss_weight=1.0, kmeans_init=False, kmeans_iters=10, sk_epsilons=[0.0, 0.0], sk_iters=50)
    model = gen.build_model_from_args(args, 24)
    ckpt = str(tmp_path / "toy.pth")
    torch.save({"args": args, "epoch": 0, "state_dict": model.state_dict(), "optimizer": {}}, ckpt, pickle_protocol=4)
    index = str(tmp_path / "four.index.json")
    gen.dump_index_json(np.zeros((4, 2), dtype=np.int64), index)
    with pytest.raises(ValueError, match=r"holds 4 items but the data file 5 rows"):
        ai.audit(ckpt, index, device="cuda:0")
    three = str(tmp_path / "three.index.json")
    gen.dump_index_json(np.zeros((5, 3), dtype=np.int64), three)
    with pytest.raises(ValueError):                                                    # an L that does not match: the reader's refusal
        ec.in_thread(ai.audit, ckpt, three, device="cuda:0")                           # (the strict reader leaves a last-error text)
