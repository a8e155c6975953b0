"""CPU: the host side of --spill -- the lcrec_spill_nearest_free entry (declared, exported, bound; its argument checks return
before any launch), the CLI flag and generate()'s refusals, and the numpy statement of the rule (tests/spill_ref.py) after
finish_ref, on small cases and on the F6 model with its last codebook cut to 16 rows.
Every comparison is of integers; there is no tolerance in this file."""
import argparse
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import extend_cases as ec
import golden_inputs as gi
import spill_cases as sc
from finish_ref import colliding_items, finish_ref
from spill_ref import spill_ref, three_op

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lcrec_spill_nearest_free", "lcrec_spill_nearest_free_workspace")


def test_header_declares_and_library_exports_the_spill_entry():
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
    assert callable(lcrec_amd.ops.spill_nearest_free)
    for n in (0, 1, 256, 257, 10 ** 6):                                 # one flag per item
        assert lib.lcrec_spill_nearest_free_workspace(n) >= max(n, 1)


def test_spill_entry_reports_argument_errors_before_any_launch():
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
        f = lib.lcrec_spill_nearest_free

        def call(rc, word, idx=p, n=8, nf=2, L=3, K=ints(48, 48, 48), r2=p, r1=p, e=16, cb2=p, cb1=p, tm=p, to=p, nt=1, sm=p, so=p,
                 ns=1, counters=p, ws=p, wsb=256):
            seen.append((f(idx, n, nf, L, K, r2, r1, e, cb2, cb1, tm, to, nt, sm, so, ns, counters, ws, wsb, None), rc, word,
                         lib.lcrec_last_error()))

        call(-1, b"L=1 (2 .. 16", L=1, K=ints(48))
        call(-1, b"L=0", L=0)
        call(-1, b"L=17", L=17)
        call(-1, b"n_frozen=-1", nf=-1)
        call(-1, b"n_frozen=9 (0 .. n=8)", nf=9)
        call(-1, b"n=-1", n=-1, nf=0)
        call(-1, b"n_tuple_groups=-1", nt=-1)
        call(-1, b"n_super_buckets=-1", ns=-1)
        for e in (0, 8, 24, 128):
            call(-2, b"e_dim=%d" % e, e=e)
        call(-1, b"K[1]=0", K=ints(48, 0, 48))
        call(-1, b"K[2]=0", K=ints(48, 48, 0))
        # 256 + 256 codes at e = 64 are taken (the call goes on to its next check); a larger pair is refused with the byte count
        call(-1, b"NULL pointer", K=ints(4, 256, 256), e=64, cb1=None)
        call(-2, b"levels 1 and 2 (K=512 and K=256, e=64) need 221696 B of LDS together", K=ints(4, 512, 256), e=64)
        call(-2, b"levels 0 and 1 (K=256 and K=2048, e=16) need 232960 B of LDS together", L=2, K=ints(256, 2048))
        for name in ("r2", "r1", "cb2", "cb1"):
            call(-1, b"must be 16-byte aligned", **{name: off8})
        for name in ("idx", "tm", "to", "sm", "so", "counters"):
            call(-1, b"must be 8-byte aligned", **{name: off4})
        call(-1, b"counters_out is NULL", counters=None)
        call(-1, b"K is NULL", K=None)
        for name in ("idx", "r2", "r1", "cb2", "cb1", "tm", "to", "sm", "so"):
            call(-1, b"NULL pointer", **{name: None})
        call(-3, b"workspace of 0 bytes, 256 needed", ws=None)
        call(-3, b"workspace of 255 bytes, 256 needed", wsb=255)
        call(-3, b"workspace of 256 bytes, 512 needed", n=300, wsb=256)

    ec.in_thread(calls)
    assert len(seen) == 41
    for rc, want, word, text in seen:
        assert rc == want and word in text and b"spill_nearest_free" in text, (rc, want, word, text)


def test_lds_formula_of_the_header():
    """(K2 + K1) * (4 e + 8) + K2 * (4 ceil(K1 / 32) + 4) + 512 <= 160 KB, as include/lcrec.h states it."""
    need = lambda K2, K1, e: (K2 + K1) * (4 * e + 8) + K2 * (4 * -(-K1 // 32) + 4) + 512
    assert need(256, 256, 64) == 144896 <= 160 * 1024
    assert need(512, 256, 64) == 221696 and need(256, 2048, 16) == 232960


def test_cli_accepts_spill_and_generate_refuses_what_it_cannot_do(tmp_path):
    from lcrec_amd import generate_indices as gen
    base = ["--ckpt_path", "c.pth", "--output_dir", "out"]
    assert gen.parse_args(base).spill is False
    assert gen.parse_args(base + ["--finish", "nearest_free", "--spill"]).spill is True
    assert callable(gen.spill_collisions)
    no, out = str(tmp_path / "no.pth"), str(tmp_path / "out.json")
    # refused before the checkpoint is even opened (none of these files exist)
    with pytest.raises(ValueError, match="--finish nearest_free or --extend"):
        gen.generate(no, out, device="cpu", spill=True)
    with pytest.raises(ValueError, match="--finish nearest_free or --extend"):
        gen.generate(no, out, device="cpu", finish="none", spill=True)
    for kw in ({"finish": "nearest_free"}, {"extend": str(tmp_path / "b.json")}):
        with pytest.raises(ValueError, match="recheck_neartie"):
            gen.generate(no, out, device="cpu", recheck=True, spill=True, **kw)
        ctx = types.SimpleNamespace(enabled=True, rank=0, world_size=2)
        with pytest.raises(ValueError, match="torchrun"):
            gen.generate(no, out, device="cpu", ctx=ctx, spill=True, **kw)
    # a one-level model: known from the checkpoint's arguments, refused before the data file (which does not exist) is opened
    ckpt = str(tmp_path / "one.pth")
    args = argparse.Namespace(data_path=str(tmp_path / "no.npy"), num_emb_list=[48], e_dim=16)
    torch.save({"args": args, "epoch": 0, "state_dict": {}, "optimizer": {}}, ckpt, pickle_protocol=4)
    for kw in ({"finish": "nearest_free"}, {"extend": str(tmp_path / "b.json")}):
        with pytest.raises(ValueError, match="one level"):
            gen.generate(ckpt, out, device="cpu", spill=True, **kw)
    # ... and without the flag nothing above is looked at
    with pytest.raises(FileNotFoundError):
        gen.generate(no, out, device="cpu", finish="nearest_free")


def test_an_unsupported_level_pair_keeps_the_earlier_result(monkeypatch, caplog):
    """generate() logs a warning and leaves the statistics at zero when the library refuses the pair of levels as unsupported;
    any other refusal is raised."""
    import lcrec_amd
    from lcrec_amd import generate_indices as gen

    def refuse_with(code):
        def refuse(*args, **kw):
            err = lcrec_amd.LcrecError(f"lcrec_spill_nearest_free failed ({code}): spill_nearest_free: levels 1 and 2 ...")
            err.code = code
            raise err
        return refuse

    monkeypatch.setattr(gen, "spill_collisions", refuse_with(-2))
    stats = {}
    with caplog.at_level("WARNING"):
        gen._spill_and_log(None, None, 0, None, None, [4, 512, 256], stats)
    assert stats == {"spill_moved": 0, "spill_unresolved": 0, "spill_super_buckets": 0, "largest_super_bucket": 0}
    assert "skipped" in caplog.text and "levels 1 and 2" in caplog.text
    monkeypatch.setattr(gen, "spill_collisions", refuse_with(-1))
    with pytest.raises(lcrec_amd.LcrecError):
        gen._spill_and_log(None, None, 0, None, None, [4, 512, 256], {})


def test_assign_all_keeps_its_default_return_value():
    import inspect
    from lcrec_amd import generate_indices as gen
    sig = inspect.signature(gen.assign_all)
    assert sig.parameters["want_prev"].default is False
    assert inspect.signature(gen.generate).parameters["spill"].default is False


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def test_nothing_to_do_is_the_identity(oracle):
    """Distinct tuples; tuples shared by frozen items only; and listed groups whose members are all out of range."""
    idx, r2, r1, cb2, cb1 = sc.skewed_case(40, [8, 16], 16, seed=1)
    idx = np.stack([np.arange(40) // 8, np.arange(40) % 8], axis=1).astype(np.int64)
    new, served, unres = spill_ref(idx, 0, r2, r1, cb2, cb1)
    assert served == [] and unres == 0 and np.array_equal(new, idx)
    idx[:10] = idx[0]                                                   # ten frozen items on one tuple, nobody new on it
    new, served, unres = spill_ref(idx, 10, r2[10:], r1[10:], cb2, cb1)
    assert served == [] and unres == 0 and np.array_equal(new, idx)
    idx[:10, 1] = 99                                                    # ... and a code out of range: no holders at all
    new, served, unres = spill_ref(idx, 0, r2, r1, cb2, cb1, tuple_groups=[list(range(10)) + [-1, 40]])
    assert served == [] and unres == 0 and np.array_equal(new, idx)


@pytest.mark.parametrize("n,ks", [(90, [8, 16]), (300, [3, 8, 16]), (200, [8, 48]), (100, [100, 1]), (1200, [5, 12, 20])])
def test_after_the_finishing_pass_exactly_its_unresolved_items_are_served(oracle, n, ks):
    idx, r2, r1, cb2, cb1 = sc.skewed_case(n, ks, 16, seed=100 + n)
    L = len(ks)
    mid, movers1, left = finish_ref(idx, r1, cb1)
    assert left > 0 and colliding_items(mid) == left
    new, served, unres = spill_ref(mid, 0, r2, r1, cb2, cb1)
    # rule 1 names the finishing pass's unresolved items and nobody else: the last `left` movers it met that stayed where they were
    stayed = sorted(i for i in movers1 if mid[i, L - 1] == idx[i, L - 1])
    assert sorted(served) == stayed and len(served) == left
    sizes = np.unique(idx[:, :L - 2], axis=0, return_counts=True)[1] if L > 2 else np.array([n])
    assert unres == int(np.maximum(0, sizes - ks[-2] * ks[-1]).sum())    # by capacity, not by chance
    assert colliding_items(new) == unres
    changed = np.flatnonzero((new != mid).any(1))
    assert len(changed) == left - unres and set(changed) <= set(served)  # only movers' rows change
    assert np.array_equal(new[:, :L - 2], mid[:, :L - 2])
    moved = [i for i in served if (new[i] != mid[i]).any()]
    cells, counts = np.unique(new, axis=0, return_counts=True)
    alone = {tuple(c) for c, k in zip(cells, counts) if k == 1}
    assert all(tuple(new[i]) in alone for i in moved)                   # a moved item collides with nobody
    again = spill_ref(mid, 0, r2, r1, cb2, cb1)
    assert np.array_equal(again[0], new) and again[1] == served


def test_a_frozen_holder_makes_every_new_holder_move(oracle):
    e = 16
    r = gi.rs(5)
    cb2, cb1 = gi.f32(r.standard_normal((3, e))), gi.f32(r.standard_normal((2, e)))
    # row 0 full: cells (0,0) and (0,1) held by frozen items 0, 1; new items 2, 3 hold (0,0) too, item 3 sitting exactly on it
    idx = np.array([[0, 0], [0, 1], [0, 0], [0, 0]], dtype=np.int64)
    r2 = gi.f32(r.standard_normal((2, e)))
    r1 = three_op(r2, cb2[[0, 0]])
    r1[1] = cb1[0]
    new, served, unres = spill_ref(idx, 2, r2, r1, cb2, cb1)
    assert served == [2, 3] and unres == 0 and np.array_equal(new[:2], idx[:2])
    assert (new[2:, 0] != 0).all() and colliding_items(new) == 0
    # without the frozen holder the nearest of the three keeps the tuple
    new, served, unres = spill_ref(idx[[0, 2, 3]], 0, gi.f32(np.concatenate([r2[:1], r2])), gi.f32(np.concatenate([r1[:1], r1])), cb2, cb1)
    assert served == [0, 1] and new[2].tolist() == [0, 0]


def test_f6_with_its_last_codebook_cut_to_16_rows(oracle):
    f = sc.f6_cut()
    idx, resid, cbs = f["idx"], f["resid"], f["cbs"]
    assert [c.shape[0] for c in cbs] == [48, 48, 16]
    assert colliding_items(idx) == 2037
    mid, movers1, left = finish_ref(idx, resid[2], cbs[2])
    _, sizes = np.unique(idx[:, :2], axis=0, return_counts=True)
    over = sizes[sizes > 16]
    assert left == 235 == int((over - 16).sum()) and len(over) == 27 and sizes.max() == 41
    new, served, unres = spill_ref(mid, 0, resid[1], resid[2], cbs[1], cbs[2])
    print("F6 cut: served", len(served), "unresolved", unres, "colliding after", colliding_items(new))
    assert len(served) == 235 and unres == 0
    assert colliding_items(new) == 0
    assert np.array_equal(new[:, 0], mid[:, 0])
    assert int((new[:, 1] != mid[:, 1]).sum()) == 235 and set(np.flatnonzero(new[:, 1] != mid[:, 1])) == set(served)
    # r2 -> r1 by the three-op update reproduces the oracle's resid[2] bit for bit
    r1 = three_op(resid[1], cbs[1][idx[:, 1]])
    assert np.array_equal(r1.view(np.uint32), np.ascontiguousarray(resid[2]).view(np.uint32))
