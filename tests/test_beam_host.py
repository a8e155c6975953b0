"""CPU: the host side of the beam-search quantiser -- the lcrec_rq_beam entry (declared, exported, bound; its argument checks return
before any launch; its workspace query), the numpy statement of its rule (tests/beam_ref.py) on every row of the case table against
the oracle's greedy quantiser and the index audit's rule (tests/audit_ref.py), the chosen-tuple rule, and the refusals of --beam."""
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
import beam_cases as bc
from audit_ref import audit_ref
from beam_ref import beam_ref, choose_ref, live_counts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(got, want):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32),
                                                                                               want[~nan].view(np.uint32))


def test_header_declares_and_library_exports_the_beam_entries():
    import lcrec_amd
    header = open(os.path.join(ROOT, "include", "lcrec.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(lcrec_[a-z_0-9]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", lcrec_amd._lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (lcrec_[a-z_0-9]+)", out))
    lib = lcrec_amd._lib.load()                                                       # (loads without a device)
    for name in ("lcrec_rq_beam", "lcrec_rq_beam_workspace"):
        assert name in declared and name in exported and name in lcrec_amd._lib.EXPORTS and hasattr(lib, name)
    assert lib.lcrec_rq_beam.argtypes[4:7] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] and len(lib.lcrec_rq_beam.argtypes) == 14
    assert lib.lcrec_rq_beam_workspace.restype is ctypes.c_size_t and len(lib.lcrec_rq_beam_workspace.argtypes) == 5
    assert callable(lcrec_amd.ops.rq_beam) and callable(lcrec_amd.RQVAE.get_indices_beam)
    assert lcrec_amd.ops.BEAM_WIDTHS == (1, 2, 4, 8)


def test_beam_entry_reports_argument_errors_before_any_launch():
    """Each refusal names its argument and comes back before anything is enqueued, so no device is needed.  (In a thread of its own:
    the library's last-error text is per thread, and other tests expect this thread's to be empty.)"""
    import lcrec_amd
    lib = lcrec_amd._lib.load()
    seen, sizes = [], []

    def calls():
        buf = (ctypes.c_double * 64)()
        base = ctypes.cast(buf, ctypes.c_void_p).value
        p = ctypes.c_void_p((base + 15) & ~15)                       # 16-byte aligned
        off2, off4, off8 = (ctypes.c_void_p(p.value + o) for o in (2, 4, 8))
        ints = lambda *v: (ctypes.c_int * len(v))(*v)
        f = lib.lcrec_rq_beam

        def call(rc, word, z=p, n=8, e=16, cb=p, K=ints(48, 100, 7), L=3, W=4, tuples=p, score=p, err=p, resid=p, ws=p,
                 ws_bytes=1 << 40):
            seen.append((f(z, n, e, cb, K, L, W, tuples, score, err, resid, ws, ws_bytes, None), rc, word, lib.lcrec_last_error()))

        for e in (0, 8, 24, 128):
            call(-1, b"e_dim=%d" % e, e=e)
        for W in (0, 3, 6, 16, -1):
            call(-1, b"width=%d" % W, W=W)
        call(-1, b"L=0", L=0)
        call(-1, b"L=17", L=17)
        call(-1, b"n=-1", n=-1)
        call(-1, b"K is NULL", K=None)
        call(-1, b"K[1]=0", K=ints(48, 0, 7))
        for name in ("z", "cb", "tuples", "score", "err"):
            word = {"cb": "codebooks", "tuples": "tuples_out", "score": "score_out", "err": "err_out"}
            call(-1, (word.get(name, name) + " is NULL").encode(), **{name: None})
        for name in ("z", "cb", "resid", "ws"):
            call(-1, b"must be 16-byte aligned", **{name: off8})
        call(-1, b"tuples_out must be 8-byte aligned", tuples=off4)
        call(-1, b"score_out and err_out must be 4-byte aligned", score=off2)
        call(-1, b"score_out and err_out must be 4-byte aligned", err=off2)
        call(-2, b"level 1 (K=4096, e=64) does not fit", K=ints(48, 4096, 7), e=64)    # lcrec_rq_assign refuses it too
        call(-2, b"level 3 (K=577, e=64) does not fit", K=ints(256, 256, 256, 577), L=4, e=64)
        call(-3, b"workspace of 256 bytes, 4352 needed", ws_bytes=256)
        call(-3, b"workspace of 0 bytes, 4352 needed", ws=None)
        call(0, b"", K=ints(256, 256, 256, 576), L=4, e=64, n=0, W=8)                 # the largest level: past every check, no launch
        call(0, b"", n=0, resid=None)
        call(0, b"", n=0, K=ints(300), L=1, ws=None, ws_bytes=0)                      # one level needs no workspace
        q = lib.lcrec_rq_beam_workspace
        sizes.extend([q(8, 16, ints(48, 100, 7), 3, 4), q(1000, 64, ints(300), 1, 8), q(1000, 32, ints(48, 7), 2, 2),
                      q(1000, 64, ints(48, 100, 7), 3, 8), q(0, 16, ints(48, 100, 7), 3, 4),
                      q(8, 24, ints(48), 1, 4), q(8, 16, ints(48), 1, 3), q(8, 16, None, 1, 4), q(8, 16, ints(48), 0, 4),
                      q(-1, 16, ints(48), 1, 4), q(8, 16, ints(48, 0), 2, 4), q(8, 64, ints(48, 4096), 2, 4)])

    worker = threading.Thread(target=calls)
    worker.start()
    worker.join()
    assert len(seen) == 33
    for rc, want, word, text in seen:
        assert rc == want and (rc == 0 or (word in text and b"rq_beam" in text)), (rc, want, word, text)
    # two halves of [n][W][e] floats and (L - 1) n W links, each rounded up to 256 bytes; one half for L = 2; nothing for L = 1 or n = 0
    assert sizes[:5] == [2 * 2048 + 256, 0, 256000 + 8192, 2 * 2048000 + 64000, 0]
    assert sizes[5:] == [0] * 7                                                       # refused arguments


@pytest.mark.parametrize("e", bc.ES)
def test_the_tables_largest_level_is_where_the_entry_draws_the_line(e):
    """audit_cases.LARGEST (derived from the LDS formula there) against lcrec_rq_beam's admission check: calls at n = 0, nothing is
    launched, no device is needed.  The grid runs that level at the narrowest and the widest beam, and the 16-level quantiser."""
    import extend_cases as ec
    import lcrec_amd
    lib = lcrec_amd._lib.load()
    buf = (ctypes.c_double * 8)()
    p = ctypes.c_void_p((ctypes.cast(buf, ctypes.c_void_p).value + 15) & ~15)

    def admits(K):
        def call():
            return lib.lcrec_rq_beam(p, 0, e, p, (ctypes.c_int * 1)(K), 1, 8, p, p, p, p, None, 0, None), lib.lcrec_last_error()
        rc, text = ec.in_thread(call)
        assert rc == 0 or (rc == -2 and b"level 0 (K=%d, e=%d) does not fit" % (K, e) in text), (rc, text)
        return rc == 0

    K = ac.LARGEST[e]
    assert ac.largest_admitted(admits) == K
    assert all((e, (K,), W, bc.N_FOR_ALL_KS) in bc.shapes() for W in (1, 8))
    assert all((16, ac.KS_DEEP, W, bc.N_FOR_ALL_KS) in bc.shapes() for W in (2, 8))
    assert live_counts(ac.KS_DEEP, 8)[:5] == [2, 2, 4, 8, 8] and live_counts(ac.KS_DEEP, 8)[-1] == 8


def test_the_binding_refuses_what_is_not_on_a_device():
    """... before the library is called: no last-error text is left in this thread."""
    import lcrec_amd
    z, cb = torch.zeros((4, 16)), torch.zeros((48, 16))
    with pytest.raises(lcrec_amd.LcrecError, match="HIP device"):
        lcrec_amd.ops.rq_beam(z, cb, [48], 4)
    assert lcrec_amd.ops.beam_chunk_rows(32, 4, 8) == ((256 << 20) - 768) // (2 * 8 * 32 * 4 + 3 * 8 * 4) == 125202
    assert lcrec_amd.ops.beam_chunk_rows(64, 2, 1, bound=1) == 1                     # a single item always goes


# ---- the reference alone, on every row of the case table -----------------------------------------------------------------------
@pytest.mark.parametrize("row", bc.shapes() + list(bc.LOOPING), ids=bc.shape_id)
def test_reference_has_the_properties_the_header_states(oracle, row):
    e, ks, W, n = row
    z, cbs, greedy = bc.inputs(e, ks, n)
    ref = bc.reference(e, ks, W, n)
    L = len(ks)
    live = live_counts(ks, W)[-1]
    assert ref["tuples"].shape == (n, W, L) and ref["score"].shape == ref["err"].shape == (n, W)
    # dead rows are padded; live rows hold codes
    assert (ref["tuples"][:, live:] == -1).all() and np.isinf(ref["score"][:, live:]).all() and np.isinf(ref["err"][:, live:]).all()
    assert (ref["tuples"][:, :live] >= 0).all() and (ref["tuples"][:, :live] < np.asarray(ks)).all()
    # sorted scores, distinct beams
    assert (np.diff(ref["score"][:, :live], axis=1) >= 0).all()
    flat = (ref["tuples"][:, :live] * np.cumprod([1] + [int(k) for k in ks[:-1]])).sum(2)
    assert all(len(set(r)) == live for r in flat[:300].tolist())
    if W == 1:                                                                        # greedy at beam 0
        assert np.array_equal(ref["tuples"][:, 0], greedy)
    if n > 2000:                                                                      # (the looping rows: a sample below)
        pick = np.r_[0:64, n - 64:n]
        z, ref = z[pick], {k: v[pick] for k, v in ref.items()}
    # every beam agrees with the audit's rule, bit for bit
    for b in range(live):
        aud = audit_ref(z, cbs, ref["tuples"][:, b])
        assert same_bits(aud["err"], ref["err"][:, b]) and same_bits(aud["d_held"][:, L - 1], ref["score"][:, b])
        assert same_bits(aud["resid"], ref["resid"][:, b]) and (aud["flags"] == 0).all()
        if b == 0 and W == 1:
            assert (aud["rank"] == 0).all()


@pytest.mark.parametrize("row", bc.shapes(), ids=bc.shape_id)
def test_chosen_tuples_never_lose_to_greedy_and_beam_0_wins_on_the_whole(oracle, row):
    e, ks, W, n = row
    z, cbs, greedy = bc.inputs(e, ks, n)
    ref = bc.reference(e, ks, W, n)
    err_g = ac.reference(e, ks, n, "greedy")["err"] if (e, ks, n) in ac.shapes() else audit_ref(z, cbs, greedy)["err"]
    chosen, err_c, keep = choose_ref(ref, greedy, err_g)
    assert (err_c <= err_g).all() and err_c.astype(np.float64).sum() <= err_g.astype(np.float64).sum()
    assert same_bits(audit_ref(z, cbs, chosen)["err"], err_c)
    assert np.array_equal(chosen[keep], greedy[keep]) and np.array_equal(chosen[~keep], ref["tuples"][~keep, 0])
    if W == 1:
        assert not keep.any() and np.array_equal(chosen, greedy) and same_bits(err_c, err_g)
    # beam 0 alone, no fallback: a property of these inputs SUMMED over the items, not of the rule (the header promises nothing of the
    # kind, least of all per item: the table's lone item at e = 16 is one on which beam 0 loses at W = 2 and 4, so n = 1 is left out)
    if W > 1 and bc.deep(ks) and n > 1:
        assert ref["err"][:, 0].astype(np.float64).sum() < err_g.astype(np.float64).sum()


def test_reference_on_exact_ties(oracle):
    z, cbs = bc.tie_case()
    ref = beam_ref(z, cbs, 4)
    for i in range(4):                                                                # the items that ARE row 7
        assert ref["tuples"][i].tolist() == bc.TIE_BEAMS_OF_ROW_7
    assert (ref["score"][:4, :3] == ref["score"][:4, :1]).all()


def test_reference_on_nan_and_inf(oracle):
    z, cbs = bc.nan_case()
    for W in (2, 8):
        ref = beam_ref(z, cbs, W)
        assert not np.isnan(ref["score"]).any()
        assert (ref["tuples"][:, :, 0] != 9).all() or np.isinf(ref["score"][(ref["tuples"][:, :, 0] == 9).any(1)]).any()
        # the all-NaN latent: every distance is +inf, so the beams are the first W candidates in (parent, code) order
        assert ref["tuples"][3].tolist() == [[0, k] for k in range(W)] and np.isinf(ref["score"][3]).all()
        assert np.isnan(ref["err"][3]).all()
        for b in range(W):
            aud = audit_ref(z, cbs, ref["tuples"][:, b])
            assert same_bits(aud["err"], ref["err"][:, b]) and same_bits(aud["d_held"][:, 1], ref["score"][:, b])


# ---- the flag --------------------------------------------------------------------------------------------------------------------
def test_generate_refuses_beam_where_it_cannot_run(tmp_path):
    from lcrec_amd import generate_indices as gen
    base = ["--ckpt_path", "c.pth", "--output_dir", "out"]
    assert gen.parse_args(base).beam == 1 and gen.parse_args(base + ["--beam", "4"]).beam == 4
    with pytest.raises(SystemExit):
        gen.parse_args(base + ["--beam", "3"])
    no, out = str(tmp_path / "no.pth"), str(tmp_path / "out.json")
    # refused before the checkpoint is even opened (none of these files exist)
    with pytest.raises(ValueError, match="--beam 3"):
        gen.generate(no, out, device="cpu", beam=3)
    with pytest.raises(ValueError, match="--beam with --extend"):
        gen.generate(no, out, device="cpu", beam=4, extend=str(tmp_path / "base.json"))
    with pytest.raises(ValueError, match="--beam with --recheck_neartie"):
        gen.generate(no, out, device="cpu", beam=2, recheck=True)
    ctx = types.SimpleNamespace(enabled=True, rank=0, world_size=2)
    with pytest.raises(ValueError, match="--beam under torchrun"):
        gen.generate(no, out, device="cpu", ctx=ctx, beam=8)
    with pytest.raises(FileNotFoundError):
        gen.generate(no, out, device="cpu", beam=4, finish="nearest_free", audit=True)
    with pytest.raises(FileNotFoundError):                                            # width 1 is the plain path, with everything
        gen.generate(no, out, device="cpu", beam=1, recheck=True)
    assert not os.path.exists(out)
