"""CPU: the host side of dropout in the captured training step -- the mask definition of include/lcrec.h restated in numpy
(tests/philox_ref.py) against the generator's published known answers, the two new entry points, and the engine's
support matrix."""
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import philox_ref as ph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_numpy_philox_reproduces_the_random123_known_answers(counter, key, want):
    got = ph.philox4x32_10(counter, key)
    assert " ".join(f"{int(v):08x}" for v in got) == want
    # vectorised over counters: the same words
    many = ph.philox4x32_10(tuple(np.full(5, c, dtype=np.uint64) for c in counter), key)
    assert many.shape == (5, 4) and (many == got).all()


def test_threshold_and_scale_of_the_keep_rule():
    assert ph.threshold(0.0) == (0, np.float32(1.0))
    assert ph.threshold(0.5) == (2 ** 31, np.float32(2.0))
    assert ph.threshold(0.1)[0] == int(0.1 * 2.0 ** 32) == 429496729
    assert ph.threshold(1.0 - 2.0 ** -40)[0] == 2 ** 32 - 1
    # element -> (counter, lane): element i of a row-major tensor takes lane i % 4 of counter i // 4, rows offset by row_offset
    w = ph.words((6, 8), seed=(5 << 32) | 7, step=3, position=2, row_offset=10)
    one = ph.philox4x32_10(((10 * 8 + 2 * 8 + 4) // 4, 0, 2, 3), (7, 5))
    assert (w[2, 4:8] == one).all()


def test_header_declares_and_library_exports_the_dropout_entries():
    import lcrec_amd
    header = open(os.path.join(ROOT, "include", "lcrec.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(lcrec_[a-z_0-9]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", lcrec_amd._lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (lcrec_[a-z_0-9]+)", out))
    for name in ("lcrec_dropout_apply", "lcrec_dropout_mask"):
        assert name in declared and name in exported and name in lcrec_amd._lib.EXPORTS, name
    assert "#define LCREC_ABI_VERSION 3" in header
    for bad in (1.0, 1.5, -0.1, float("nan")):
        with pytest.raises(lcrec_amd.LcrecError):
            lcrec_amd.ops.dropout_threshold(bad)
    assert lcrec_amd.ops.dropout_threshold(0.1) == (ph.threshold(0.1)[0], 1.0 / 0.9)


def test_dropout_entries_report_argument_errors_before_any_launch():
    """LCREC_EINVAL comes back before anything is launched, so no device is needed.  (In a thread of its own: the library's
    last-error text is per thread, and other tests expect this thread's to be empty until they set it.)"""
    import ctypes
    import threading
    import lcrec_amd
    lib = lcrec_amd._lib.load()
    seen = []

    def calls():
        buf = (ctypes.c_int64 * 64)()
        p = ctypes.cast(buf, ctypes.c_void_p)
        T, s = ph.threshold(0.1)[0], float(ph.threshold(0.1)[1])
        seen.append((lib.lcrec_dropout_apply(p, p, 4, 30, T, s, p, p, 0, 0, None), b"features", lib.lcrec_last_error()))
        seen.append((lib.lcrec_dropout_apply(p, p, 4, 32, T, s, None, p, 0, 0, None), b"NULL", lib.lcrec_last_error()))
        for bad in (float("inf"), -3.0, 0.5, float("nan")):              # p = 1, p > 1, p < 0, p = NaN
            seen.append((lib.lcrec_dropout_apply(p, p, 4, 32, T, bad, p, p, 0, 0, None), b"scale", lib.lcrec_last_error()))
        seen.append((lib.lcrec_dropout_mask(p, 4, 32, T, p, p, -1, 0, None), b"position", lib.lcrec_last_error()))
        seen.append((lib.lcrec_dropout_mask(p, 4, 32, T, p, p, 0, -5, None), b"row_offset", lib.lcrec_last_error()))

    worker = threading.Thread(target=calls)
    worker.start()
    worker.join()
    assert len(seen) == 8
    for rc, word, text in seen:
        assert rc == -1 and word in text, (rc, word, text)


def _tiny_cpu(bn, dropout_prob):
    """The model of tests/test_gpu_train.py's _tiny, on the host."""
    import lcrec_amd
    g = np.load(os.path.join(GOLD, f"f4_step_bn{bn}.npz"))
    model = lcrec_amd.RQVAE(in_dim=128, num_emb_list=[256] * 4, e_dim=16, layers=[64, 32], dropout_prob=dropout_prob, bn=bool(bn),
                            loss_type="mse", quant_loss_weight=1.0, beta=0.25, kmeans_init=False, kmeans_iters=100,
                            sk_epsilons=[0.0, 0.0, 0.0, 0.003], sk_iters=50)
    model.load_state_dict({k[4:]: torch.from_numpy(g[k].copy()) for k in g.files if k.startswith("sd__")}, strict=True)
    return model


@pytest.mark.parametrize("bn", [0, 1])
def test_support_matrix_accepts_dropout_on_one_process_only(monkeypatch, bn):
    """unsupported_reason with the device check stubbed (the model is on the host here): 0 < p < 1 is covered; p >= 1 and
    data-parallel runs still name dropout, so the trainer falls back for them as before."""
    from lcrec_amd.engine import TrainEngine
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    model = _tiny_cpu(bn, 0.1)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
    assert TrainEngine.unsupported_reason(model, opt) is None
    off = types.SimpleNamespace(enabled=False, world_size=1)
    assert TrainEngine.unsupported_reason(model, opt, dist=off) is None
    on = types.SimpleNamespace(enabled=True, world_size=2)
    assert "dropout" in TrainEngine.unsupported_reason(model, opt, dist=on)
    for p in (1.0,):
        full = _tiny_cpu(bn, p)
        assert "dropout" in TrainEngine.unsupported_reason(full, torch.optim.AdamW(full.parameters(), lr=1e-3))
    # and without dropout neither context matters
    plain = _tiny_cpu(bn, 0.0)
    assert TrainEngine.unsupported_reason(plain, torch.optim.AdamW(plain.parameters(), lr=1e-3), dist=on) is None
