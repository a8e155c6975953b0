"""CPU: the host side of converting fp16 / fp64 embedding files in HBM -- the lcrec_cast_rows entry (declared, exported, bound,
its argument checks, which return before any launch) and EmbDataset.to_device's `cast` keyword where no device is involved."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_cast_entry():
    import lcrec_amd
    header = open(os.path.join(ROOT, "include", "lcrec.h")).read()
    assert "#define LCREC_ABI_VERSION 3" in header
    assert re.search(r"#define LCREC_DTYPE_F16 1\b", header) and re.search(r"#define LCREC_DTYPE_F64 2\b", header)
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(lcrec_[a-z_0-9]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", lcrec_amd._lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (lcrec_[a-z_0-9]+)", out))
    assert "lcrec_cast_rows" in declared and "lcrec_cast_rows" in exported and "lcrec_cast_rows" in lcrec_amd._lib.EXPORTS
    assert hasattr(lcrec_amd._lib.load(), "lcrec_cast_rows")


def test_cast_entry_reports_argument_errors_before_any_launch():
    """LCREC_EINVAL, with a text that names the argument, comes back before anything is launched, so no device is needed.  (In a
    thread of its own: the library's last-error text is per thread, and other tests expect this thread's to be empty.)"""
    import ctypes
    import threading
    import lcrec_amd
    lib = lcrec_amd._lib.load()
    seen = []

    def calls():
        buf = (ctypes.c_double * 16)()
        p = ctypes.cast(buf, ctypes.c_void_p)                     # 16-byte aligned or not, 8-byte aligned for sure
        odd = ctypes.c_void_p(p.value + 2)
        seen.append((lib.lcrec_cast_rows(p, 0, 4, p, None), b"src_dtype", lib.lcrec_last_error()))
        seen.append((lib.lcrec_cast_rows(p, 7, 4, p, None), b"src_dtype", lib.lcrec_last_error()))
        seen.append((lib.lcrec_cast_rows(p, 1, -1, p, None), b"count -1", lib.lcrec_last_error()))
        seen.append((lib.lcrec_cast_rows(None, 1, 4, p, None), b"src is NULL", lib.lcrec_last_error()))
        seen.append((lib.lcrec_cast_rows(p, 2, 4, None, None), b"dst is NULL", lib.lcrec_last_error()))
        seen.append((lib.lcrec_cast_rows(odd, 2, 4, p, None), b"src must be aligned", lib.lcrec_last_error()))      # fp64 source at +2 bytes
        seen.append((lib.lcrec_cast_rows(p, 1, 4, odd, None), b"dst must be 4-byte aligned", lib.lcrec_last_error()))      # fp32 destination at +2 bytes
        seen.append((lib.lcrec_cast_rows(None, 1, 0, None, None), None, b""))                      # nothing to do: no launch, no error

    worker = threading.Thread(target=calls)
    worker.start()
    worker.join()
    assert len(seen) == 8
    for rc, word, text in seen[:-1]:
        assert rc == -1 and word in text, (rc, word, text)
    assert seen[-1][0] == 0


def test_cast_rows_refuses_cpu_tensors_and_other_dtypes():
    import lcrec_amd
    with pytest.raises(lcrec_amd.LcrecError):
        lcrec_amd.ops.cast_rows(torch.zeros(4, 8, dtype=torch.float16))
    with pytest.raises(lcrec_amd.LcrecError):
        lcrec_amd.ops.cast_rows(torch.zeros(4, 8, dtype=torch.float64))


@pytest.mark.parametrize("dtype", [np.float16, np.float64])
@pytest.mark.parametrize("mmap", [False, True])
def test_to_device_on_the_host_is_unchanged_for_fp16_and_fp64_files(tmp_path, dtype, mmap):
    from lcrec_amd.datasets import EmbDataset
    a = np.random.RandomState(11).standard_normal((53, 20)).astype(dtype)
    path = str(tmp_path / "T.emb-x-td.npy")
    np.save(path, a)
    want = a.astype(np.float32)
    for kwargs in ({}, {"cast": "auto"}, {"cast": "host"}, {"chunk_rows": 7}):
        got = EmbDataset(path, mmap=mmap).to_device("cpu", **kwargs)
        assert got.dtype == torch.float32 and got.device.type == "cpu"
        assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32)), kwargs
    part = EmbDataset(path, mmap=mmap).to_device("cpu", rows=(5, 41), chunk_rows=7)
    assert np.array_equal(part.numpy().view(np.uint32), want[5:41].view(np.uint32))


def test_explicit_device_cast_names_what_it_cannot_take(tmp_path):
    from lcrec_amd.datasets import EmbDataset
    a = np.random.RandomState(12).standard_normal((9, 8))
    files = {}
    for name, arr in (("f16", a.astype(np.float16)), ("f64", a), ("be", a.astype(">f2")), ("f32", a.astype(np.float32)),
                      ("i32", (a * 100).astype(np.int32)), ("fortran", np.asfortranarray(a))):
        files[name] = str(tmp_path / f"{name}.npy")
        np.save(files[name], arr)
    # a CPU target: refused whatever the file (checked before any device is touched)
    for name in ("f16", "f64"):
        with pytest.raises(ValueError, match="cpu"):
            EmbDataset(files[name]).to_device("cpu", cast="device")
    # files the kernel has no form for: the text names the dtype / the layout.  The target is never reached.
    for name, word in (("be", ">f2"), ("f32", "<f4"), ("i32", "<i4"), ("fortran", "C-contiguous")):
        with pytest.raises(ValueError, match=re.escape(word)):
            EmbDataset(files[name]).to_device("cuda:0", cast="device")
    # the predicate a caller can ask beforehand
    assert not EmbDataset(files["f16"]).casts_on_device("cpu") and EmbDataset(files["f16"]).casts_on_device("cuda:0")
    assert EmbDataset(files["f64"]).casts_on_device("cuda:0")
    assert not any(EmbDataset(files[k]).casts_on_device("cuda:0") for k in ("be", "f32", "i32", "fortran"))
    with pytest.raises(ValueError, match="sideways"):
        EmbDataset(files["f16"]).to_device("cpu", cast="sideways")
    # ... and under "auto" the same files take the host path as before
    for name in ("be", "i32", "fortran", "f32"):
        ds = EmbDataset(files[name])
        got = ds.to_device("cpu")
        assert np.array_equal(got.numpy(), np.asarray(ds.embeddings).astype(np.float32))
