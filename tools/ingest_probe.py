#!/usr/bin/env python3
"""The step in front of the path: a `<DS>.emb-<plm>-td.npy` on the host -> fp32 rows resident in HBM
(EmbDataset.to_device: memory-mapped file, cast into two pinned staging buffers, chunked H2D copies on a side stream), and
what encode+assign makes per second when the items have to come over PCIe first.  --dtype is the file's dtype; for a float16 /
float64 file --cast says where it becomes fp32: in the host threads (the link then carries fp32) or in HBM (ops.cast_rows).
    python tools/ingest_probe.py [--items 1000000] [--dim 768] [--dtype float16] [--cast device]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lcrec_amd.datasets import EmbDataset  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--items", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--workers", type=int, nargs="*", default=[1, 4, 8, 16])
ap.add_argument("--dtype", choices=["float32", "float16", "float64"], default="float32", help="dtype of the file written")
ap.add_argument("--cast", choices=["auto", "host", "device"], default="auto", help="EmbDataset.to_device's cast path")
a = ap.parse_args()
if a.cast == "device" and a.dtype == "float32":
    ap.error("--cast device needs --dtype float16 or float64: an fp32 file has nothing to convert")
with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
    path = os.path.join(tmp, "Synth.emb-test-td.npy")
    rs = np.random.default_rng(0)
    x = rs.standard_normal((a.items, a.dim), dtype=np.float32)
    np.save(path, x.astype(a.dtype, copy=False))
    del x
    item = np.dtype(a.dtype).itemsize
    torch.zeros(1, device="cuda:0")
    t0 = time.perf_counter()
    pin = torch.empty((256 << 20) // 4, dtype=torch.float32, pin_memory=True)
    print(f"pinning 256 MB: {time.perf_counter() - t0:.3f} s")
    del pin
    for mmap in (False, True):
        for w in a.workers:
            t0 = time.perf_counter()
            ds = EmbDataset(path, mmap=mmap)
            t1 = time.perf_counter()
            dev = ds.to_device("cuda:0", workers=w, cast=a.cast)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            gb = dev.numel() * item / 1e9                      # bytes of the file, whatever the link carried
            path_taken = a.cast if a.cast != "auto" else ("device" if ds.casts_on_device(dev.device) else "host")
            print(f"{a.items} x {a.dim} {a.dtype} ({gb:.2f} GB), cast={path_taken}, mmap={mmap}, {w} host threads: np.load {t1 - t0:.2f} s, "
                  f"to_device {t2 - t1:.3f} s = {gb / (t2 - t1):.1f} GB/s = {a.items / (t2 - t1) / 1e6:.2f} M items/s over the link "
                  f"(page cache warm: the file was just written)", flush=True)
            assert torch.equal(dev[-3:].cpu(), torch.from_numpy(np.ascontiguousarray(ds.embeddings[-3:], dtype=np.float32)))
            del ds, dev
            torch.cuda.empty_cache()
