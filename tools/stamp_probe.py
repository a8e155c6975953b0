#!/usr/bin/env python3
"""Where does a ping-pong GEMM phase spend its cycles?  Needs the diagnostic library
(make -C lc-rec_amd/csrc STAMP=1 into another directory) loaded through LCREC_LIB_PATH:

    LCREC_LIB_PATH=tools/diag/liblcrec_hip_stamp.so python tools/stamp_probe.py

Stamps (s_memtime, shader cycles) of workgroup 8, lane 0 of every wave, first 64 phases:
  compute role: 0 = phase entry, 1 = before the mid-phase barrier, 2 = after it, 3 = all 64 MFMAs issued
  staging role: 0 = phase entry, 1 = LDS writes done (before the barrier), 2 = after the barrier

Which phases those are.  The per-tile kernel (linear_fwd_pp2_kernel) stamps the 64 first phases of the workgroup's tile.  The
persistent kernel (linear_fwd_pp3_kernel, LCREC_STAMP3) numbers its phases on across the tiles of the workgroup's list and
keeps the first 64 of the LIST: at the default PROBE_K=2048 (64 K-tiles = 128 phases per tile) that is the first half of the
workgroup's FIRST tile -- no pieces of a previous tile in its HEAD -- where this probe used to show the last tile written.

    PROBE_K=768 PROBE_N=2048 LCREC_LIB_PATH=... python tools/stamp_probe.py --handover

prints the hand-over instead (profiles/pp3_handover_stamps.txt): with 24 K-tiles = 48 phases per tile, phases 44..47 are
TAIL0 / TAIL1 of the first tile, 48..49 HEAD0 of the second and 50..63 its piece phases; per phase the entry-to-entry
length of waves 0 and 4, and per part of the tile the length of a K-tile (two phases) against a STEADY one.
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lcrec_amd import _lib, ops  # noqa: E402


def handover(s, k):
    """Phase lengths around the hand-over from the first to the second tile of the workgroup's list (persistent kernel)."""
    assert k == 768, "--handover reads the phase numbers of 24 K-tiles per tile: PROBE_K=768"
    ent = s[:, :, 0]                       # phase entry of every wave
    length = np.diff(ent, axis=1)          # phase p -> p + 1
    print("phase lengths (entry to entry), waves 0 (group 0) and 4 (group 1); C = computes, S = stages")
    for p in range(20, 63):
        print(f"{p:3d}  w0 {'C' if p % 2 == 0 else 'S'} {int(length[0, p]):6d}   w4 {'C' if p % 2 == 1 else 'S'} {int(length[4, p]):6d}")

    def per_ktile(lo, hi, wave):
        return (ent[wave, hi] - ent[wave, lo]) / ((hi - lo) / 2)
    print("per K-tile (two phases), wave 0 / wave 4:")
    for name, lo, hi in (("STEADY  K-tiles 10..21 of tile 1", 20, 44), ("TAIL    K-tiles 22..23 of tile 1", 44, 48),
                         ("HEAD0   K-tile 0 of tile 2      ", 48, 50), ("PIECES  K-tiles 1..6 of tile 2  ", 50, 62)):
        print(f"  {name}: {per_ktile(lo, hi, 0):8.0f} {per_ktile(lo, hi, 4):8.0f}")
    print("tile 1 phases 2..19 (HEAD without pieces, first tile): %.0f %.0f per K-tile" % (per_ktile(2, 20, 0), per_ktile(2, 20, 4)))
    for wave, phases in ((0, (44, 46, 48, 50, 52, 54)), (4, (45, 47, 49, 51, 53, 55))):
        for p in phases:
            v = s[wave, p]
            print(f"compute phase {p} wave {wave}: entry->barrier {int(v[1] - v[0])}  in barrier {int(v[2] - v[1])}  "
                  f"barrier->64th MFMA {int(v[3] - v[2])}")


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    rows, k, n = 131072, int(os.environ.get("PROBE_K", "2048")), int(os.environ.get("PROBE_N", "1024"))
    x = torch.randn((rows, k), generator=g, device=dev)
    w = torch.randn((n, k), generator=g, device=dev) * 0.02
    b = torch.zeros(n, device=dev)
    for _ in range(3):
        ops.linear_forward(x, w, b, relu=True)
    torch.cuda.synchronize()
    lib = _lib.load()
    buf = (ctypes.c_ulonglong * (8 * 64 * 4))()
    lib.lcrec_debug_gemm_stamps.argtypes = [ctypes.c_void_p]
    rc = lib.lcrec_debug_gemm_stamps(ctypes.cast(buf, ctypes.c_void_p))
    assert rc == 0, rc
    s = np.frombuffer(buf, dtype=np.uint64).reshape(8, 64, 4).astype(np.int64)
    if "--handover" in sys.argv[1:]:
        return handover(s, k)
    t0 = s[:, 8, 0].min()
    print("phase | wave0 (group 0)                       | wave4 (group 1)        [cycles since phase 8 entry]")
    for p in range(int(os.environ.get("PROBE_P0", "8")), 24):
        def fmt(w):
            v = s[w, p] - t0
            role = "C" if (p % 2) == (w // 4) else "S"
            return role + " " + " ".join(f"{int(t):7d}" for t in v[: (4 if role == "C" else 3)])
        print(f"{p:5d} | {fmt(0):38s} | {fmt(4)}")
    # arrival of each computing wave at the mid-phase barrier, relative to the earliest of the four: who is late?
    print("phase | computing group | arrival at the barrier, cycles after the first of the four waves | barrier exit - last arrival")
    for p in range(int(os.environ.get("PROBE_P0", "8")), 24):
        g = p % 2
        arr = s[4 * g:4 * g + 4, p, 1]
        stg = s[4 * (1 - g):4 * (1 - g) + 4, p, 3]          # staging waves: just before their barrier (persistent form only)
        late = f" | staging waves arrive {' '.join(f'{int(a - arr.max()):6d}' for a in stg)} after the last computing wave" if stg.any() else ""
        print(f"{p:5d} | group {g}         | " + " ".join(f"{int(a - arr.min()):6d}" for a in arr) +
              f" | {int(s[4 * g, p, 2] - arr.max()):6d}" + late)
    # per-phase durations for a computing wave: entry -> barrier wait start -> barrier exit -> last MFMA issued
    comp = []
    for w in (0, 4):
        for p in range(8, 60):
            if (p % 2) == (w // 4):
                v = s[w, p]
                comp.append((v[1] - v[0], v[2] - v[1], v[3] - v[2]))
    comp = np.array(comp)
    print("compute phase, mean cycles: entry->before barrier %.0f | in barrier %.0f | barrier->64th MFMA issued %.0f"
          % tuple(comp.mean(0)))
    mbuf = (ctypes.c_ulonglong * (8 * 4))()
    if hasattr(lib, "lcrec_debug_gemm_marks"):
        lib.lcrec_debug_gemm_marks.argtypes = [ctypes.c_void_p]
        assert lib.lcrec_debug_gemm_marks(ctypes.cast(mbuf, ctypes.c_void_p)) == 0
        m = np.frombuffer(mbuf, dtype=np.uint64).reshape(8, 4).astype(np.int64)
        for w in (0, 4):
            d = np.diff(m[w])
            print("wave %d of workgroup 8: prologue %d | K loop %d (%d K-tiles) | epilogue issued %d cycles"
                  % (w, d[0], d[1], k // 32, d[2]))
    per = np.diff(s[0, 8:60:2, 0])
    print("period of two phases (wave 0 entry to entry): mean %.0f cycles (ideal: 8192 at K slice 32, 16384 at 64)" % per.mean())


if __name__ == "__main__":
    main()
