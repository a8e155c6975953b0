"""What the three index-trie entries cost on the device (needs a MI355X; there is no CPU path and no fallback).

    python tools/trie_probe.py [--items 1000000] [--reps 200]

Every figure is the median of 5 samples after a warm-up of the same shape; a sample is `reps` back-to-back calls between two device
events, divided by reps (a single call of the smaller shapes is too short to time on its own).
  1. trie_build at `items` items of 4 x 256 codes, beside lcrec_collision_groups on the same matrix in the same run (three sorts
     against the build's one: the yardstick).
  2. trie_find at B = 640 and B = 65 536, depth 1 .. 4, on that trie; the queries are held tuples and random ones, half and half.
  3. trie_mask at B = 640 with V = 33 024 and V = 129 280, at depth 1 (256 children per node), beside a torch fill_ of the same
     [B, V] buffer in the same run.  The kernel only stores, so its bytes are B * V * 4; the rate is those bytes over the call time
     and `share` is the fill's time over the mask's.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import lcrec_amd  # noqa: E402
from lcrec_amd import ops  # noqa: E402

SAMPLES = 5


def timed(fn, reps):
    """median over SAMPLES of (device time of `reps` calls) / reps, in microseconds, after one warm-up sample"""
    times = []
    for sample in range(SAMPLES + 1):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        stop.synchronize()
        if sample:
            times.append(start.elapsed_time(stop) * 1e3 / reps)
    return statistics.median(times), min(times), max(times)


def line(name, t, extra=""):
    med, lo, hi = t
    print(f"{name:<44s} {med:10.1f} us   (min {lo:.1f}, max {hi:.1f}){extra}", flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("trie_probe needs a HIP device: nothing is measured without one")
    lcrec_amd._lib.load()
    dev = torch.device("cuda:0")
    ks, L, n = [256] * 4, 4, a.items
    g = torch.Generator(device=dev).manual_seed(1)
    idx = torch.randint(0, 256, (n, L), dtype=torch.int64, device=dev, generator=g)
    print(f"device: {torch.cuda.get_device_name(0)}; items {n}, codes 4 x 256; median of {SAMPLES}, {a.reps} calls per sample")

    # 1. build, beside collision_groups
    arrays = {name: torch.empty(size, dtype=dict(ops.TRIE_ARRAYS)[name], device=dev) for name, size in ops.trie_array_sizes(n, L).items()}
    line(f"trie_build            n={n}", timed(lambda: ops.trie_build(idx, ks, arrays=arrays), max(a.reps // 20, 1)))
    counters = torch.zeros(4, dtype=torch.int64, device=dev)
    members, offsets = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n // 2 + 2, dtype=torch.int64, device=dev)
    lib, karr = lcrec_amd._lib.load(), ops._ints(ks)
    ws = ops._workspace(lib.lcrec_collision_groups_workspace(n, L), dev)

    def groups():
        lcrec_amd._lib.check(lib.lcrec_collision_groups(ops._ptr(idx), n, L, karr, ops._ptr(members), ops._ptr(offsets), ops._ptr(counters),
                                                        ops._ptr(ws), ws.numel(), ops._stream_ptr()), "lcrec_collision_groups")
    line(f"collision_groups      n={n}", timed(groups, max(a.reps // 20, 1)))
    trie = ops.trie_build(idx, ks, arrays=arrays)
    counts = arrays["counts"][:L + 1].tolist()
    print(f"nodes per depth: {counts}")

    # 2. find
    for B in (640, 65536):
        held = idx[torch.randint(0, n, (B,), device=dev, generator=g)]
        rand = torch.randint(0, 256, (B, L), dtype=torch.int64, device=dev, generator=g)
        q = torch.where((torch.arange(B, device=dev) % 2 == 0)[:, None], held, rand).contiguous()
        node_out, depth_out = torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
        for depth in range(1, L + 1):
            t = timed(lambda: ops.trie_find(trie, q, depth, longest=True, node_out=node_out, depth_out=depth_out), a.reps)
            line(f"trie_find             B={B} depth={depth}", t)

    # 3. mask, beside a fill of the same bytes
    B, depth = 640, 1
    node = torch.randint(0, counts[depth], (B,), dtype=torch.int64, device=dev, generator=g)
    for V in (33024, 129280):
        logits = torch.zeros((B, V), dtype=torch.float32, device=dev)
        token_ids = (V - 1024 + 256 * depth + torch.arange(256, device=dev)).to(torch.int32)
        nbytes = B * V * 4
        mask = timed(lambda: ops.trie_mask_logits_(trie, logits, node, depth, token_ids, 2), a.reps)
        fill = timed(lambda: logits.fill_(float("-inf")), a.reps)
        again = timed(lambda: ops.trie_mask_logits_(trie, logits, node, depth, token_ids, 2), a.reps)   # alternated: mask, fill, mask
        line(f"trie_mask             B={B} V={V}", mask, f"  {nbytes / mask[0] / 1e6:.2f} TB/s written")
        line(f"torch fill_           B={B} V={V}", fill, f"  {nbytes / fill[0] / 1e6:.2f} TB/s written")
        line(f"trie_mask (again)     B={B} V={V}", again, f"  {nbytes / again[0] / 1e6:.2f} TB/s written; share of the fill's rate "
                                                          f"{fill[0] / again[0]:.2f}")


if __name__ == "__main__":
    main()
