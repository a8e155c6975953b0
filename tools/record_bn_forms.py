#!/usr/bin/env python3
"""Records tests/golden/f12_bn_forms.json: per row of tests/bn_cases.py and per call, the sha256 of the raw bytes of every output
tensor of the library as built, with the commit, the device and the hipcc version -- the bits a refactor of the BatchNorm strip
kernels must keep.  tests/test_gpu_bn_forms.py makes the same calls and compares.
  python tools/record_bn_forms.py [--commit SHA] [--out FILE]     on the GPU: run every case, write FILE
  python tools/record_bn_forms.py --manifest                      anywhere: enter the fixture into tests/golden/manifest.json"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
GOLD = os.path.join(ROOT, "tests", "golden")
NAME = "f12_bn_forms.json"


def dump(doc, path, end="\n"):
    with open(path, "w") as fh:
        fh.write(json.dumps(doc, indent=1, sort_keys=True) + end)


def record(commit, out):
    import torch
    import bn_cases as bn
    from lcrec_amd import ops
    cases = {}
    for run in bn.runs():
        cases[bn.run_id(run)] = got = bn.digests(bn.run_calls(ops, run[0], run[1], torch.device("cuda:0"))[0])
        same = got["backward_y"] == got["backward_beta"] == got["backward_fold"]
        print(f"{bn.run_id(run):>14}: {sum(map(len, got.values()))} outputs, the three mask sources {'agree' if same else 'DIFFER'}")
    said = subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True).stdout.splitlines()
    dump({"commit": commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip(),
          "device": torch.cuda.get_device_name(0), "hipcc": next((l for l in said if "version" in l), "unknown"), "cases": cases}, out)


def enter_into_manifest():
    with open(os.path.join(GOLD, NAME), "rb") as fh:
        raw = fh.read()
    with open(os.path.join(GOLD, "manifest.json")) as fh:
        m = json.load(fh)
    m["fixtures"][NAME] = {"bytes": len(raw), "inputs": "bn_cases.inputs(case) for every run of bn_cases.runs()",
                           "pins": "csrc/train_ops.hip: the bits of every output of the BatchNorm strip calls, form by form",
                           "recorded_at_commit": json.loads(raw)["commit"], "sha256": hashlib.sha256(raw).hexdigest()}
    dump(m, os.path.join(GOLD, "manifest.json"), end="")          # as oracle/make_golden.py leaves it


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit the loaded library was built from (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(GOLD, NAME))
    ap.add_argument("--manifest", action="store_true")
    a = ap.parse_args()
    enter_into_manifest() if a.manifest else record(a.commit, a.out)
