#!/usr/bin/env python3
"""Records the two fixtures that hold generate_indices.generate() still while its Python side is refactored, with the commit, the
device and the hipcc version; tests/generate_flow_cases.py lists what is recorded, and the two tests named below replay it.
  tests/golden/f13_generate_refusals.json: every combination of arguments that generate() refuses before it opens a file, and which
    refusal wins (host only; tests/test_generate_refusals_host.py)
  tests/golden/f14_generate_flows.json: per flow the sha256 of the file written and the statistics returned (GPU;
    tests/test_gpu_generate_flows.py).  Recorded in two processes of its own; a flow whose two recordings differ is left out and named.
  python tools/record_generate_flows.py --refusals [--commit SHA]           anywhere: write f13
  python tools/record_generate_flows.py --flows [--commit SHA] [--traces]   on the GPU: write f14 (--traces: print the per-kernel
                                                                             launch counts of cut-fbeam-spill and extend-cut-xbeam-spill-audit)
  python tools/record_generate_flows.py --manifest                          anywhere: enter both into tests/golden/manifest.json"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
GOLD = os.path.join(ROOT, "tests", "golden")
REFUSALS, FLOWS = "f13_generate_refusals.json", "f14_generate_flows.json"
TRACED = ("cut-fbeam-spill", "extend-cut-xbeam-spill-audit")


def dump(doc, path, end="\n"):
    with open(path, "w") as fh:
        fh.write(json.dumps(doc, indent=1, sort_keys=True) + end)


def header(commit, device):
    said = subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True).stdout.splitlines()
    return {"commit": commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip(),
            "device": device, "hipcc": next((l for l in said if "version" in l), "unknown")}


def record_refusals(commit):
    import generate_flow_cases as gfc
    from lcrec_amd import generate_indices as gen
    with tempfile.TemporaryDirectory() as tmp:
        outcomes, which = gfc.refusal_outcomes(gen, tmp)
    print(f"{len(which)} combinations, {len(outcomes)} distinct outcomes, {which.count(outcomes.index('FileNotFoundError'))} not refused")
    dump(dict(header(commit, "host"), grid=[[name, list(values)] for name, values in gfc.REFUSAL_GRID], outcomes=outcomes,
              which="".join(chr(ord("a") + w) for w in which)), os.path.join(GOLD, REFUSALS))


def flows_once(traces):
    """Every flow in this process -> {id: {"sha256", "stats"}}; printed as one JSON line for the parent."""
    import generate_flow_cases as gfc
    from lcrec_amd import generate_indices as gen, ops

    def traced(call):
        ops.trace_enable(True)
        try:
            stats = call()
        finally:
            seen = ops.trace_collect()
            ops.trace_enable(False)
        print("launches", json.dumps({k: v[0] for k, v in sorted(seen.items())}), file=sys.stderr)
        return stats

    with tempfile.TemporaryDirectory() as tmp:
        setup = gfc.Setup(gen, tmp)
        got = {}
        for flow in gfc.FLOWS:
            trace_it = traces and flow["id"] in TRACED
            if trace_it:
                print("flow", flow["id"], file=sys.stderr)
            got[flow["id"]] = setup.run(flow, traced if trace_it else None)
    print(json.dumps(got))


def record_flows(commit, traces):
    import torch
    import generate_flow_cases as gfc
    runs = []
    for k in range(2):
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--flows_once"] + (["--traces"] if traces and k == 0 else []),
                              capture_output=True, text=True, cwd=ROOT)
        sys.stderr.write(done.stderr)
        if done.returncode:
            sys.exit(f"recording {k} ended with {done.returncode}")
        runs.append(json.loads(done.stdout.strip().splitlines()[-1]))
    unstable = [name for name in gfc.FLOW_IDS if runs[0][name] != runs[1][name]]
    flows = {name: runs[0][name] for name in gfc.FLOW_IDS if name not in unstable}
    stats = [json.loads(f["stats"]) for f in flows.values()]
    print(f"{len(flows)} flows recorded; two recordings differ on: {unstable or 'none'}")
    for what, ok in (("spill_moved > 0", lambda s: s.get("spill_moved", 0) > 0),
                     ("finish_beam_moved > 0", lambda s: s.get("finish_beam_moved", 0) > 0),
                     ("extend_beam_moved > 0", lambda s: s.get("extend_beam_moved", 0) > 0),
                     ("extend_moved > 0 behind a beam step", lambda s: "extend_beam_width" in s and s["extend_moved"] > 0)):
        hits = [name for name, s in zip(flows, stats) if ok(s)]
        print(f"  {what}: {hits}")
        if not hits:
            sys.exit(f"no recorded flow has {what}")
    dump(dict(header(commit, torch.cuda.get_device_name(0)), flows=flows), os.path.join(GOLD, FLOWS))


def enter_into_manifest():
    with open(os.path.join(GOLD, "manifest.json")) as fh:
        m = json.load(fh)
    for name, inputs, pins in (
            (REFUSALS, "generate_flow_cases.REFUSAL_GRID, every combination, paths that do not exist",
             "generate_indices.generate: which arguments it refuses before it opens a file, and which refusal wins"),
            (FLOWS, "generate_flow_cases.FLOWS over golden_inputs.toy_checkpoint (F6, and F6 with its last codebook cut to 16 rows)",
             "generate_indices.generate, whole file and --extend: the bytes of the file written and every statistic returned")):
        with open(os.path.join(GOLD, name), "rb") as fh:
            raw = fh.read()
        m["fixtures"][name] = {"bytes": len(raw), "inputs": inputs, "pins": pins, "recorded_at_commit": json.loads(raw)["commit"],
                               "sha256": hashlib.sha256(raw).hexdigest()}
    dump(m, os.path.join(GOLD, "manifest.json"), end="")          # as oracle/make_golden.py leaves it


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="the commit the loaded package was built from (default: git rev-parse HEAD)")
    ap.add_argument("--refusals", action="store_true")
    ap.add_argument("--flows", action="store_true")
    ap.add_argument("--flows_once", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--traces", action="store_true")
    ap.add_argument("--manifest", action="store_true")
    a = ap.parse_args()
    if a.refusals:
        record_refusals(a.commit)
    if a.flows_once:
        flows_once(a.traces)
    if a.flows:
        record_flows(a.commit, a.traces)
    if a.manifest:
        enter_into_manifest()
