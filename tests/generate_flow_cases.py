"""What tools/record_generate_flows.py records and tests/test_generate_refusals_host.py / tests/test_gpu_generate_flows.py replay:
the arguments of generate_indices.generate() that it refuses before it opens a file (f13), and its flows over the F6 toy model,
whole file and --extend (f14).  Both fixtures were recorded before the whole-file and the --extend flow were folded into one
finishing pipeline: they say what that pipeline must keep -- which refusal wins, and every byte and statistic of a run."""
import hashlib
import itertools
import json
import os
import types

import numpy as np

import golden_inputs as gi

F6_CUT = 16                                                # spill_cases.F6_CUT: the cut model's last codebook
N0 = 2000                                                  # the rows of the --extend bases

# ---- f13: the refusals, in itertools.product order of these lists ------------------------------------------------------------------
REFUSAL_GRID = (("beam", (1, 4, 3)), ("finish", ("none", "nearest_free", "beam", "suffix")), ("extend", (None, "BASE")),
                ("extend_finish", ("nearest_free", "beam", "x")), ("spill", (False, True)), ("audit", (False, True)),
                ("recheck", (False, True)), ("ctx", (None, "TORCHRUN")), ("rounds", (20, 0, -1)), ("finish_width", (8, 3)))


def refusal_outcomes(gen, directory):
    """generate() on every combination of REFUSAL_GRID with checkpoint, base and output paths under `directory` that do not exist
    -> (the distinct outcomes in order of first appearance, one index per combination).  An outcome is the full ValueError text or
    the class name of any other exception (FileNotFoundError: nothing was refused, the checkpoint was looked for)."""
    ckpt, base, out = (os.path.join(str(directory), name) for name in ("no.pth", "no_base.index.json", "out/No.index.json"))
    torchrun = types.SimpleNamespace(enabled=True, rank=0, world_size=2)
    outcomes, which = [], []
    for combo in itertools.product(*(values for _, values in REFUSAL_GRID)):
        kw = dict(zip((name for name, _ in REFUSAL_GRID), combo))
        kw["extend"] = base if kw["extend"] else None
        kw["ctx"] = torchrun if kw["ctx"] else None
        try:
            gen.generate(ckpt, out, device="cpu", verbose=False, **kw)
            said = "returned"
        except ValueError as exc:
            said = str(exc)                                # (no refusal names a path)
        except Exception as exc:                           # noqa: BLE001  (the class is the outcome)
            said = type(exc).__name__
        if said not in outcomes:
            outcomes.append(said)
        which.append(outcomes.index(said))
    assert not os.path.exists(os.path.dirname(out)), "a refused call wrote something"
    return outcomes, which


# ---- f14: the flows ---------------------------------------------------------------------------------------------------------------
def _flow(name, model, base=None, rows=3000, **kw):
    return {"id": name, "model": model, "base": base, "rows": rows, "kw": kw}


NF, BEAM = "nearest_free", "beam"
FLOWS = [
    _flow("whole-defaults", "f6"),
    _flow("whole-rounds3", "f6", rounds=3),
    _flow("whole-rounds0", "f6", rounds=0),
    _flow("whole-nf", "f6", finish=NF),
    _flow("whole-nf-audit", "f6", finish=NF, audit=True),
    _flow("whole-fbeam-rounds0", "f6", finish=BEAM, rounds=0),
    _flow("whole-fbeam-w2-audit", "f6", finish=BEAM, finish_width=2, audit=True),
    _flow("whole-beam4-nf-audit", "f6", beam=4, finish=NF, audit=True),
    _flow("whole-beam2-fbeam-w4", "f6", beam=2, finish=BEAM, finish_width=4),
    _flow("cut-nf-spill", "cut", finish=NF, spill=True),
    _flow("cut-nf-spill-audit", "cut", finish=NF, spill=True, audit=True),
    _flow("cut-fbeam-spill", "cut", finish=BEAM, spill=True),
    _flow("cut-beam2-fbeam-w4-spill-audit", "cut", beam=2, finish=BEAM, finish_width=4, spill=True, audit=True),
    _flow("extend-finished-plain", "f6", "finished"),
    _flow("extend-finished-audit", "f6", "finished", audit=True),
    _flow("extend-finished-xbeam", "f6", "finished", extend_finish=BEAM),
    _flow("extend-finished-xbeam-w2-audit", "f6", "finished", extend_finish=BEAM, finish_width=2, audit=True),
    _flow("extend-finished-finish-ignored", "f6", "finished", finish=NF),
    _flow("extend-colliding-plain", "f6", "colliding"),
    _flow("extend-colliding-xbeam", "f6", "colliding", extend_finish=BEAM),
    _flow("extend-cut-spill", "cut", "finished", spill=True),
    _flow("extend-cut-xbeam-spill-audit", "cut", "finished", extend_finish=BEAM, spill=True, audit=True),
    _flow("extend-nothing-new-plain", "f6", "finished", rows=N0),
    _flow("extend-nothing-new-xbeam-spill", "cut", "finished", rows=N0, extend_finish=BEAM, spill=True),
]
FLOW_IDS = [f["id"] for f in FLOWS]


class Setup:
    """The two checkpoints over gi.toy_items and the --extend bases of their first N0 rows, each built once under `directory`:
    "finished" with finish="nearest_free" (and spill=True on the cut model), "colliding" with the defaults."""

    def __init__(self, gen, directory):
        self.gen, self.dir, self.ckpt, self.bases = gen, str(directory), {}, {}
        for model, cut in (("f6", None), ("cut", F6_CUT)):
            where = os.path.join(self.dir, model)
            os.makedirs(where)
            items, self.ckpt[model] = gi.toy_checkpoint(where, cut_last=cut)
        self.head = os.path.join(self.dir, f"Toy{N0}.emb.npy")      # the first N0 rows: the bases' data file, and N == N0's
        np.save(self.head, items[:N0])

    def base(self, model, kind):
        if (model, kind) not in self.bases:
            path = os.path.join(self.dir, f"Base.{model}.{kind}.index.json")
            kw = {} if kind == "colliding" else {"finish": NF, "spill": model == "cut"}
            self.gen.generate(self.ckpt[model], path, device="cuda:0", data_path=self.head, verbose=False, **kw)
            self.bases[(model, kind)] = path
        return self.bases[(model, kind)]

    def run(self, flow, on_call=None):
        """One generate() call -> {"sha256": of the file it wrote, "stats": its statistics as json.dumps(sort_keys=True) writes
        them, so that floats keep their repr}.  on_call: wraps the call alone (the bases are built before it)."""
        out = os.path.join(self.dir, flow["id"] + ".index.json")
        kw = dict(flow["kw"])
        if flow["base"]:
            kw["extend"] = self.base(flow["model"], flow["base"])
        if flow["rows"] == N0:
            kw["data_path"] = self.head
        call = lambda: self.gen.generate(self.ckpt[flow["model"]], out, device="cuda:0", verbose=False, **kw)
        stats = on_call(call) if on_call else call()
        with open(out, "rb") as fh:
            return {"sha256": hashlib.sha256(fh.read()).hexdigest(), "stats": json.dumps(stats, sort_keys=True)}
