"""Inputs shared by test_finish_host.py and test_gpu_finish.py: the F6 fixture's final tuples with the last-level residuals
recomputed by the oracle, and small synthetic buckets."""
import json
import os
import re

import numpy as np

import golden_inputs as gi
from oracle import cpu_oracle

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_f6 = {}


def f6_case():
    """(idx int64 [3000, 3] decoded from the reference's json_text, resid_last [3000, 16], last codebook [48, 16], fixture)."""
    if not _f6:
        g = np.load(os.path.join(GOLD, "f6_generate.npz"))
        meta = json.load(open(os.path.join(GOLD, "manifest.json")))["fixtures"]["f6_generate.npz"]
        doc = json.loads(bytes(g["json_text"]).decode())
        assert list(doc) == [str(i) for i in range(len(doc))]
        idx = np.array([[int(re.fullmatch(r"<[a-z]_(\d+)>", t).group(1)) for t in doc[k]] for k in doc], dtype=np.int64)
        model = meta["model"]
        names = gi.state_dict_names(len(model["layers"]) + 1, model["bn"], len(model["num_emb_list"]))
        Ws = [g["sd__" + n + ".weight"] for n in names["encoder"]]
        bs = [g["sd__" + n + ".bias"] for n in names["encoder"]]
        cbs = [g["sd__" + n] for n in names["codebooks"]]
        enc = cpu_oracle.encode_assign(gi.toy_items(meta["seed"]), Ws, bs, cbs)
        rq = cpu_oracle.rq_assign(enc["latent"], cbs, want_resid=True)
        L = len(cbs)
        assert np.array_equal(rq["idx"][:, :L - 1], idx[:, :L - 1])        # the rounds never touch the codes above the last level
        _f6["case"] = (idx, gi.f32(rq["resid"][L - 1]), gi.f32(cbs[-1]), g)
    return _f6["case"]


def movers_by_count(idx):
    """Sum over tuples of (holders - 1): how many items must move for all tuples to be distinct."""
    _, counts = np.unique(np.asarray(idx), axis=0, return_counts=True)
    return int((counts - 1).sum())


def random_case(n, ks, e, seed, spread=1.0):
    """n items with random prefixes over ks[:-1] and random last codes in [0, ks[-1]): plenty of shared tuples when n is large
    against the number of tuples.  The residuals and the codebook are N(0, 1) draws."""
    r = gi.rs(seed)
    idx = np.stack([r.randint(0, k, size=n) for k in ks], axis=1).astype(np.int64)
    resid = gi.f32(r.standard_normal((n, e)) * spread)
    cb = gi.f32(r.standard_normal((ks[-1], e)))
    return idx, resid, cb
