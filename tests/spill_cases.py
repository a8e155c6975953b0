"""Inputs shared by test_spill_host.py and test_gpu_spill.py: skewed random tuples whose buckets overflow while their super-bucket
has room, hand-built super-buckets, and the F6 model with its last codebook cut to its first 16 rows."""
import json
import os

import numpy as np

import finish_cases as fc
import golden_inputs as gi
from oracle import cpu_oracle
from spill_ref import three_op

_cache = {}


def skewed_case(n, ks, e, seed):
    """n items; the level L-2 column is drawn with p proportional to 2^-a, the other columns uniformly, so the low rows overflow
    while their super-bucket has room.  N(0, 1) residuals entering level L-2 and both codebooks; r1 follows from r2 and the item's
    code by the three-op update.  -> (idx int64 [n, L], r2 [n, e], r1 [n, e], cb_prev [K2, e], cb_last [K1, e])."""
    r = gi.rs(seed)
    L = len(ks)
    p = 0.5 ** np.arange(ks[L - 2], dtype=np.float64)
    cols = [r.randint(0, k, size=n) for k in ks]
    cols[L - 2] = r.choice(ks[L - 2], size=n, p=p / p.sum())
    idx = np.stack(cols, axis=1).astype(np.int64)
    r2 = gi.f32(r.standard_normal((n, e)))
    cb_prev = gi.f32(r.standard_normal((ks[L - 2], e)))
    cb_last = gi.f32(r.standard_normal((ks[L - 1], e)))
    return idx, r2, three_op(r2, cb_prev[idx[:, L - 2]]), cb_prev, cb_last


def colliding_among(idx, n_frozen):
    head = np.asarray(idx)[:n_frozen]
    return int(head.shape[0] - np.unique(head, axis=0).shape[0]) if n_frozen else 0


def groups_of(rows, ids=None):
    """Lists of item ids sharing a row of `rows` (two or more holders), first-occurrence order, ids ascending: what
    lcrec_collision_groups lists.  ids: only these items are looked at."""
    found = {}
    for i in (range(len(rows)) if ids is None else ids):
        found.setdefault(tuple(rows[i]), []).append(int(i))
    return [g for g in found.values() if len(g) >= 2]


def nine_movers_case(e):
    """L = 2, K2 = 6, K1 = 4.  Row 0 holds 13 items on 4 cells: the finishing pass leaves nine of them.  Row 1 holds two items, so
    it has two free cells, rows 2 .. 5 are empty.  Along the first axis the codes of level L-2 sit at 0, 10, 10.5, 11, 12 and 40
    and every r2 near 10.1: row 1 is every mover's nearest row with room, then row 2, then row 3."""
    r = gi.rs(61)
    cb_prev = np.zeros((6, e), dtype=np.float32)
    cb_prev[:, 0] = [0.0, 10.0, 10.5, 11.0, 12.0, 40.0]
    cb_prev[:, 1] = 0.25
    cb_last = gi.f32(r.standard_normal((4, e)))
    idx = np.array([[0, k] for k in r.randint(0, 4, size=13)] + [[1, 0], [1, 1]], dtype=np.int64)
    r2 = np.zeros((15, e), dtype=np.float32)
    r2[:, 0] = 10.1 + 0.02 * r.standard_normal(15)
    r2[:, 2] = 0.01 * r.standard_normal(15)
    return idx, r2, three_op(r2, cb_prev[idx[:, 0]]), cb_prev, cb_last


def exact_ties_case():
    """Small integers, so every product, sum and three-op update is exact in fp32.  K2 = 6 with rows 4 and 5 copies of rows 1 and
    2, K1 = 8 with rows 6 and 7 copies of rows 2 and 3; the residual rows come from a pool of five, so holders tie exactly too."""
    r = gi.rs(62)
    e, n = 32, 40
    cb_prev = gi.f32(r.randint(-2, 3, size=(6, e)))
    cb_prev[4], cb_prev[5] = cb_prev[1], cb_prev[2]
    cb_last = gi.f32(r.randint(-2, 3, size=(8, e)))
    cb_last[6], cb_last[7] = cb_last[2], cb_last[3]
    pool = gi.f32(r.randint(-2, 3, size=(5, e)))
    r2 = gi.f32(pool[r.randint(0, 5, size=n)])
    idx = np.stack([np.zeros(n, dtype=np.int64), r.randint(0, 4, size=n)], axis=1).astype(np.int64)   # all in row 0, codes 0 .. 3
    idx[30:, 0] = 3                                                                                 # ... and ten in row 3
    return idx, r2, three_op(r2, cb_prev[idx[:, 0]]), cb_prev, cb_last


def scattered_case():
    """5000 items on [2, 6, 8]; 40 of them, far apart, form the super-bucket of prefix 0, all in its row 0 (8 cells): 32 spill.
    The other 4960 carry prefix 1 and collide freely; they are not listed, so nothing may happen to them."""
    r = gi.rs(63)
    n, e = 5000, 32
    ids = np.unique(np.concatenate([[3, n - 1], r.choice(n, size=38, replace=False)]))
    idx = np.stack([np.ones(n, dtype=np.int64), r.randint(0, 6, size=n), r.randint(0, 8, size=n)], axis=1).astype(np.int64)
    idx[ids, 0] = 0
    idx[ids, 1] = 0
    r2 = gi.f32(r.standard_normal((n, e)))
    cb_prev, cb_last = gi.f32(r.standard_normal((6, e))), gi.f32(r.standard_normal((8, e)))
    return idx, r2, three_op(r2, cb_prev[idx[:, 1]]), cb_prev, cb_last, ids


F6_CUT = 16


def f6_cut():
    """The F6 model with its last codebook cut to its first 16 rows (num_emb_list 48, 48, 16), on the oracle:
    dict(idx = pass-1 tuples int64 [3000, 3], resid = [4, 3000, 16] residuals entering each level, cbs, fixture, meta, state)."""
    if "f6" not in _cache:
        g = fc.f6_case()[3]
        meta = json.load(open(os.path.join(fc.GOLD, "manifest.json")))["fixtures"]["f6_generate.npz"]
        model = meta["model"]
        names = gi.state_dict_names(len(model["layers"]) + 1, model["bn"], len(model["num_emb_list"]))
        Ws = [g["sd__" + n + ".weight"] for n in names["encoder"]]
        bs = [g["sd__" + n + ".bias"] for n in names["encoder"]]
        cbs = [gi.f32(g["sd__" + n]) for n in names["codebooks"]]
        cbs[-1] = np.ascontiguousarray(cbs[-1][:F6_CUT])
        enc = cpu_oracle.encode_assign(gi.toy_items(meta["seed"]), Ws, bs, cbs)
        rq = cpu_oracle.rq_assign(enc["latent"], cbs, want_resid=True)
        assert np.array_equal(rq["idx"], enc["idx"])
        _cache["f6"] = {"idx": rq["idx"].astype(np.int64), "resid": rq["resid"], "cbs": cbs, "fixture": g, "meta": meta,
                        "last_name": "sd__" + names["codebooks"][-1]}
    return _cache["f6"]
