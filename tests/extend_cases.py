"""Inputs shared by test_extend_host.py and test_gpu_extend.py: the F6 fixture split into a frozen base and new items, small
synthetic buckets with frozen holders, and a helper that keeps the library's per-thread last-error text out of the main thread."""
import json
import os
import threading

import numpy as np

import finish_cases as fc
import golden_inputs as gi
from finish_ref import finish_ref
from oracle import cpu_oracle

_cache = {}


def in_thread(fn, *args, **kw):
    """fn(*args, **kw) in a thread of its own; its result or exception comes back.  (The library's last-error text is per thread,
    and other tests expect the main thread's to be empty: every call that is refused on purpose goes through here.)"""
    box = {}

    def run():
        try:
            box["value"] = fn(*args, **kw)
        except BaseException as exc:                                        # noqa: B902 -- handed to the caller
            box["error"] = exc
    t = threading.Thread(target=run)
    t.start()
    t.join()
    if "error" in box:
        raise box["error"]
    return box["value"]


def f6_pass1():
    """The oracle's pass-1 tuples of the 3000 F6 items (cpu_oracle.encode_assign): int64 [3000, 3]."""
    if "pass1" not in _cache:
        idx, resid, cb, g = fc.f6_case()
        meta = json.load(open(os.path.join(fc.GOLD, "manifest.json")))["fixtures"]["f6_generate.npz"]
        model = meta["model"]
        names = gi.state_dict_names(len(model["layers"]) + 1, model["bn"], len(model["num_emb_list"]))
        Ws = [g["sd__" + n + ".weight"] for n in names["encoder"]]
        bs = [g["sd__" + n + ".bias"] for n in names["encoder"]]
        cbs = [g["sd__" + n] for n in names["codebooks"]]
        first = cpu_oracle.encode_assign(gi.toy_items(meta["seed"]), Ws, bs, cbs)["idx"].astype(np.int64)
        assert np.array_equal(first[:, :-1], idx[:, :-1])                   # the rounds only ever moved last codes
        _cache["pass1"] = first
    return _cache["pass1"]


def f6_split(n0, base="finished"):
    """(union idx int64 [3000, 3], resid_new [3000 - n0, 16], last codebook [48, 16]).
    base "finished": finish_ref of the first n0 of F6's final tuples, a collision-free base; "reference": the reference's own
    final tuples, which still collide.  The new items carry the oracle's pass-1 tuples."""
    key = ("split", n0, base)
    if key not in _cache:
        idx, resid, cb, _ = fc.f6_case()
        head = idx[:n0].copy()
        if base == "finished":
            head, _, unresolved = finish_ref(head, resid[:n0], cb)
            assert unresolved == 0
        union = np.concatenate([head, f6_pass1()[n0:]]).astype(np.int64)
        _cache[key] = (union, gi.f32(resid[n0:]), cb)
    u, r, c = _cache[key]
    return u.copy(), r, c


def one_bucket(codes, n_frozen, K, e, seed, prefix=None):
    """One bucket (L = 2, prefix code 0) whose items hold `codes` in id order; N(0, 1) residuals for the new items and codebook."""
    r = gi.rs(seed)
    n = len(codes)
    idx = np.stack([np.zeros(n, dtype=np.int64), np.asarray(codes, dtype=np.int64)], axis=1)
    if prefix is not None:
        idx[:, 0] = prefix
    resid_new = gi.f32(r.standard_normal((n - n_frozen, e)))
    cb = gi.f32(r.standard_normal((K, e)))
    return idx, resid_new, cb


def random_split_case(n, n_frozen, ks, e, seed):
    """fc.random_case with the first n_frozen items frozen: frozen items collide among themselves too, as a base file may."""
    idx, resid, cb = fc.random_case(n, ks, e, seed)
    return idx, gi.f32(resid[n_frozen:]), cb


def colliding_among(idx, n_frozen):
    head = np.asarray(idx)[:n_frozen]
    return int(head.shape[0] - np.unique(head, axis=0).shape[0]) if n_frozen else 0
