"""The case table of the beam finishing pass (lcrec_finish_beam), shared by tests/test_beam_finish_host.py (CPU: the numpy rule of
tests/beam_finish_ref.py alone, on every row) and tests/test_gpu_beam_finish.py (GPU: the kernels against that rule, integer-exact).

A row is (idx, ks, members, offsets, err_held, cand, cand_err): the entry needs no quantiser.  QUANT rows are made by one all the
same -- audit_cases.inputs' latents and greedy tuples, the groups of those tuples, audit_ref's err of the members' held tuples and
beam_ref's beams of the members' latents -- and SYNTH rows are drawn or written by hand for what a quantiser does not produce:
keys wider than 64 bits, dead candidates in the middle of a list, a candidate equal to the item's own tuple, NaN errors, member
ids outside [0, n), error ties, the workgroup boundary, and enough items and candidates to take the sorts past one block."""
import functools

import numpy as np

import audit_cases as ac
import golden_inputs as gi
from audit_ref import audit_ref
from beam_finish_ref import finish_beam_ref, groups_of
from beam_ref import beam_ref

WIDTHS = (1, 2, 4, 8)

# (name, e, ks, n or (distinct, repeats), widths)
QUANT = (("q-48_100_7", 32, (48, 100, 7), 1000, (2, 4, 8)),
         ("q-8_8_8", 16, (8, 8, 8), 257, (2, 4, 8)),
         ("q-3_5_2", 16, (3, 5, 2), 257, (2, 4, 8)),          # nearly everything unresolved
         ("q-2", 16, (2,), 65, (1, 8)),                       # no candidate is ever free
         ("q-nogroup", 32, (256, 256, 256, 256), 1000, (8,)),  # no group: no launch
         ("q-repeat10", 16, (48, 100, 7), (40, 10), (8,)),    # identical candidates, exact error ties
         ("q-deep", ac.DEEP_E, ac.KS_DEEP, (64, 5), (8,)))
WIDE_KS = (32,) * 16                                           # 80 bits: levels 0 .. 2 lie in the high word, level 3 straddles
# (name, n, ks, width, what)
SYNTH = (("s-wide-hi", 300, WIDE_KS, 4, "hi"), ("s-wide-lo", 300, WIDE_KS, 8, "lo"), ("s-wide-both", 300, WIDE_KS, 2, "both"),
         ("s-dead", 257, (48, 100, 7), 8, "dead"), ("s-own", 257, (8, 8, 8), 4, "own"), ("s-nan", 257, (8, 8, 8), 4, "nan"),
         ("s-foreign", 257, (8, 8, 8), 4, "foreign"), ("s-sync", 6, (8, 8), 4, "sync"),
         ("s-n1", 1, (8, 8), 2, ""), ("s-n255", 255, (20, 20), 4, ""), ("s-n256", 256, (20, 20), 4, ""), ("s-n257", 257, (20, 20), 8, ""),
         ("s-w1", 257, (8, 8, 8), 1, ""), ("s-large", 20000, (48, 100, 7), 8, "large"))


def rows():
    return [f"{name}-W{W}" for name, _, _, _, widths in QUANT for W in widths] + [name for name, *_ in SYNTH]


def true_groups(row):
    """whether the row's group table is that of its idx (so that n minus the distinct tuples afterwards equals `unresolved`)"""
    return not row.startswith("s-foreign")


def _frozen(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def quant_inputs(name):
    """(z, codebooks, greedy tuples) of a QUANT row"""
    _, e, ks, n, _ = next(q for q in QUANT if q[0] == name)
    if isinstance(n, tuple):
        z, cbs, _, _, _ = ac.inputs(e, ks, n[0])
        z = np.ascontiguousarray(np.repeat(z, n[1], axis=0))
        greedy = np.repeat(ac.inputs(e, ks, n[0])[2], n[1], axis=0)
    else:
        z, cbs, greedy, _, _ = ac.inputs(e, ks, n)
    return z, cbs, np.ascontiguousarray(greedy)


def from_quantiser(z, cbs, idx, W):
    """the entry's inputs for the tuples idx of the latents z: what beam_finish_collisions computes on the device"""
    ks = tuple(int(c.shape[0]) for c in cbs)
    members, offsets = groups_of(idx, ks)
    L = len(ks)
    if len(members):
        err_held = audit_ref(z[members], cbs, idx[members])["err"]
        beams = beam_ref(z[members], cbs, W)
        cand, cand_err = beams["tuples"], beams["err"]
    else:
        err_held, cand, cand_err = np.zeros(0, np.float32), np.zeros((0, W, L), np.int64), np.zeros((0, W), np.float32)
    return {"idx": idx, "ks": ks, "members": members, "offsets": offsets, "err_held": gi.f32(err_held),
            "cand": np.ascontiguousarray(cand, dtype=np.int64), "cand_err": gi.f32(cand_err), "W": W}


def _draw(r, n, ks, W, pool_size, held_size, levels=None):
    """idx and candidates drawn from one pool of tuples (so that candidates meet held tuples and each other), errors on a coarse
    grid (so that they tie).  levels: the levels in which the pool's tuples differ (None: all)."""
    L = len(ks)
    base = np.array([r.randint(0, k) for k in ks], dtype=np.int64)
    pool = np.tile(base, (pool_size, 1))
    for l in (range(L) if levels is None else levels):
        pool[:, l] = r.randint(0, ks[l], size=pool_size)
    idx = pool[r.randint(0, min(held_size, pool_size), size=n)]
    members, offsets = groups_of(idx, ks)
    M = len(members)
    cand = pool[r.randint(0, pool_size, size=(M, W))]
    err_held = gi.f32(r.randint(0, 6, size=M) / 4.0)
    cand_err = gi.f32(np.sort(r.randint(0, 12, size=(M, W)) / 4.0, axis=1))
    return {"idx": np.ascontiguousarray(idx), "ks": tuple(ks), "members": members, "offsets": offsets, "err_held": err_held,
            "cand": np.ascontiguousarray(cand), "cand_err": cand_err, "W": W}


def _sync_case():
    """Synchronous rounds against sequential service.  Items 0 .. 3 hold X = (0, 0); item 0 keeps it.  A = item 1, B = item 2 and
    C = item 3 move.  Round 0: A and B propose T1 and A wins; C proposes T2 and takes it.  Round 1: B's next candidate is T2, which
    C claimed in the round B lost in, so B goes on to T3.  Served one after the other in id order B would have taken T2 before C.
    Items 4 and 5 hold other tuples."""
    X, T1, T2, T3, T4, T5 = (0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, 5)
    idx = np.array([X, X, X, X, (6, 6), (7, 7)], dtype=np.int64)
    cand = np.array([[T4, T4, T4, T4],                      # the keeper's list is never read
                     [T1, T4, T5, X], [T1, T2, T3, T4], [T2, T5, T4, X]], dtype=np.int64)
    cand_err = gi.f32([[9, 9, 9, 9], [0.1, 1, 2, 3], [0.2, 0.1, 0.3, 0.4], [0.5, 1, 2, 3]])
    return {"idx": idx, "ks": (8, 8), "members": np.arange(4, dtype=np.int64), "offsets": np.array([0, 4], dtype=np.int64),
            "err_held": gi.f32([0.0, 1, 1, 1]), "cand": cand, "cand_err": cand_err, "W": 4}


SYNC_WANT = {"idx": [(0, 0), (1, 1), (3, 3), (2, 2), (6, 6), (7, 7)], "choice": [-1, 0, 2, 0], "counters": [3, 3, 0, 2]}


@functools.lru_cache(maxsize=None)
def case(row):
    """the row's inputs: a dict of idx, ks, members, offsets, err_held, cand, cand_err, W (read-only arrays)"""
    if row.startswith("q-"):
        name, W = row.rsplit("-W", 1)
        z, cbs, greedy = quant_inputs(name)
        return _frozen(from_quantiser(z, cbs, greedy, int(W)))
    name, n, ks, W, what = next(s for s in SYNTH if s[0] == row)
    r = gi.rs(7100 + sum(map(ord, row)))
    if what == "sync":
        return _frozen(_sync_case())
    if what in ("hi", "lo", "both"):
        levels = {"hi": (0, 1, 2), "lo": tuple(range(5, 16)), "both": None}[what]
        return _frozen(_draw(r, n, ks, W, 400, 120, levels))
    if what == "large":
        return _frozen(_draw(r, n, ks, W, 30000, 12000))
    c = _draw(r, n, ks, W, max(4, 2 * n), max(2, n // 2))
    M = len(c["members"])
    if what == "dead" and M:
        for j in range(M):                                  # one or two dead candidates inside the list, of every kind
            b = r.randint(0, W - 1)
            c["cand"][j, b, r.randint(0, len(ks))] = (-1, ks[0] + 200, 1 << 40, -(1 << 40))[j % 4]
            if j % 3 == 0:
                c["cand"][j, (b + 2) % W] = -1              # a whole -1 row, as lcrec_rq_beam pads
    if what == "own" and M:
        for j in range(M):
            c["cand"][j, j % 2] = c["idx"][c["members"][j]]
    if what == "nan" and M:
        c["err_held"][::3] = np.nan                         # a NaN never keeps a tuple against a finite value ...
        c["err_held"][1::7] = np.inf
        c["cand_err"][::2, 0] = np.nan                      # ... and never wins one
        c["cand_err"][1::5, 1] = -0.0
        c["cand_err"][2::5, 1] = 0.0
    if what == "foreign" and M:
        G = len(c["offsets"]) - 1
        for g in range(G):                                  # the first / last member of some groups is not an item
            if g % 3 == 0:
                c["members"][c["offsets"][g]] = (-3, -(1 << 40))[g % 2]
            if g % 3 == 1:
                c["members"][c["offsets"][g + 1] - 1] = (n, n + 5, 1 << 33)[g % 3]
    return _frozen(c)


@functools.lru_cache(maxsize=None)
def reference(row):
    """finish_beam_ref of the row: (idx, choice, counters), computed once, shared, read only"""
    c = case(row)
    idx, choice, counters = finish_beam_ref(c["idx"], c["ks"], c["members"], c["offsets"], c["err_held"], c["cand"], c["cand_err"])
    idx.setflags(write=False)
    choice.setflags(write=False)
    return idx, choice, tuple(counters)


def capture_pair():
    """Two input sets that share every host-side argument of the call (n, L, ks, the group count, the member count, the width) and
    differ in everything the device reads: B holds A's tuples with the codes of level 0 permuted -- the same groups in the same
    order -- other errors, and every member's candidate list reshuffled."""
    a = dict(case("s-dead"))
    r = gi.rs(7177)
    perm = r.permutation(a["ks"][0]).astype(np.int64)
    b = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in a.items()}
    b["idx"][:, 0] = perm[a["idx"][:, 0]]
    M, W = a["cand_err"].shape
    order = np.argsort(r.random_sample((M, W)), axis=1)
    cand = np.take_along_axis(a["cand"], order[:, :, None], axis=1)
    live = (cand[:, :, 0] >= 0) & (cand[:, :, 0] < a["ks"][0])
    cand[:, :, 0] = np.where(live, perm[np.clip(cand[:, :, 0], 0, a["ks"][0] - 1)], cand[:, :, 0])
    b["cand"] = np.ascontiguousarray(cand)
    b["err_held"] = gi.f32(r.randint(0, 6, size=M) / 4.0)
    b["cand_err"] = gi.f32(r.randint(0, 12, size=(M, W)) / 4.0)
    m2, o2 = groups_of(b["idx"], b["ks"])
    assert np.array_equal(m2, a["members"]) and np.array_equal(o2, a["offsets"])
    return a, _frozen(b)


# ---- the trained F6 model (tests/golden/f6_generate.npz) -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def f6_model():
    """(latents, codebooks, pass-1 greedy tuples, the reference's final tuples) of the F6 fixture, on the oracle, once"""
    import json
    import os

    import finish_cases as fc
    from oracle import cpu_oracle
    held, _, _, g = fc.f6_case()
    meta = json.load(open(os.path.join(fc.GOLD, "manifest.json")))["fixtures"]["f6_generate.npz"]
    names = gi.state_dict_names(len(meta["model"]["layers"]) + 1, meta["model"]["bn"], len(meta["model"]["num_emb_list"]))
    cbs = [gi.f32(g["sd__" + n]) for n in names["codebooks"]]
    enc = cpu_oracle.encode_assign(gi.toy_items(meta["seed"]), [g["sd__" + n + ".weight"] for n in names["encoder"]],
                                   [g["sd__" + n + ".bias"] for n in names["encoder"]], cbs)
    return gi.f32(enc["latent"]), cbs, enc["idx"].astype(np.int64), held


def prefix_resid(z, cbs, idx, depth):
    """the residual entering level `depth` of the tuples idx: audit_ref's residual of the prefix idx[:, :depth] (depth 0: the latent)"""
    return z if depth == 0 else audit_ref(z, cbs[:depth], np.ascontiguousarray(idx[:, :depth]))["resid"]


@functools.lru_cache(maxsize=None)
def f6_flow(W=8):
    """The numpy flow of generate(rounds=0, finish="beam") on F6: the rule on the greedy tuples, then finish_ref on what it leaves,
    with the residuals of the moved items' new prefixes.  -> dict of idx_beam, choice, counters, idx_final, finish (moved, unresolved)"""
    from finish_ref import finish_ref
    z, cbs, greedy, _ = f6_model()
    L = len(cbs)
    c = from_quantiser(z, cbs, greedy, W)
    idx_beam, choice, counters = finish_beam_ref(c["idx"], c["ks"], c["members"], c["offsets"], c["err_held"], c["cand"], c["cand_err"])
    resid = prefix_resid(z, cbs, idx_beam, L - 1)
    idx_final, movers, unresolved = finish_ref(idx_beam, resid, cbs[-1])
    return {"case": c, "idx_beam": idx_beam, "choice": choice, "counters": counters, "resid_last": resid, "idx_final": idx_final,
            "finish": (len(movers) - unresolved, unresolved)}
