"""The case table of the frozen-aware beam finishing pass (lcrec_extend_finish_beam), shared by tests/test_extend_beam_host.py (CPU:
the numpy rule of tests/extend_beam_ref.py alone, on every row) and tests/test_gpu_extend_beam.py (GPU: the kernels against that
rule, integer-exact).

A row is beam_finish_cases' (idx, ks, members, offsets, err_held, cand, cand_err, W) with n_frozen.  Three kinds:
  * q-...-f1 / -f2: the QUANT rows of beam_finish_cases with about n/3 and about 2n/3 items frozen.  Latents exist for the new items
    only: err_held and the candidates are computed from z[n_frozen:], for the new members, and scattered to their positions;
  * s-...-f1 / -f2, s-...-nf0 / -nfn / -nfn1: its SYNTH rows with a frozen head (the 80-bit keys, dead candidates, NaN errors,
    foreign member ids, 255 / 256 / 257 items, widths 1 .. 8, the 20 000 items that take the sorts past one block);
  * h-...: rows written by hand, each with the result it must give.
In a CLEAN row the positions of frozen members hold dead candidates (-1), cand_err +inf and err_held FILL_ERR.  poisoned(row) is the
same row with those positions holding what would change the result if it were read: the candidate lists of new movers (free,
attractive tuples, which real movers propose) with cand_err -inf, and err_held -inf or NaN.  The result must be the clean row's."""
import functools

import numpy as np

import beam_finish_cases as bfc
import golden_inputs as gi
from audit_ref import audit_ref
from beam_finish_ref import groups_of
from beam_ref import beam_ref
from extend_beam_ref import extend_finish_beam_ref

FILL_ERR = np.float32(0.0)            # a clean frozen position's err_held: smaller than any new holder's, were it read

# SYNTH rows of beam_finish_cases and the frozen counts they get here: "f1" about n / 3, "f2" about 2 n / 3, and the edges
SYNTH_FROZEN = (("s-wide-hi", ("f1", "f2")), ("s-wide-lo", ("f1",)), ("s-wide-both", ("f2",)), ("s-dead", ("f1", "f2", "nf0", "nfn", "nfn1")),
                ("s-own", ("f1",)), ("s-nan", ("f1", "f2")), ("s-foreign", ("f1", "f2")), ("s-n1", ("nf0", "nfn")),
                ("s-n255", ("f1",)), ("s-n256", ("f1", "f2")), ("s-n257", ("f2",)), ("s-w1", ("f1", "nfn1")), ("s-large", ("f1",)))


def _count(n, tag):
    return {"f1": n // 3, "f2": (2 * n) // 3, "nf0": 0, "nfn": n, "nfn1": max(n - 1, 0)}[tag]


def _frozen(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def from_quantiser(z_new, cbs, idx, n_frozen, W):
    """the entry's inputs for the tuples idx, the latents of the NEW items only (row i - n_frozen): what extend_beam_collisions
    computes on the device.  Frozen positions are clean."""
    ks = tuple(int(c.shape[0]) for c in cbs)
    members, offsets = groups_of(idx, ks)
    M, L = len(members), len(ks)
    err_held = np.full(M, FILL_ERR, dtype=np.float32)
    cand = np.full((M, W, L), -1, dtype=np.int64)
    cand_err = np.full((M, W), np.inf, dtype=np.float32)
    fresh = np.flatnonzero(members >= n_frozen)
    if fresh.size:
        items = members[fresh]
        zz = np.ascontiguousarray(z_new[items - n_frozen])
        err_held[fresh] = audit_ref(zz, cbs, idx[items])["err"]
        beams = beam_ref(zz, cbs, W)
        cand[fresh], cand_err[fresh] = beams["tuples"], beams["err"]
    return {"idx": np.ascontiguousarray(idx), "ks": ks, "members": members, "offsets": offsets, "err_held": err_held, "cand": cand,
            "cand_err": cand_err, "W": W, "n_frozen": int(n_frozen)}


def with_frozen_head(c, n_frozen):
    """a beam_finish_cases row with items below n_frozen frozen: their positions are made clean"""
    c = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    held = (c["members"] >= 0) & (c["members"] < n_frozen)
    c["err_held"][held] = FILL_ERR
    c["cand"][held] = -1
    c["cand_err"][held] = np.inf
    c["n_frozen"] = int(n_frozen)
    return c


# ---- rows written by hand: (case, (idx, choice, counters)) ---------------------------------------------------------------------------
def _hand(idx, n_frozen, members, offsets, err_held, cand, cand_err, ks=(8, 8)):
    cand = np.array(cand, dtype=np.int64)
    return {"idx": np.array(idx, dtype=np.int64), "ks": tuple(ks), "members": np.array(members, dtype=np.int64),
            "offsets": np.array(offsets, dtype=np.int64), "err_held": gi.f32(err_held), "cand": cand, "cand_err": gi.f32(cand_err),
            "W": cand.shape[1], "n_frozen": n_frozen}


X, Y, Z, F = (0, 0), (7, 7), (6, 1), (5, 5)
DEAD = (-1, -1)
INF = float("inf")


def _hand_rows():
    rows = {}
    # a frozen holder against a new holder whose err_held is smaller: the frozen one keeps the tuple
    rows["h-frozen-keeps"] = (
        _hand([X, X], 1, [0, 1], [0, 2], [5.0, 0.1], [[DEAD, DEAD], [(1, 1), (2, 2)]], [[INF, INF], [0.5, 0.6]]),
        ([X, (1, 1)], [-1, 0], [1, 1, 0, 1]))
    # a group whose holders are all frozen beside one that mixes them: items 0 and 1 go on colliding, items 3 and 4 both move (item
    # 4 wins (1, 1) in round 0, item 3 takes its next candidate in round 1)
    rows["h-allfrozen-mixed"] = (
        _hand([X, X, Y, Y, Y, Z], 3, [0, 1, 2, 3, 4], [0, 2, 5], [0, 0, 0, 0.1, 0.2],
              [[DEAD, DEAD], [DEAD, DEAD], [DEAD, DEAD], [(1, 1), (2, 2)], [(1, 1), (3, 3)]],
              [[INF, INF], [INF, INF], [INF, INF], [0.2, 0.3], [0.1, 0.5]]),
        ([X, X, Y, (2, 2), (1, 1), Z], [-1, -1, -1, 1, 0], [2, 2, 0, 2]))
    # a group whose only new holder is its last member; its candidate 0 is its own tuple, which is in O
    rows["h-last-new"] = (
        _hand([X, X, X, X], 3, [0, 1, 2, 3], [0, 4], [0, 0, 0, 3.0],
              [[DEAD, DEAD], [DEAD, DEAD], [DEAD, DEAD], [X, (4, 4)]], [[INF, INF], [INF, INF], [INF, INF], [0.0, 1.0]]),
        ([X, X, X, (4, 4)], [-1, -1, -1, 1], [1, 1, 0, 1]))
    # beam_finish_cases' s-sync with item 0 frozen: items 1, 2 and 3 all move, whatever item 0's err_held (here the LARGEST)
    sync = with_frozen_head(bfc.case("s-sync"), 1)
    sync["err_held"][0] = 9.0
    rows["h-sync-f0"] = (sync, (bfc.SYNC_WANT["idx"], bfc.SYNC_WANT["choice"], bfc.SYNC_WANT["counters"]))
    # a mover whose candidate 0 is the tuple of a frozen item that collides with nobody: in O all the same
    rows["h-cand0-frozen"] = (
        _hand([F, X, X], 2, [1, 2], [0, 2], [0, 0.4], [[DEAD, DEAD], [F, (6, 6)]], [[INF, INF], [0.1, 0.9]]),
        ([F, X, (6, 6)], [-1, 1], [1, 1, 0, 1]))
    # nobody is new in the one group (n_frozen = n - 1, and the new item collides with nobody)
    rows["h-new-alone"] = (
        _hand([X, X, Z], 2, [0, 1], [0, 2], [0, 0], [[DEAD, DEAD], [DEAD, DEAD]], [[INF, INF], [INF, INF]]),
        ([X, X, Z], [-1, -1], [0, 0, 0, 0]))
    return rows


HAND = _hand_rows()


def rows():
    quant = [f"{name}-W{W}-{tag}" for name, _, _, _, widths in bfc.QUANT for W in widths for tag in ("f1", "f2")]
    synth = [f"{name}-{tag}" for name, tags in SYNTH_FROZEN for tag in tags]
    return quant + synth + list(HAND)


def true_groups(row):
    """whether the row's group table is that of its idx"""
    return not row.startswith("s-foreign")


@functools.lru_cache(maxsize=None)
def case(row):
    """the row's inputs: beam_finish_cases' dict with n_frozen (read-only arrays), frozen positions clean"""
    if row in HAND:
        return _frozen({k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in HAND[row][0].items()})
    base, tag = row.rsplit("-", 1)
    if row.startswith("q-"):
        name, W = base.rsplit("-W", 1)
        z, cbs, greedy = bfc.quant_inputs(name)
        n_frozen = _count(len(greedy), tag)
        return _frozen(from_quantiser(z[n_frozen:], cbs, greedy, n_frozen, int(W)))
    c = bfc.case(base)
    return _frozen(with_frozen_head(c, _count(len(c["idx"]), tag)))


@functools.lru_cache(maxsize=None)
def poisoned(row):
    """the row with the frozen members' positions holding what must never be read"""
    c = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in case(row).items()}
    members, n_frozen, W = c["members"], c["n_frozen"], c["W"]
    n, L = c["idx"].shape
    r = gi.rs(9100 + sum(map(ord, row)))
    held = np.flatnonzero((members >= 0) & (members < n_frozen))
    fresh = np.flatnonzero((members >= n_frozen) & (members < n))
    taken = {tuple(t) for t in c["idx"].tolist()}
    for k, j in enumerate(held):
        if fresh.size:                                      # the list of a new member: tuples that real movers propose
            c["cand"][j] = c["cand"][fresh[k % fresh.size]]
        else:                                               # nobody is new: free tuples drawn at random
            for b in range(W):
                t = tuple(int(r.randint(0, kk)) for kk in c["ks"])
                c["cand"][j, b] = t if t not in taken else -1
        c["cand_err"][j] = -np.inf
        c["err_held"][j] = (-np.inf, np.nan)[k % 2]
    return _frozen(c)


def run_rule(c):
    out = extend_finish_beam_ref(c["idx"], c["n_frozen"], c["ks"], c["members"], c["offsets"], c["err_held"], c["cand"], c["cand_err"])
    out[0].setflags(write=False)
    out[1].setflags(write=False)
    return out[0], out[1], tuple(out[2])


@functools.lru_cache(maxsize=None)
def reference(row):
    """extend_finish_beam_ref of the clean row: (idx, choice, counters), computed once, shared, read only"""
    return run_rule(case(row))


def capture_pair():
    """beam_finish_cases.capture_pair with the first third of the items frozen in both sets: every host-side argument is shared,
    n_frozen included; set A is clean at the frozen positions and set B poisoned there."""
    a, b = bfc.capture_pair()
    n_frozen = len(a["idx"]) // 3
    a, b = _frozen(with_frozen_head(a, n_frozen)), with_frozen_head(b, n_frozen)
    held = (b["members"] >= 0) & (b["members"] < n_frozen)
    src = np.flatnonzero(~held)
    b["cand"][held] = b["cand"][src[np.arange(held.sum()) % src.size]]
    b["cand_err"][held] = -np.inf
    b["err_held"][held] = np.nan
    return a, _frozen(b)


# ---- the trained F6 model: a frozen base and new items on their pass-1 tuples (extend_cases.f6_split) -------------------------------
@functools.lru_cache(maxsize=None)
def f6_flow(n0=2000, base="finished", W=8):
    """The numpy flow of generate(extend=..., extend_finish="beam") on the F6 split: the rule on the union, then extend_ref on what it
    leaves, with the residuals of the moved items' new prefixes.  Also extend_ref alone (today's --extend) and the error sums of the
    new items' tuples (float64): greedy, after the beam step, after the flow, after extend_ref alone."""
    import extend_cases as ec
    from extend_ref import extend_ref
    z, cbs, greedy, _ = bfc.f6_model()
    L = len(cbs)
    union, resid_new, cb_last = ec.f6_split(n0, base)
    assert np.array_equal(union[n0:], greedy[n0:])
    z_new = np.ascontiguousarray(z[n0:])
    c = from_quantiser(z_new, cbs, union, n0, W)
    idx_beam, choice, counters = run_rule(c)
    resid = bfc.prefix_resid(z_new, cbs, np.ascontiguousarray(idx_beam[n0:]), L - 1)
    idx_final, movers, unresolved = extend_ref(idx_beam, n0, resid, cbs[-1])
    alone, alone_movers, alone_unresolved = extend_ref(union, n0, resid_new, cb_last)
    err = lambda idx: float(audit_ref(z_new, cbs, np.ascontiguousarray(idx[n0:]))["err"].astype(np.float64).sum())
    return {"case": c, "union": union, "idx_beam": idx_beam, "choice": choice, "counters": counters, "resid_new": resid,
            "idx_final": idx_final, "extend": (len(movers) - unresolved, unresolved), "alone": alone,
            "alone_extend": (len(alone_movers) - alone_unresolved, alone_unresolved),
            "err": {"greedy": err(union), "beam": err(idx_beam), "flow": err(idx_final), "alone": err(alone)}}
