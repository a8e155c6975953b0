"""The capture table of the index-side entries that launch more than once per call -- lcrec_finish_nearest_free,
lcrec_extend_nearest_free, lcrec_spill_nearest_free, lcrec_rq_audit and lcrec_rq_beam -- shared by tests/test_capture_cases_host.py
(CPU: the references alone) and tests/test_gpu_capture_forms.py (GPU: each call recorded into a graph once and replayed on other
inputs, bit for bit).  include/lcrec.h promises of each "no allocation, no synchronisation, capturable".

A row is (entry, e), one per entry and e in ES.  Its shape comes from the entry's own case table, so that the references of input
set A are the cached ones the other tests use:
  finish    nearest_free_cases' random_buckets row, ks (3, 48), n = 96
  extend    the same row with n_frozen = 32
  spill     nearest_free_cases' over_64 row, ks (6, 40), n = 218: more than 64 holders, an idle keeper wave, both kernels and both
            memsets
  rq_audit  audit_cases' (48, 100, 7) at n = 257, the tuples columns 1 .. L of an int64 [n, L + 2] matrix (idx_stride = L + 2),
            `best` and `resid` requested
  rq_beam   beam_cases' (48, 100, 7) at W = 4, n = 257, `resid` requested
A graph bakes in every host-side argument -- n, ks, W, n_frozen, the lengths of the group tables, the bucket counts, every address --
so the second input set B of a row shares all of those with A and differs in device DATA only:
  finish, extend   every residual row negated (the group tables depend on idx alone, and idx is A's)
  spill            r2 negated, r1 = three_op(r2, cb_prev[idx[:, 0]])
  rq_audit         the oracle's greedy tuples instead of the random ones
  rq_beam          z with its rows reversed; items are independent, so its reference is A's reversed
variant(row, which) gives one set: the host-side arguments, the device inputs by name and the expected outputs by name.  For the
nearest-free entries the in/out `idx` is both: the input is the starting idx, the expected one the reference's.  Every comparison
is exact (same_bits, the judge of test_gpu_audit.py and test_gpu_beam.py): nothing here has a tolerance."""
import functools
from collections import namedtuple

import numpy as np

import audit_cases as ac
import beam_cases as bc
import nearest_free_cases as nc
from extend_ref import extend_ref
from finish_ref import finish_ref
from spill_ref import spill_ref, three_op

ES = (16, 32, 64)
ENTRIES = ("finish", "extend", "spill", "rq_audit", "rq_beam")
Row = namedtuple("Row", "entry e")
Variant = namedtuple("Variant", "host inputs expected")
ROWS = [Row(entry, e) for entry in ENTRIES for e in ES]
GARBAGE = 0x7FC12345                                        # (as int32: a NaN as a float, a large code as an integer)

KS_WALK = (48, 100, 7)                                      # rq_audit and rq_beam
N_WALK = 257
BEAM_W = 4
AUDIT_NAMES = ("d_held", "d_best", "rank", "best", "err", "resid", "flags")
BEAM_NAMES = ("tuples", "score", "err", "resid")


def row_id(row):
    return f"{row.entry}-e{row.e}"


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return False
    if got.dtype.kind != "f":
        return np.array_equal(got.astype(np.int64), want.astype(np.int64))
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].astype(np.float32).view(np.uint32))


def judge(got, want):
    """the GPU test's judge: every expected output is there, with the expected bits"""
    return set(got) == set(want) and all(same_bits(got[name], want[name]) for name in want)


def garbage_like(expected):
    """what a replay that wrote nothing would leave behind: every output element the GARBAGE fill of its buffer"""
    out = {}
    for name, a in expected.items():
        a = np.asarray(a)
        words = np.full(a.size * a.dtype.itemsize // 4, GARBAGE, dtype=np.int32)
        out[name] = words.view(a.dtype).reshape(a.shape)
    return out


def nearest_free_row(row):
    """the row of nearest_free_cases.ROWS whose shape and inputs this row runs"""
    want = {"finish": (nc.random_buckets, (3, 48)), "extend": (nc.random_buckets, (3, 48)), "spill": (nc.over_64, (6, 40))}[row.entry]
    found = [r for r in nc.ROWS if (r.entry, r.e, r.builder, r.ks) == (row.entry, row.e) + want]
    assert len(found) == 1, row_id(row)
    return found[0]


def flat_table(groups):
    """item-id lists -> (members, offsets) int64 in lcrec_collision_groups' "device" layout"""
    members = np.array([int(i) for g in groups for i in g], dtype=np.int64)
    offsets = np.cumsum([0] + [len(g) for g in groups]).astype(np.int64)
    return members, offsets


def _counters(moved, unresolved):
    return np.array([moved, unresolved], dtype=np.int64)


def _nearest_free(row, which):
    nrow = nearest_free_row(row)
    inp = nc.inputs(nrow)
    idx, nf = inp["idx"], nrow.n_frozen
    host = {"n": nrow.n, "ks": tuple(nrow.ks), "e": row.e, "n_frozen": nf}
    if row.entry == "spill":
        tg, sg = nc.tables(nrow, idx)
        r2, r1 = inp["r2"], inp["r1"]
        if which == "B":
            r2 = np.negative(r2)
            r1 = three_op(r2, inp["cb_prev"][idx[nf:, -2]])
        (tmem, toff), (smem, soff) = flat_table(tg), flat_table(sg)
        inputs = {"idx": idx, "r2": r2, "r1": r1, "cb_prev": inp["cb_prev"], "cb_last": inp["cb_last"], "tuple_members": tmem,
                  "tuple_offsets": toff, "super_members": smem, "super_offsets": soff}
        if which == "A":
            res = nc.reference(nrow)
        else:
            new, served, unres = spill_ref(idx, nf, r2, r1, inp["cb_prev"], inp["cb_last"], tg, sg)
            res = nc.Result(new, tuple(served), int(unres), len(served) - int(unres))
        host.update(n_tuple_groups=len(tg), n_super_groups=len(sg), tuple_members=len(tmem), super_members=len(smem))
    else:
        buckets = nc.tables(nrow, idx)
        resid = inp["resid"] if which == "A" else np.negative(inp["resid"])
        members, offsets = flat_table(buckets)
        inputs = {"idx": idx, "resid": resid, "cb": inp["cb"], "members": members, "offsets": offsets}
        if which == "A":
            res = nc.reference(nrow)
        else:
            if row.entry == "finish":
                new, served, unres = finish_ref(idx, resid, inp["cb"], buckets=buckets)
            else:
                new, served, unres = extend_ref(idx, nf, resid, inp["cb"], buckets=buckets)
            res = nc.Result(new, tuple(served), int(unres), len(served) - int(unres))
        host.update(n_buckets=len(buckets), members=len(members))
    return Variant(host, inputs, {"idx": np.asarray(res.idx), "counters": _counters(res.moved, res.unresolved)})


def _flat(cbs):
    return np.concatenate([c.reshape(-1) for c in cbs])


def _rq_audit(row, which):
    e, ks, n, L = row.e, KS_WALK, N_WALK, len(KS_WALK)
    z, cbs, greedy, _, rand = ac.inputs(e, ks, n)
    wide = np.full((n, L + 2), -3, dtype=np.int64)                # (the columns beside the tuples are never read)
    wide[:, 1:1 + L] = rand if which == "A" else greedy
    ref = ac.reference(e, ks, n, "random" if which == "A" else "greedy")
    host = {"n": n, "e": e, "ks": ks, "idx_stride": L + 2, "first_column": 1}
    return Variant(host, {"z": z, "codebooks": _flat(cbs), "idx_wide": wide}, {name: ref[name] for name in AUDIT_NAMES})


def _rq_beam(row, which):
    e, ks, n = row.e, KS_WALK, N_WALK
    z, cbs, _ = bc.inputs(e, ks, n)
    ref = bc.reference(e, ks, BEAM_W, n)
    if which == "B":
        z, ref = np.ascontiguousarray(z[::-1]), {name: np.ascontiguousarray(a[::-1]) for name, a in ref.items()}
    host = {"n": n, "e": e, "ks": ks, "width": BEAM_W}
    return Variant(host, {"z": z, "codebooks": _flat(cbs)}, {name: ref[name] for name in BEAM_NAMES})


@functools.lru_cache(maxsize=None)
def variant(row, which):
    """input set `which` ("A" or "B") of a row: computed once, shared, read only"""
    assert which in ("A", "B")
    build = {"rq_audit": _rq_audit, "rq_beam": _rq_beam}.get(row.entry, _nearest_free)
    v = build(row, which)
    for a in list(v.inputs.values()) + list(v.expected.values()):
        a.setflags(write=False)
    return v


def rows_differing(a, b):
    """the items on which two expected results differ in any per-item output"""
    n = len(a["idx"]) if "idx" in a else len(a["err"])
    bad = np.zeros(n, dtype=bool)
    for name in a:
        if len(a[name]) == n:
            bad |= np.array([not same_bits(x, y) for x, y in zip(a[name], b[name])])
    return int(bad.sum())
