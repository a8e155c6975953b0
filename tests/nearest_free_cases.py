"""The case table of the nearest-free kernels of finish.hip -- finish_nearest_free_kernel<E, false> (entry `finish`), its frozen
form <E, true> (`extend`), spill_keepers_kernel<E> and spill_movers_kernel<E> (`spill`) -- shared by
tests/test_nearest_free_cases_host.py (CPU: the numpy rules of finish_ref.py, extend_ref.py and spill_ref.py alone) and
tests/test_gpu_nearest_free_forms.py (GPU: each row once through its entry, bit for bit).

A row is (entry, e, ks, n, n_frozen, builder, covers).  builder(row) is a deterministic numpy function: for finish and extend it
returns (idx, resid_new, cb, buckets) -- buckets a list of item-id lists as a caller would pass them, or None for the groups of
idx[:, :L-1] -- and for spill (idx, r2_new, r1_new, cb_prev, cb_last, listing), listing(idx) -> (tuple groups, super groups) or None
for the groups of idx and of idx[:, :L-2].  The residual arrays hold the rows of the new items only.

covers names entries of PROPERTIES: each a predicate over (row, the row's inputs, the reference's own result), where the result
gives the served order, where every mover went and the unresolved count -- so a row cannot claim a path its data does not reach.
REQUIRED is every property; each must be claimed at every e in ES (the largest_level_* ones by one row per entry and e)."""
import functools
from collections import namedtuple

import numpy as np

import golden_inputs as gi
import spill_cases as sc
from extend_ref import extend_ref
from finish_ref import finish_ref
from oracle import cpu_oracle
from spill_ref import spill_ref, three_op

ES = (16, 32, 64)
CHUNK = 256                                                                  # positions a workgroup walks at a time; threads
Row = namedtuple("Row", "entry e ks n n_frozen builder covers")
Result = namedtuple("Result", "idx served unresolved moved")
Step = namedtuple("Step", "id group pos free taken")                         # one served mover: see timeline()

# ---- the largest last level each entry admits at L = 2, derived from the LDS formulas (include/lcrec.h: a level lcrec_rq_assign
# takes, and K * (4 e + 20) + 512 bytes -- 4 more per code with the frozen-holder counts -- within 160 KB) ------------------------
LDS_PER_CU = 160 * 1024
LARGEST = {"finish": {16: 1920, 32: 1088, 64: 576}, "extend": {16: 1856, 32: 1074, 64: 576}}


def level_fits(entry, K, e, L=2):
    rows = (K + 31) & ~31                                                    # lcrec_rq_assign's 256-thread form: rows of e + 4 floats,
    rq = (rows * (e + 4) + ((rows + 3) & ~3)) * 4 + 4 * L * 8               # cc, and one double per wave and level
    own = K * (8 + (e + 1) * 4 + 4 + 4 + (4 if entry == "extend" else 0)) + 512
    return K > 0 and rq <= LDS_PER_CU and own <= LDS_PER_CU


# ---- builders ----------------------------------------------------------------------------------------------------------------------
def _one_bucket(codes, L=2):
    idx = np.zeros((len(codes), L), dtype=np.int64)
    idx[:, L - 1] = codes
    return idx


def _as_spill(idx, r1, cb_last, row, r):
    """the rows of a finish / extend case in one super-bucket: every item in row 0 of level L-2, K2 = row.ks[-2]"""
    K2, e = row.ks[-2], row.e
    full = np.zeros((idx.shape[0], 2), dtype=np.int64)
    full[:, 1] = idx[:, -1]
    cb_prev = gi.f32(r.standard_normal((K2, e)))
    r2 = gi.f32(r.standard_normal(r1.shape))
    return full, r2, r1, cb_prev, cb_last, None


NEG_SEED = {16: 916, 32: 937, 64: 965}                                       # draws on which the property below holds


def negative(row):
    """Holders on codes 0 .. 3 of K = 24, each residual its own code's row plus noise of 0.01 under a codebook of scale 37: the
    own-code distance is rounding noise of either sign (xx and cc are near 1369 e, their ulp above the true 1e-4 e).  extend: four
    frozen bystanders on codes 10 .. 13; spill: the same rows in row 0 of a K2 = 3 super-bucket."""
    r = gi.rs(NEG_SEED[row.e])
    K, e, nf = row.ks[-1], row.e, row.n_frozen
    codes = np.concatenate([np.arange(10, 10 + nf), r.randint(0, 4, size=row.n - nf)])
    cb = gi.f32(r.standard_normal((K, e)) * 37)
    resid = gi.f32(cb[codes[nf:]] + gi.f32(r.standard_normal((row.n - nf, e)) * 0.01))
    idx = _one_bucket(codes, L=len(row.ks))
    if row.entry == "spill":
        return _as_spill(idx, resid, cb, row, r)
    return idx, resid, cb, None


def nan_inf(row):
    """K = 16 (spill: K1 = 16 under K2 = 4, every item in row 1, row 0 filled by sixteen bystanders).  Code 0 is held alone.  Code 1:
    an all-NaN holder and two finite ones.  Code 6: a holder with one NaN element, then a finite one with a higher id.  Code 8: three
    holders with a NaN each.  The last code's row -- and for spill the last row of level L-2 too -- holds a +inf element."""
    r = gi.rs(910 + row.e)
    K, e, nf = row.ks[-1], row.e, row.n_frozen
    codes = [4, 5][:nf] + [0, 1, 1, 1, 6, 6, 8, 8, 8, 3]
    cb = gi.f32(r.standard_normal((K, e)))
    cb[K - 1, 2] = np.inf
    resid = gi.f32(r.standard_normal((len(codes) - nf, e)))
    resid[1] = np.nan                                                        # code 1: all NaN -> a mover with no finite distance
    resid[4, 5] = np.nan                                                     # code 6: loses to the finite holder behind it
    resid[6, 0] = np.nan                                                     # code 8: nobody is finite -> the lowest id keeps
    resid[7] = np.nan
    resid[8, e - 1] = np.nan
    if row.entry != "spill":
        return _one_bucket(codes), resid, cb, None
    full = np.array([[1, c] for c in codes], dtype=np.int64)
    fill = np.array([[0, k] for k in range(K)], dtype=np.int64)              # row 0 has no room: new bystanders behind everyone
    full = np.concatenate([full, fill])
    r1 = np.concatenate([resid, gi.f32(r.standard_normal((K, e)))])
    cb_prev = gi.f32(r.standard_normal((row.ks[-2], e)))
    cb_prev[row.ks[-2] - 1, 1] = np.inf
    r2 = gi.f32(r.standard_normal(r1.shape))
    r2[np.isnan(r1).all(axis=1)] = np.nan                                    # the all-NaN items are NaN at both levels
    return full, r2, r1, cb_prev, cb, None


TIE_SEED = {16: 936, 32: 952, 64: 985}                                       # (at e = 64 draw 984 has no tied keeper for spill)


def ties(row):
    """Small integers: every product, sum and three-op update is exact in fp32.  finish / extend: K = 12 with rows 7 and 9 copies of
    row 3; three new items hold code 5 with the residual row cb[3] each, two more hold code 6 with one row.  spill:
    spill_cases.exact_ties_case's shape at this e."""
    r = gi.rs(TIE_SEED[row.e])
    e, nf = row.e, row.n_frozen
    if row.entry != "spill":
        K = row.ks[-1]
        cb = gi.f32(r.randint(-2, 3, size=(K, e)))
        cb[7], cb[9] = cb[3], cb[3]
        codes = [0, 1][:nf] + [5, 5, 5, 6, 6]
        one = gi.f32(r.randint(-2, 3, size=e))
        resid = gi.f32(np.stack([cb[3]] * 3 + [one] * 2))
        return _one_bucket(codes), resid, cb, None
    n = row.n
    cb_prev = gi.f32(r.randint(-2, 3, size=(6, e)))
    cb_prev[4], cb_prev[5] = cb_prev[1], cb_prev[2]
    cb_last = gi.f32(r.randint(-2, 3, size=(8, e)))
    cb_last[6], cb_last[7] = cb_last[2], cb_last[3]
    pool = gi.f32(r.randint(-2, 3, size=(5, e)))
    r2 = gi.f32(pool[r.randint(0, 5, size=n)])
    idx = np.stack([np.zeros(n, dtype=np.int64), r.randint(0, 4, size=n)], axis=1).astype(np.int64)
    idx[30:, 0] = 3
    r1 = three_op(r2, cb_prev[idx[:, 0]])
    return idx, r2[nf:], r1[nf:], cb_prev, cb_last, None


def out_of_range(row):
    """One listed group whose member list carries ids -5, -1, n, n + 3 and 2^40, over items whose code is -1, -9, K or K + 3 (spill:
    at either level)."""
    r = gi.rs(930 + row.e)
    e, nf, n = row.e, row.n_frozen, row.n
    everybody = [-5, -1] + list(range(n)) + [n, n + 3, 1 << 40]
    if row.entry != "spill":
        K = row.ks[-1]
        codes = [2, -1, 2, K, 4, 2, K + 3, 4, 4, -9, 7, 2]
        return _one_bucket(codes), gi.f32(r.standard_normal((n - nf, e))), gi.f32(r.standard_normal((K, e))), [everybody]
    K2, K1 = row.ks
    codes = [(0, 0), (0, 0), (0, 1), (0, 2), (0, 3), (0, 0), (0, K1), (0, -1), (K2, 0), (-2, 0), (0, 0), (1, 1), (0, K1), (0, 0),
             (0, K1 + 3)]
    idx = np.array(codes, dtype=np.int64)
    r2 = gi.f32(r.standard_normal((n, e)))
    cb2, cb1 = gi.f32(r.standard_normal((K2, e))), gi.f32(r.standard_normal((K1, e)))
    r1 = three_op(r2, cb2[np.clip(idx[:, 0], 0, K2 - 1)])

    def listing(now):
        """the shared tuples as they are -- items 6 and 12 share (0, K1) -- with bad ids around the first, and a group of bad codes"""
        found = groups_of(now)
        return [[-1] + found[0] + [n]] + found[1:] + [[6, 7, 8, 9, 1 << 40]], [everybody]
    return idx, r2, r1, cb2, cb1, listing


def four_listed(row):
    """Four listed groups of which the second is empty (equal offsets) and the others are touched: ks = [3, ..], prefixes 0, 1, 2
    with six new items each on three codes; extend and spill have one frozen item in front of each group, holding a code alone."""
    r = gi.rs(940 + row.e)
    e, nf = row.e, row.n_frozen
    per = 6
    prefix = np.concatenate([np.arange(nf) % 3, np.repeat(np.arange(3), per)])
    n = len(prefix)
    groups = [[int(i) for i in np.flatnonzero(prefix == p)] for p in range(3)]
    listed = [groups[0], [], groups[1], groups[2]]
    last = np.concatenate([np.full(nf, 5), r.randint(0, 3, size=n - nf)])
    if row.entry != "spill":
        idx = np.stack([prefix, last], axis=1).astype(np.int64)
        return idx, gi.f32(r.standard_normal((n - nf, e))), gi.f32(r.standard_normal((row.ks[-1], e))), listed
    K2, K1 = row.ks[-2:]
    idx = np.stack([prefix, np.zeros(n, dtype=np.int64), last], axis=1).astype(np.int64)
    r2 = gi.f32(r.standard_normal((n, e)))
    cb2, cb1 = gi.f32(r.standard_normal((K2, e))), gi.f32(r.standard_normal((K1, e)))
    r1 = three_op(r2, cb2[idx[:, 1]])

    def listing(now):
        found = groups_of(now)
        return (found[:1] + [[]] + found[1:] if found else []), listed       # (no shared tuple: no table, not one of no members)
    return idx, r2[nf:], r1[nf:], cb2, cb1, listing


def random_buckets(row):
    """Three buckets of about two thirds of K items each over the K codes (K = 1: four items each); extend: the first third of the
    items is frozen and collides within itself."""
    r = gi.rs(950 + row.e + row.ks[-1])
    idx = np.stack([r.randint(0, k, size=row.n) for k in row.ks], axis=1).astype(np.int64)
    resid = gi.f32(r.standard_normal((row.n, row.e)))
    return idx, resid[row.n_frozen:], gi.f32(r.standard_normal((row.ks[-1], row.e))), None


SKEW_SEED = {(300, 4): {16: 5, 32: 5, 64: 5}, (3, 300): {16: 800, 32: 800, 64: 800}}


def skewed_after_first_pass(row):
    """spill_cases.skewed_case after the finishing pass (finish_ref): what that pass leaves colliding is what spills."""
    idx, r2, r1, cb2, cb1 = sc.skewed_case(row.n, list(row.ks), row.e, SKEW_SEED[tuple(row.ks)][row.e])
    mid, _, _ = finish_ref(idx, r1, cb1)
    return mid, r2, r1, cb2, cb1, None


def chunk_walk(row):
    """One listed group of 600 members on 40 of 320 places -- codes 0 .. 39 of K = 320, or for spill cells (0 .. 3, 0 .. 9) of
    4 x 80 -- given to the pass as it stands: 280 free places for far more movers, so the last one goes in the second or third
    chunk of 256 positions, the movers behind it in that chunk are counted one by one, and a later chunk starts with none left.
    extend / spill with n_frozen = 100: the frozen boundary lies inside the first chunk."""
    r = gi.rs(960 + row.e)
    n, e, nf = row.n, row.e, row.n_frozen
    if row.entry != "spill":
        idx = r.randint(0, 40, size=(n, 1)).astype(np.int64)
        return idx, gi.f32(r.standard_normal((n - nf, e))), gi.f32(r.standard_normal((row.ks[-1], e))), None
    idx = np.stack([r.randint(0, 4, size=n), r.randint(0, 10, size=n)], axis=1).astype(np.int64)
    r2 = gi.f32(r.standard_normal((n, e)))
    cb2, cb1 = gi.f32(r.standard_normal((row.ks[0], e))), gi.f32(r.standard_normal((row.ks[1], e)))
    r1 = three_op(r2, cb2[idx[:, 0]])
    return idx, r2[nf:], r1[nf:], cb2, cb1, None


def straddle(row):
    """250 items on codes 0 .. 249 of K = 320, one each, and 30 more that hold codes of theirs: the movers sit at positions
    250 .. 279, on both sides of the first chunk's end.  finish (spill without frozen items): the 250 sit exactly on their code's
    row, so each keeps it; with n_frozen = 250 they are frozen."""
    r = gi.rs(970 + row.e)
    e, nf, K = row.e, row.n_frozen, row.ks[-1]
    codes = np.concatenate([np.arange(250), r.randint(0, 250, size=30)])
    cb = gi.f32(r.standard_normal((K, e)))
    resid = gi.f32(r.standard_normal((280, e)))
    resid[:250] = cb[:250]
    idx = _one_bucket(codes)
    if row.entry == "spill":
        return _as_spill(idx, resid[nf:], cb, row, r)
    return idx, resid[nf:], cb, None


def frozen_small(row):
    """Two listed groups.  Prefix 0: three frozen items on one code (tuple) and nobody else.  Prefix 1: frozen item 3 and the new
    items 4 and 5 on code 2, item 4's residual exactly that code's row -- it moves all the same -- and new item 6 alone on code 5."""
    r = gi.rs(980 + row.e)
    e = row.e
    pairs = [(0, 3), (0, 3), (0, 3), (1, 2), (1, 2), (1, 2), (1, 5)]
    cb = gi.f32(r.standard_normal((row.ks[-1], e)))
    resid = gi.f32(r.standard_normal((3, e)))
    resid[0] = cb[2]
    if row.entry != "spill":
        return np.array(pairs, dtype=np.int64), resid, cb, [[0, 1, 2], [3, 4, 5, 6]]
    idx = np.array([(p, 1, k) for p, k in pairs], dtype=np.int64)
    cb2 = gi.f32(r.standard_normal((row.ks[-2], e)))
    r2 = gi.f32(r.standard_normal((3, e)))
    listing = lambda now: (groups_of(now), [[0, 1, 2], [3, 4, 5, 6]])
    return idx, r2, resid, cb2, cb, listing


def over_64(row):
    """K2 = 6, K1 = 40.  Tuple (0, 5) is held by 65 items, (1, 7) by 150 and (2, 2) by 3, ids interleaved; the residual that sits
    exactly on the shared code's row is the 65th holder's, and the 101st's: both keepers lie past the first 64 holders.  240 cells
    for 218 items, and three tuple groups: the keepers' only workgroup has an idle wave."""
    r = gi.rs(990 + row.e)
    e, n = row.e, row.n
    K2, K1 = row.ks
    which = r.permutation(np.repeat([0, 1, 2], [65, 150, 3]))
    idx = np.array([[(0, 5), (1, 7), (2, 2)][w] for w in which], dtype=np.int64)
    cb2, cb1 = gi.f32(r.standard_normal((K2, e))), gi.f32(r.standard_normal((K1, e)))
    r2 = gi.f32(r.standard_normal((n, e)))
    r1 = three_op(r2, cb2[idx[:, 0]])
    r1[np.flatnonzero(which == 0)[64]] = cb1[5]
    r1[np.flatnonzero(which == 1)[100]] = cb1[7]
    return idx, r2, r1, cb2, cb1, None


def largest_level(row):
    """The largest K the entry admits: one bucket of about 1.2 K items on the first K / 2 codes; extend: K / 8 of them frozen."""
    r = gi.rs(1000 + row.e)
    K = row.ks[-1]
    idx = _one_bucket(r.randint(0, K // 2, size=row.n))
    resid = gi.f32(r.standard_normal((row.n - row.n_frozen, row.e)))
    return idx, resid, gi.f32(r.standard_normal((K, row.e))), None


# ---- inputs, tables and the reference of a row: computed once, shared, read only --------------------------------------------------
def groups_of(rows):
    """Lists of the item ids sharing a row of `rows` (two or more holders), first-occurrence order, ids ascending -- what
    lcrec_collision_groups lists; no columns: one group of all items."""
    found = {}
    for i in range(len(rows)):
        found.setdefault(tuple(rows[i]), []).append(i)
    return [g for g in found.values() if len(g) >= 2]


@functools.lru_cache(maxsize=None)
def inputs(row):
    names = ("idx", "r2", "r1", "cb_prev", "cb_last", "listing") if row.entry == "spill" else ("idx", "resid", "cb", "buckets")
    inp = dict(zip(names, row.builder(row)))
    assert inp["idx"].shape == (row.n, len(row.ks)) and inp["idx"].dtype == np.int64, row_id(row)
    for a in inp.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return inp


def tables(row, idx):
    """The listed tables of a call on `idx`: the buckets (finish, extend), or (tuple groups, super-buckets) (spill)."""
    inp = inputs(row)
    L = idx.shape[1]
    if row.entry != "spill":
        return inp["buckets"] if inp["buckets"] is not None else groups_of(idx[:, :L - 1])
    if inp["listing"] is not None:
        return inp["listing"](idx)
    return groups_of(idx), groups_of(idx[:, :L - 2])


def run_reference(row, idx):
    inp = inputs(row)
    if row.entry == "finish":
        new, served, unres = finish_ref(idx, inp["resid"], inp["cb"], buckets=tables(row, idx))
    elif row.entry == "extend":
        new, served, unres = extend_ref(idx, row.n_frozen, inp["resid"], inp["cb"], buckets=tables(row, idx))
    else:
        tg, sg = tables(row, idx)
        new, served, unres = spill_ref(idx, row.n_frozen, inp["r2"], inp["r1"], inp["cb_prev"], inp["cb_last"], tg, sg)
    new.setflags(write=False)
    return Result(new, tuple(int(i) for i in served), int(unres), len(served) - int(unres))


@functools.lru_cache(maxsize=None)
def reference(row):
    return run_reference(row, inputs(row)["idx"])


@functools.lru_cache(maxsize=None)
def reference_again(row):
    """the reference applied to its own output, with tables built from that output"""
    return run_reference(row, reference(row).idx)


# ---- what the predicates look at ---------------------------------------------------------------------------------------------------
def _dist(x, cb):
    """raw fp32 distances of one row to every code, NaN kept"""
    return cpu_oracle.distances(np.ascontiguousarray(x, dtype=np.float32).reshape(1, -1), cb)[0]


def _last(row, inp):
    """(the residual rows entering the last level, the last codebook)"""
    return (inp["r1"], inp["cb_last"]) if row.entry == "spill" else (inp["resid"], inp["cb"])


def _takes_part(row, inp, i):
    idx, n = inp["idx"], row.n
    if not 0 <= i < n or not 0 <= idx[i, -1] < row.ks[-1]:
        return False
    return row.entry != "spill" or 0 <= idx[i, -2] < row.ks[-2]


def _groups(row, inp):
    """the listed groups a workgroup walks: the buckets, or the super-buckets"""
    t = tables(row, inp["idx"])
    return t[1] if row.entry == "spill" else t


def _place(row, tup):
    return (int(tup[-2]), int(tup[-1])) if row.entry == "spill" else int(tup[-1])


def contests(row, inp):
    """[(shared last code, holders ascending)] of the given tuples: per bucket and code, or per listed tuple group"""
    idx, out = inp["idx"], []
    if row.entry == "spill":
        for g in tables(row, idx)[0]:
            h = [int(i) for i in g if _takes_part(row, inp, int(i))]
            if len(h) >= 2:
                out.append((int(idx[h[0], -1]), h))
        return out
    for b in tables(row, idx):
        held = {}
        for i in b:
            if _takes_part(row, inp, int(i)):
                held.setdefault(int(idx[int(i), -1]), []).append(int(i))
        out += [(k, h) for k, h in held.items() if len(h) >= 2]
    return out


def keeper_contests(row, inp, res):
    """[(code, holders, their raw own-code distances, keeper)] of the contests without a frozen holder"""
    rows, cb = _last(row, inp)
    served, out = set(res.served), []
    for k, h in contests(row, inp):
        if h[0] < row.n_frozen:
            continue
        keeper = [i for i in h if i not in served]
        assert len(keeper) == 1
        out.append((k, h, [_dist(rows[i - row.n_frozen], cb)[k] for i in h], keeper[0]))
    return out


def timeline(row, inp, res):
    """One Step per served mover, in served order: its id, the listed group that serves it and its position there, the places free
    before it was served (bool [K], or [K2, K1] for spill) and the place it took (a code, or (a, k); None: unresolved).
    Rebuilt from the inputs and the result alone."""
    idx = inp["idx"]
    shape = tuple(row.ks[-2:]) if row.entry == "spill" else (row.ks[-1],)
    where, free = {}, []
    for g, listed in enumerate(_groups(row, inp)):
        occupied = np.zeros(shape, dtype=bool)
        for pos, i in enumerate(listed):
            if _takes_part(row, inp, int(i)):
                occupied[_place(row, idx[int(i)])] = True
                where[int(i)] = (g, pos)
        free.append(~occupied)
    steps = []
    for i in res.served:
        g, pos = where[i]
        moved = not np.array_equal(res.idx[i], idx[i])
        taken = _place(row, res.idx[i]) if moved else None
        steps.append(Step(i, g, pos, free[g].copy(), taken))
        if moved:
            assert free[g][taken]
            free[g][taken] = False
    return steps


def _moved_in(steps, g):
    return [s for s in steps if s.group == g and s.taken is not None]


# ---- the properties ---------------------------------------------------------------------------------------------------------------
def keeper_negative_distance(row, inp, res):
    """One contested code has three or more holders whose own-code distances are negative and pairwise distinct, and another has
    contenders of both signs: the `~u` branch of ordered_bits decides a keeper."""
    found = keeper_contests(row, inp, res)
    deep = {k for k, h, d, _ in found if len({float(x) for x in d if x < 0}) >= 3}
    mixed = {k for k, h, d, _ in found if any(x < 0 for x in d) and any(x > 0 for x in d)}
    return any(a != b for a in deep for b in mixed)


def keeper_nan(row, inp, res):
    """A holder with a NaN distance loses its code to a finite holder with a higher id; and a code whose holders are all NaN goes
    to the lowest id."""
    found = keeper_contests(row, inp, res)
    loses = any(np.isnan(d[0]) and not np.isnan(d[h.index(keeper)]) and keeper > h[0] for k, h, d, keeper in found)
    lowest = any(np.isnan(d).all() and len(h) >= 3 and keeper == h[0] for k, h, d, keeper in found)
    return loses and lowest


def mover_nan(row, inp, res):
    """A mover whose row is all NaN takes the lowest free code -- for spill the lowest row with room, then its lowest free cell --
    and that is not the very first place."""
    rows = inp["r2"] if row.entry == "spill" else inp["resid"]
    for s in timeline(row, inp, res):
        if s.taken is None or not np.isnan(rows[s.id - row.n_frozen]).all():
            continue
        if row.entry == "spill":
            a = int(np.flatnonzero(s.free.any(axis=1))[0])
            if a > 0 and s.taken == (a, int(np.flatnonzero(s.free[a])[0])) and np.isnan(inp["r1"][s.id - row.n_frozen]).all():
                return True
        elif s.taken == int(np.flatnonzero(s.free)[0]) > 0:
            return True
    return False


def code_row_inf(row, inp, res):
    """A codebook row with a +inf element (spill: one at each level) is free throughout, finite movers are served past it, and
    nobody takes it."""
    steps = timeline(row, inp, res)
    rows = inp["r2"] if row.entry == "spill" else inp["resid"]
    finite = [s for s in steps if s.taken is not None and np.isfinite(rows[s.id - row.n_frozen]).all()]
    if not finite or res.unresolved:
        return False
    bad_last = np.flatnonzero(np.isposinf(_last(row, inp)[1]).any(axis=1))
    if bad_last.size == 0:
        return False
    if row.entry != "spill":
        return all(s.free[bad_last].all() and s.taken not in bad_last for s in steps)
    bad_prev = np.flatnonzero(np.isposinf(inp["cb_prev"]).any(axis=1))
    return bad_prev.size > 0 and all(s.free[bad_prev].all() and s.taken[0] not in bad_prev and s.taken[1] not in bad_last
                                     for s in steps)


def keeper_exact_tie(row, inp, res):
    """A code's nearest holders tie exactly, and the lowest id among them keeps it."""
    for k, h, d, keeper in keeper_contests(row, inp, res):
        tied = [i for i, x in zip(h, d) if x == min(d)]
        if len(tied) >= 2 and keeper == tied[0]:
            return True
    return False


def free_exact_tie(row, inp, res):
    """A mover's nearest free places tie exactly, and it takes the lowest (spill: among the rows with room, and among the cells)."""
    nf = row.n_frozen
    rows_tie = cells_tie = False
    for s in timeline(row, inp, res):
        if s.taken is None:
            continue
        if row.entry != "spill":
            d = _dist(inp["resid"][s.id - nf], inp["cb"])
            tied = [k for k in np.flatnonzero(s.free) if d[k] == d[s.taken]]
            if len(tied) >= 2 and s.taken == tied[0]:
                return True
            continue
        a, k = s.taken
        d2 = _dist(inp["r2"][s.id - nf], inp["cb_prev"])
        tied = [b for b in np.flatnonzero(s.free.any(axis=1)) if d2[b] == d2[a]]
        rows_tie |= len(tied) >= 2 and a == tied[0]
        d1 = _dist(three_op(inp["r2"][s.id - nf], inp["cb_prev"][a]), inp["cb_last"])
        tied = [c for c in np.flatnonzero(s.free[a]) if d1[c] == d1[k]]
        cells_tie |= len(tied) >= 2 and k == tied[0]
    return rows_tie and cells_tie


def out_of_range_members(row, inp, res):
    """The listed members carry ids below 0, from n on and past 2^32, and items whose code is below 0, K and past K (spill: at both
    levels, and in both tables); none of those is written, and the others are served."""
    idx, n = inp["idx"], row.n
    t = tables(row, idx)
    for table in (t if row.entry == "spill" else (t,)):
        ids = [int(i) for g in table for i in g]
        if not (any(i < 0 for i in ids) and any(n <= i < 1 << 32 for i in ids)):
            return False
    ids = [int(i) for g in _groups(row, inp) for i in g]
    if not any(i >= 1 << 32 for i in ids):
        return False
    inside = [i for i in ids if 0 <= i < n]
    for col in ((-2, -1) if row.entry == "spill" else (-1,)):
        K = row.ks[col]
        if not (any(idx[i, col] < 0 for i in inside) and any(idx[i, col] == K for i in inside)):
            return False
    if not any(idx[i, -1] > row.ks[-1] for i in inside):
        return False
    out = [i for i in inside if not _takes_part(row, inp, i)]
    return res.moved > 0 and np.array_equal(res.idx[out], idx[out])


def empty_bucket_listed(row, inp, res):
    """Four listed groups: the second is empty, each of the others serves a mover (spill: the tuple table has an empty group too)."""
    listed = _groups(row, inp)
    steps = timeline(row, inp, res)
    if row.entry == "spill" and [] not in tables(row, inp["idx"])[0]:
        return False
    return len(listed) == 4 and list(listed[1]) == [] and all(_moved_in(steps, g) for g in (0, 2, 3))


def _trips(K):
    def prop(row, inp, res):
        if row.entry == "spill" or row.ks[-1] != K:
            return False
        taken = [s.taken for s in timeline(row, inp, res) if s.taken is not None]
        if K == 1:
            return res.moved == 0 and res.unresolved > 0
        low = {1: 0, 48: 32, 256: 192, 320: 256}[K]
        return any(k >= low for k in taken)
    return prop


code_trips_1 = _trips(1)
code_trips_1.__doc__ = "K = 1: nothing is ever free, every mover is unresolved."
code_trips_48 = _trips(48)
code_trips_48.__doc__ = "K = 48, below a wave and no multiple of 32: a mover takes a code from 32 on."
code_trips_256 = _trips(256)
code_trips_256.__doc__ = "K = 256, exactly one code per thread: a mover takes a code of the last wave."
code_trips_320 = _trips(320)
code_trips_320.__doc__ = "K = 320, a second trip over the codes: a mover takes a code from 256 on."


def code_trips_cells_300(row, inp, res):
    """spill with K1 = 300: a second trip over the cells and twelve valid bits in a row's tenth occupancy word; movers take cells
    from 256 on and from 288 on."""
    if row.entry != "spill" or row.ks[-1] != 300:
        return False
    cells = [s.taken[1] for s in timeline(row, inp, res) if s.taken is not None]
    return any(256 <= k < 288 for k in cells) and any(k >= 288 for k in cells)


def code_trips_rows_300(row, inp, res):
    """spill with K2 = 300: a second trip over the rows in round 1, and fre[a] owned by thread a & 255 for a >= 256: at least 16
    served movers take a row from 256 on, and all are resolved."""
    if row.entry != "spill" or row.ks[-2] != 300:
        return False
    return res.unresolved == 0 and sum(1 for s in timeline(row, inp, res) if s.taken is not None and s.taken[0] >= 256) >= 16


def keepers_over_64_holders(row, inp, res):
    """spill: one tuple with 65 or more holders and another with 150 or more, each keeper at a position from 64 on in its group (the
    lane loops' second and third trips decide); room for every member, and a number of tuple groups that is no multiple of 4."""
    if row.entry != "spill":
        return False
    found = keeper_contests(row, inp, res)
    deep = sorted(len(h) for k, h, d, keeper in found if h.index(keeper) >= 64)
    return (len(deep) >= 2 and deep[-1] >= 150 and deep[-2] >= 65 and deep[-2] < 128 and res.unresolved == 0
            and len(tables(row, inp["idx"])[0]) % 4 != 0 and row.ks[-2] * row.ks[-1] >= row.n)


def walk_straddles_chunk(row, inp, res):
    """Consecutive movers of one group are served on both sides of position 256."""
    steps = timeline(row, inp, res)
    for g in {s.group for s in steps}:
        pos = [s.pos for s in _moved_in(steps, g)]
        if any(CHUNK - 8 <= p < CHUNK for p in pos) and any(CHUNK <= p < CHUNK + 8 for p in pos):
            return True
    return False


def _run_out(steps, g):
    """(chunk of the group's last served mover, positions of its unresolved movers) -- None when nobody is unresolved"""
    moved = [s.pos for s in _moved_in(steps, g)]
    late = [s.pos for s in steps if s.group == g and s.taken is None]
    if not moved or not late:
        return None
    return max(moved) // CHUNK, late


def walk_runs_out_mid_chunk(row, inp, res):
    """The last free place goes inside a chunk after the first, and movers behind it in that chunk are counted one by one."""
    steps = timeline(row, inp, res)
    for g in {s.group for s in steps}:
        out = _run_out(steps, g)
        if out and out[0] >= 1 and any(p // CHUNK == out[0] for p in out[1]):
            return True
    return False


def walk_whole_chunk_counted(row, inp, res):
    """A chunk behind the one in which the free places ran out holds movers: it starts with none left and is counted in parallel."""
    steps = timeline(row, inp, res)
    for g in {s.group for s in steps}:
        out = _run_out(steps, g)
        if out and sum(1 for p in out[1] if p // CHUNK > out[0]) >= 2:
            return True
    return False


def frozen_holder_beats_nearest(row, inp, res):
    """A new item whose nearest code of all is its own shares it with a frozen holder, and moves."""
    rows, cb = _last(row, inp)
    steps = {s.id: s for s in timeline(row, inp, res)}
    for k, h in contests(row, inp):
        if h[0] >= row.n_frozen:
            continue
        for i in h:
            if i >= row.n_frozen and i in steps and steps[i].taken is not None:
                d = _dist(rows[i - row.n_frozen], cb)
                if d[k] == np.nanmin(d) and (d == d[k]).sum() == 1:
                    return True
    return False


def frozen_only_bucket_listed(row, inp, res):
    """A listed group of frozen items that share a code (spill: a listed tuple group of frozen holders too) stays as it is beside a
    group that serves a mover."""
    listed = _groups(row, inp)
    steps = timeline(row, inp, res)
    idx = inp["idx"]
    if row.entry == "spill" and not any(len(g) >= 2 and max(g) < row.n_frozen for g in tables(row, idx)[0]):
        return False
    for g, members in enumerate(listed):
        if len(members) >= 2 and max(members) < row.n_frozen and len({tuple(idx[i]) for i in members}) < len(members):
            return np.array_equal(res.idx[members], idx[members]) and any(_moved_in(steps, h) for h in range(len(listed)) if h != g)
    return False


def frozen_boundary_inside_chunk(row, inp, res):
    """n_frozen falls inside a chunk of a group: frozen members and served movers share those 256 positions."""
    steps = timeline(row, inp, res)
    for g, members in enumerate(_groups(row, inp)):
        first_new = next((pos for pos, i in enumerate(members) if i >= row.n_frozen), None)
        if first_new and first_new % CHUNK and any(s.pos // CHUNK == first_new // CHUNK for s in _moved_in(steps, g)):
            return True
    return False


def _largest(entry):
    def prop(row, inp, res):
        K = row.ks[-1]
        taken = [s.taken for s in timeline(row, inp, res) if s.taken is not None]
        return (row.entry == entry and len(row.ks) == 2 and K == LARGEST[entry][row.e] and len(res.served) > K // 4
                and res.unresolved > 0 and any(k >= K - K % CHUNK for k in taken) and len(_groups(row, inp)) == 1)
    prop.__doc__ = (f"The largest last level lcrec_{entry}_nearest_free admits at this e and L = 2: more than K / 4 movers, a walk of "
                    "every code trip up to the last, ragged one, and some movers left unresolved.")
    return prop


largest_level_finish = _largest("finish")
largest_level_extend = _largest("extend")

PROPERTIES = {
    "keeper_negative_distance": keeper_negative_distance, "keeper_nan": keeper_nan, "mover_nan": mover_nan,
    "code_row_inf": code_row_inf, "keeper_exact_tie": keeper_exact_tie, "free_exact_tie": free_exact_tie,
    "out_of_range_members": out_of_range_members, "empty_bucket_listed": empty_bucket_listed,
    "code_trips_1": code_trips_1, "code_trips_48": code_trips_48, "code_trips_256": code_trips_256,
    "code_trips_320": code_trips_320, "code_trips_cells_300": code_trips_cells_300, "code_trips_rows_300": code_trips_rows_300,
    "keepers_over_64_holders": keepers_over_64_holders, "walk_straddles_chunk": walk_straddles_chunk,
    "walk_runs_out_mid_chunk": walk_runs_out_mid_chunk, "walk_whole_chunk_counted": walk_whole_chunk_counted,
    "frozen_holder_beats_nearest": frozen_holder_beats_nearest, "frozen_only_bucket_listed": frozen_only_bucket_listed,
    "frozen_boundary_inside_chunk": frozen_boundary_inside_chunk,
    "largest_level_finish": largest_level_finish, "largest_level_extend": largest_level_extend,
}
REQUIRED = frozenset(PROPERTIES)
PER_ENTRY = ("largest_level_finish", "largest_level_extend")                 # one row per entry and e; every other: some row per e

# the wrong rule of tests/nearest_free_mutants.py that each property's rows must refuse, and the entries it applies to
MUTANT_OF = {
    "M1": (("keeper_negative_distance",), ("finish", "extend", "spill")),
    "M2": (("keeper_nan",), ("finish", "extend", "spill")),
    "M3": (("keeper_exact_tie", "free_exact_tie"), ("finish", "extend", "spill")),
    "M4": (("code_trips_cells_300", "code_trips_rows_300"), ("spill",)),
    "M5": (("keepers_over_64_holders",), ("spill",)),
    "M6": (("out_of_range_members",), ("finish", "extend", "spill")),
    "M7": (("walk_whole_chunk_counted",), ("finish", "extend", "spill")),
}


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def _rows():
    rows = []
    for e in ES:
        for entry, nf in (("finish", 0), ("extend", 4)):
            add = lambda ks, n, n_frozen, builder, *covers: rows.append(Row(entry, e, tuple(ks), n, n_frozen, builder, covers))
            fz = entry == "extend"
            add([24], 40 + nf, nf, negative, "keeper_negative_distance")
            add([2, 16], 10 + nf // 2, nf // 2, nan_inf, "keeper_nan", "mover_nan", "code_row_inf")
            add([2, 12], 5 + nf // 2, nf // 2, ties, "keeper_exact_tie", "free_exact_tie")
            add([2, 12], 12, 5 if fz else 0, out_of_range, "out_of_range_members")
            add([3, 12], 18 + (3 if fz else 0), 3 if fz else 0, four_listed, "empty_bucket_listed")
            add([3, 1], 12, 4 if fz else 0, random_buckets, "code_trips_1")
            add([3, 48], 96, 32 if fz else 0, random_buckets, "code_trips_48")
            add([3, 256], 512, 170 if fz else 0, random_buckets, "code_trips_256")
            add([320], 600, 100 if fz else 0, chunk_walk, "code_trips_320", "walk_runs_out_mid_chunk", "walk_whole_chunk_counted",
                *(("frozen_boundary_inside_chunk",) if fz else ()))
            add([2, 320], 280, 250 if fz else 0, straddle, "walk_straddles_chunk", *(("frozen_boundary_inside_chunk",) if fz else ()))
            if fz:
                add([2, 12], 7, 4, frozen_small, "frozen_holder_beats_nearest", "frozen_only_bucket_listed")
            K = LARGEST[entry][e]
            n = K + K // 5
            add([2, K], n, K // 8 if fz else 0, largest_level, "largest_level_" + entry)
        add = lambda ks, n, n_frozen, builder, *covers: rows.append(Row("spill", e, tuple(ks), n, n_frozen, builder, covers))
        add([3, 24], 40, 0, negative, "keeper_negative_distance")
        add([4, 16], 26, 0, nan_inf, "keeper_nan", "mover_nan", "code_row_inf")
        add([6, 8], 40, 0, ties, "keeper_exact_tie", "free_exact_tie")
        add([3, 4], 15, 0, out_of_range, "out_of_range_members")
        add([3, 4, 6], 21, 3, four_listed, "empty_bucket_listed")
        add([3, 300], 700, 0, skewed_after_first_pass, "code_trips_cells_300")
        add([300, 4], 700, 0, skewed_after_first_pass, "code_trips_rows_300")
        add([6, 40], 218, 0, over_64, "keepers_over_64_holders")
        add([4, 80], 600, 0, chunk_walk, "walk_runs_out_mid_chunk", "walk_whole_chunk_counted")
        add([4, 80], 600, 100, chunk_walk, "walk_runs_out_mid_chunk", "walk_whole_chunk_counted", "frozen_boundary_inside_chunk")
        add([2, 320], 280, 0, straddle, "walk_straddles_chunk")
        add([2, 320], 280, 250, straddle, "walk_straddles_chunk", "frozen_boundary_inside_chunk")
        add([2, 3, 12], 7, 4, frozen_small, "frozen_holder_beats_nearest", "frozen_only_bucket_listed")
    return rows


def row_id(row):
    return f"{row.entry}-e{row.e}-{row.builder.__name__}-{'_'.join(map(str, row.ks))}-n{row.n}-f{row.n_frozen}"


ROWS = _rows()
