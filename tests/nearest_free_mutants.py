"""The three nearest-free rules of include/lcrec.h (lcrec_finish_nearest_free, lcrec_extend_nearest_free, lcrec_spill_nearest_free)
once more in numpy, with a switch that applies ONE wrong rule: what a subtly wrong kernel would compute.  With mutant=None the two
functions restate tests/finish_ref.py, extend_ref.py and spill_ref.py (tests/test_nearest_free_cases_host.py proves that on every
row of the case table); with a mutant they must differ from them on every row that claims the matching property, which proves that
the bit-exact judge of tests/test_gpu_nearest_free_forms.py would refuse such a kernel.

  M1  the keeper is chosen by the raw unsigned bits of d (a negative d loses to every positive one, and to a less negative one)
  M2  a NaN is not turned into +inf: it wins an argmin
  M3  ties go to the highest id / the highest code
  M4  rows and codes >= 256 are never candidates (one trip over the codes per thread)
  M5  the spill keepers look at the first 64 holders of a tuple only
  M6  an out-of-range code is clamped into range and its item counted as a holder
  M7  movers of the chunks (256 positions of the listed group) that start with no free place left are not counted as unresolved

Tables are always given (lists of item-id lists, as a caller would pass them to the entry); a mover's position is its index in the
listed group.  -> (new idx int64, served ids in order, unresolved, moved)."""
import numpy as np

from oracle import cpu_oracle

MUTANTS = ("M1", "M2", "M3", "M4", "M5", "M6", "M7")
CHUNK = 256


def _d(x, cb):
    """raw fp32 distances of one row to every code (NaN kept)"""
    return cpu_oracle.distances(np.ascontiguousarray(x, dtype=np.float32).reshape(1, -1), cb)[0]


def _pick(d, mutant, keeper=False):
    """position of the winner among the distances d"""
    d = np.asarray(d, dtype=np.float32)
    d = np.where(np.isnan(d), np.float32(-np.inf if mutant == "M2" else np.inf), d).astype(np.float32)
    key = d.view(np.uint32) if (keeper and mutant == "M1") else d
    best = np.flatnonzero(key == key.min())
    return int(best[-1] if mutant == "M3" else best[0])


def _three_op(r, c):
    t = c - r
    s = r + t
    return (r - s).astype(np.float32)


def _code(c, K, mutant):
    """the code an item takes part with, or None"""
    c = int(c)
    if mutant == "M6":
        return min(max(c, 0), K - 1)
    return c if 0 <= c < K else None


def _walk(listed_movers, free_left, serve, mutant):
    """The movers of one listed group, (position, id) ascending, a chunk of 256 positions at a time.  serve(id) -> True when the
    mover took a place.  -> (served ids, unresolved, moved)."""
    served, unresolved, moved = [], 0, 0
    chunk, counted = -1, True
    for pos, i in listed_movers:
        if pos // CHUNK != chunk:
            chunk = pos // CHUNK
            counted = not (mutant == "M7" and free_left == 0)            # a chunk that starts with nothing left
        served.append(i)
        if free_left == 0:
            unresolved += counted
            continue
        if serve(i):
            moved += 1
            free_left -= 1
        else:                                                               # (M4 only: places are left, none is a candidate)
            unresolved += 1
    return served, unresolved, moved


def nearest_free(idx, n_frozen, resid_new, cb, buckets, mutant=None):
    """lcrec_extend_nearest_free's rule (n_frozen = 0: lcrec_finish_nearest_free's)."""
    idx = np.array(idx, dtype=np.int64)
    n, L = idx.shape
    K, nf = cb.shape[0], int(n_frozen)
    served_all, unresolved, moved = [], 0, 0
    for listed in buckets:
        part = [(pos, int(i), _code(idx[int(i), L - 1], K, mutant)) for pos, i in enumerate(listed) if 0 <= int(i) < n]
        part = [(pos, i, c) for pos, i, c in part if c is not None]
        holders = {}
        for pos, i, c in part:
            holders.setdefault(c, []).append(i)
        movers = set()
        for k, h in holders.items():
            fresh = [i for i in h if i >= nf]
            if len(h) < 2 or not fresh:
                continue
            if len(fresh) < len(h):                                         # a frozen holder: every new holder moves
                movers.update(fresh)
                continue
            keeper = fresh[_pick([_d(resid_new[i - nf], cb)[k] for i in fresh], mutant, keeper=True)]
            movers.update(i for i in fresh if i != keeper)
        if not movers:
            continue
        occupied = np.zeros(K, dtype=bool)
        occupied[list(holders)] = True

        def serve(i):
            free = np.flatnonzero(~occupied)
            if mutant == "M4":
                free = free[free < CHUNK]
                if free.size == 0:
                    return False
            k = int(free[_pick(_d(resid_new[i - nf], cb)[free], mutant)])
            idx[i, L - 1] = k
            occupied[k] = True
            return True

        s, u, m = _walk([(pos, i) for pos, i, c in part if i in movers], int((~occupied).sum()), serve, mutant)
        served_all += s
        unresolved += u
        moved += m
    return idx, served_all, unresolved, moved


def spill(idx, n_frozen, r2_new, r1_new, cb_prev, cb_last, tuple_groups, super_groups, mutant=None):
    """lcrec_spill_nearest_free's rule."""
    idx = np.array(idx, dtype=np.int64)
    n, L = idx.shape
    K2, K1, nf = cb_prev.shape[0], cb_last.shape[0], int(n_frozen)

    def codes(i):
        if not 0 <= i < n:
            return None
        a, c = _code(idx[i, L - 2], K2, mutant), _code(idx[i, L - 1], K1, mutant)
        return None if a is None or c is None else (a, c)

    movers = set()
    for listed in tuple_groups:
        h = [int(i) for i in listed if codes(int(i)) is not None]
        if mutant == "M5":
            h = h[:64]
        fresh = [i for i in h if i >= nf]
        if len(h) < 2 or not fresh:
            continue
        if len(fresh) < len(h):
            movers.update(fresh)
            continue
        keeper = fresh[_pick([_d(r1_new[i - nf], cb_last)[codes(i)[1]] for i in fresh], mutant, keeper=True)]
        movers.update(i for i in (int(j) for j in listed) if codes(i) is not None and i >= nf and i != keeper)
    served_all, unresolved, moved = [], 0, 0
    for listed in super_groups:
        part = [(pos, int(i)) for pos, i in enumerate(listed) if codes(int(i)) is not None]
        mine = [(pos, i) for pos, i in part if i in movers]
        if not mine:
            continue
        occupied = np.zeros((K2, K1), dtype=bool)
        for pos, i in part:
            occupied[codes(i)] = True

        def serve(i):
            rows = np.flatnonzero(~occupied.all(axis=1))
            if mutant == "M4":
                rows = np.array([a for a in rows if a < CHUNK and not occupied[a, :CHUNK].all()], dtype=np.int64)
                if rows.size == 0:
                    return False
            r2 = r2_new[i - nf]
            a = int(rows[_pick(_d(r2, cb_prev)[rows], mutant)])
            free = np.flatnonzero(~occupied[a])
            if mutant == "M4":
                free = free[free < CHUNK]
            k = int(free[_pick(_d(_three_op(r2, cb_prev[a]), cb_last)[free], mutant)])
            idx[i, L - 2], idx[i, L - 1] = a, k
            occupied[a, k] = True
            return True

        s, u, m = _walk(mine, int((~occupied).sum()), serve, mutant)
        served_all += s
        unresolved += u
        moved += m
    return idx, served_all, unresolved, moved
