"""The spill rule of lcrec_spill_nearest_free (include/lcrec.h) in numpy, on the oracle's distances: written from the rule's text,
not from the kernel.  d = oracle.distances (xx, cc, dot as fp32 fma chains; d = (xx + cc) - 2 dot); a NaN counts as +inf wherever
distances are compared; np.argmin takes the first minimum.  Level L-2 has codebook cb_prev (K2 codes) and the residual r2 entering
it; the last level has cb_last (K1 codes) and r1."""
import numpy as np

from oracle import cpu_oracle


def three_op(r, c):
    """The residual behind code row c, as rq_assign and the oracle compute it (oracle/lcrec_oracle.c:33): three fp32 operations
    per element."""
    r, c = np.asarray(r, dtype=np.float32), np.asarray(c, dtype=np.float32)
    t = c - r
    s = r + t
    return (r - s).astype(np.float32)


def _d(x, cb):
    d = cpu_oracle.distances(np.ascontiguousarray(x, dtype=np.float32).reshape(1, -1), cb)[0]
    return np.where(np.isnan(d), np.float32(np.inf), d)


def spill_ref(idx, n_frozen, resid_prev_new, resid_last_new, cb_prev, cb_last, tuple_groups=None, super_groups=None):
    """idx int [N, L], L >= 2; items below n_frozen are frozen; resid_prev_new / resid_last_new [N - n_frozen, e] hold the rows of
    the new items only (r2 and r1); cb_prev [K2, e], cb_last [K1, e].
    tuple_groups / super_groups: None = the items sharing the full tuple / sharing idx[:, :L-2]; or lists of item-id lists as a
    caller would pass them to the entry -- a member whose id is outside [0, N) or whose code of level L-2 or L-1 is out of range
    takes no part.
    -> (new idx int64 [N, L], mover ids in the order they were served, unresolved)."""
    idx = np.array(idx, dtype=np.int64)
    n, L = idx.shape
    assert L >= 2
    K2, K1 = cb_prev.shape[0], cb_last.shape[0]
    nf = int(n_frozen)

    def takes_part(i):
        return 0 <= i < n and 0 <= idx[i, L - 2] < K2 and 0 <= idx[i, L - 1] < K1

    # 1. movers: of every full tuple held by two or more items
    if tuple_groups is None:
        found = {}
        for i in range(n):
            found.setdefault(tuple(idx[i]), []).append(i)
        tuple_groups = [g for g in found.values() if len(g) >= 2]
    movers = set()
    for listed in tuple_groups:
        holders = sorted(int(i) for i in listed if takes_part(int(i)))
        if len(holders) < 2:
            continue
        new = [i for i in holders if i >= nf]
        if len(new) < len(holders):                                         # a frozen holder: every new holder moves
            movers.update(new)
            continue
        d = [_d(resid_last_new[i - nf], cb_last)[idx[i, L - 1]] for i in new]
        keeper = new[int(np.argmin(d))]                                     # smallest d(r1, C1[k]); a tie goes to the lowest id
        movers.update(i for i in new if i != keeper)

    # 2. super-buckets: frozen and new items together
    if super_groups is None:
        found = {}
        for i in range(n):
            found.setdefault(tuple(idx[i, :L - 2]), []).append(i)
        super_groups = list(found.values())
    served, unresolved = [], 0
    for listed in super_groups:
        members = sorted(int(i) for i in listed if takes_part(int(i)))
        mine = [i for i in members if i in movers]
        if not mine:
            continue                                                        # not touched
        occupied = np.zeros((K2, K1), dtype=bool)
        for i in members:
            occupied[idx[i, L - 2], idx[i, L - 1]] = True
        # 3. movers in ascending id
        for i in mine:
            served.append(i)
            rows = np.flatnonzero(~occupied.all(axis=1))                    # the codes a' whose row still has a free cell
            if rows.size == 0:
                unresolved += 1                                             # this one and all later ones keep their tuple
                continue
            r2 = resid_prev_new[i - nf]
            a = int(rows[np.argmin(_d(r2, cb_prev)[rows])])
            r = three_op(r2, cb_prev[a])
            free = np.flatnonzero(~occupied[a])
            k = int(free[np.argmin(_d(r, cb_last)[free])])
            idx[i, L - 2], idx[i, L - 1] = a, k
            occupied[a, k] = True
    return idx, served, unresolved
