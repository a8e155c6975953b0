"""The frozen-aware nearest-free-code rule of lcrec_extend_nearest_free (include/lcrec.h) in numpy, on the oracle's distances:
written from the rule's text, not from the kernel.  d = oracle.distances (xx, cc, dot as fp32 fma chains; d = (xx + cc) - 2 dot);
a NaN counts as +inf wherever distances are compared; np.argmin takes the first minimum."""
import numpy as np

from oracle import cpu_oracle


def extend_ref(idx, n_frozen, resid_new, cb_last, buckets=None):
    """idx int [N, L]; items below n_frozen are frozen; resid_new [N - n_frozen, e] holds the rows of the new items only (no
    residual exists for a frozen item, and none is looked at); cb_last [K, e].
    buckets: None = the items sharing idx[:, :L-1]; or lists of item ids as a caller would pass them to the entry -- a member whose
    id is outside [0, N) or whose last code is outside [0, K) takes no part.
    -> (new idx int64 [N, L], mover ids in the order they were served, unresolved)."""
    idx = np.array(idx, dtype=np.int64)
    n, L = idx.shape
    K = cb_last.shape[0]
    if buckets is None:
        found = {}
        for i in range(n):                                                  # 1. buckets: frozen and new together
            found.setdefault(tuple(idx[i, :L - 1]), []).append(i)
        buckets = list(found.values())
    movers_all, unresolved = [], 0
    for listed in buckets:
        items = sorted(int(i) for i in listed if 0 <= i < n and 0 <= idx[i, L - 1] < K)
        holders = {}
        for i in items:
            holders.setdefault(int(idx[i, L - 1]), []).append(i)
        shared = {k: h for k, h in holders.items() if len(h) >= 2 and h[-1] >= n_frozen}   # ... at least one of them new
        if not shared:
            continue                                                        # untouched (always so without a new item)
        new = [i for i in items if i >= n_frozen]
        d = cpu_oracle.distances(np.ascontiguousarray(resid_new[[i - n_frozen for i in new]]), cb_last)
        d = np.where(np.isnan(d), np.float32(np.inf), d)
        row = {i: r for r, i in enumerate(new)}
        movers = []
        for k, h in shared.items():                                         # 2. a frozen holder: every new holder moves
            fresh = [i for i in h if i >= n_frozen]
            if len(fresh) < len(h):
                movers += fresh
            else:                                                           #    else the nearest keeps it, tie -> lowest id
                keeper = fresh[int(np.argmin([d[row[i], k] for i in fresh]))]
                movers += [i for i in fresh if i != keeper]
        occupied = np.zeros(K, dtype=bool)                                  # 3. every code held by any item of the bucket
        occupied[list(holders)] = True
        for i in sorted(movers):                                            # 4. movers in ascending id
            movers_all.append(i)
            if occupied.all():
                unresolved += 1
                continue
            free = np.flatnonzero(~occupied)
            k = int(free[np.argmin(d[row[i], free])])                       # first minimum in code order
            idx[i, L - 1] = k
            occupied[k] = True
    return idx, movers_all, unresolved
