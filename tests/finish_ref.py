"""The nearest-free-code rule of lcrec_finish_nearest_free (include/lcrec.h) in numpy, on the oracle's distances: written from the
rule, not from the kernel.  d = oracle.distances (xx, cc, dot as fp32 fma chains; d = (xx + cc) - 2 dot); a NaN counts as +inf
wherever distances are compared; np.argmin takes the first minimum."""
import numpy as np

from oracle import cpu_oracle


def finish_ref(idx, resid_last, cb_last, buckets=None):
    """idx int [N, L], resid_last [N, e], cb_last [K, e] -> (new idx int64 [N, L], mover ids in the order they were served,
    unresolved).  len(movers) - unresolved items moved.
    buckets: None = the items sharing idx[:, :L-1]; or lists of item ids as a caller would pass them to the entry -- a member whose
    id is outside [0, N) or whose last code is outside [0, K) takes no part."""
    idx = np.array(idx, dtype=np.int64)
    n, L = idx.shape
    K = cb_last.shape[0]
    if buckets is None:
        found = {}
        for i in range(n):                                                  # 1. buckets: items sharing idx[:, :L-1]
            found.setdefault(tuple(idx[i, :L - 1]), []).append(i)
        buckets = list(found.values())
    movers_all, unresolved = [], 0
    for listed in buckets:                                                  # (ids ascend inside a bucket)
        items = sorted(int(i) for i in listed if 0 <= i < n and 0 <= idx[i, L - 1] < K)
        holders = {}
        for i in items:
            holders.setdefault(int(idx[i, L - 1]), []).append(i)
        shared = {k: h for k, h in holders.items() if len(h) >= 2}
        if not shared:
            continue                                                        # untouched
        d = cpu_oracle.distances(resid_last[items], cb_last)
        d = np.where(np.isnan(d), np.float32(np.inf), d)
        row = {i: r for r, i in enumerate(items)}
        movers = []
        for k, h in shared.items():                                         # 2. keepers: smallest d(i, k), tie -> lowest id
            keeper = h[int(np.argmin([d[row[i], k] for i in h]))]
            movers += [i for i in h if i != keeper]
        occupied = np.zeros(K, dtype=bool)                                  # 3. every code held by any item of the bucket
        occupied[list(holders)] = True
        for i in sorted(movers):                                            # 4. movers in ascending id
            movers_all.append(i)
            if occupied.all():                                              #    no code free: this one and all later stay
                unresolved += 1
                continue
            free = np.flatnonzero(~occupied)
            k = int(free[np.argmin(d[row[i], free])])                       # first minimum in code order
            idx[i, L - 1] = k
            occupied[k] = True
    return idx, movers_all, unresolved


def colliding_items(idx):
    """Items that share their tuple with an earlier item: N - |distinct tuples|, the numerator of the collision rate."""
    idx = np.asarray(idx)
    return int(idx.shape[0] - np.unique(idx, axis=0).shape[0])
