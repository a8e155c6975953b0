"""The rule of lcrec_finish_beam (include/lcrec.h) in numpy with dicts and sets: written from the rule, not from the kernels.
Tuples are compared as Python tuples of clamped codes; errors as floats with a NaN counted as +inf (so -0 and +0 tie, as they do
for a float comparison); every tie goes to the lowest item id."""
import numpy as np


def _err(x):
    x = float(x)
    return float("inf") if x != x else x


def clamp(idx, ks):
    """codes brought into their level as lcrec_collision_groups does it: v < 0 counts as 0, v >= K as K - 1"""
    return np.clip(np.asarray(idx, dtype=np.int64), 0, np.asarray(ks, dtype=np.int64) - 1)


def groups_of(idx, ks):
    """(members, offsets) of the shared tuples in lcrec_collision_groups' layout: groups in first-occurrence order, ids ascending"""
    seen = {}
    for i, row in enumerate(clamp(idx, ks).tolist()):
        seen.setdefault(tuple(row), []).append(i)
    groups = [g for g in seen.values() if len(g) > 1]
    members = np.array([i for g in groups for i in g], dtype=np.int64)
    offsets = np.cumsum([0] + [len(g) for g in groups]).astype(np.int64)
    return members, offsets


def finish_beam_ref(idx, ks, members, offsets, err_held, cand, cand_err):
    """idx int64 [n, L]; members [M], offsets [G + 1]; err_held float32 [M]; cand int64 [M, W, L]; cand_err float32 [M, W]
    -> (new idx, choice int32 [M], counters [movers, moved, unresolved, rounds with a proposal])"""
    idx = np.array(idx, dtype=np.int64)
    n, L = idx.shape
    M, W = cand_err.shape
    ks = [int(k) for k in ks]
    choice = np.full(M, -1, dtype=np.int32)
    # 1. keepers and movers
    movers = []
    for g in range(len(offsets) - 1):
        part = [j for j in range(int(offsets[g]), int(offsets[g + 1])) if 0 <= int(members[j]) < n]
        if len(part) < 2:
            continue
        keeper = min(part, key=lambda j: (_err(err_held[j]), int(members[j])))
        movers.extend(j for j in part if j != keeper)
    # 2. the occupied set
    occupied = {tuple(row) for row in clamp(idx, ks).tolist()}
    # 3. rounds
    live = lambda t: all(0 <= c < k for c, k in zip(t, ks))
    tuples = {j: [tuple(int(c) for c in cand[j, b]) for b in range(W)] for j in movers}
    ptr = {j: 0 for j in movers}
    rounds = 0
    while True:
        proposals = {}
        for j in list(ptr):
            p = ptr[j]
            while p < W and (not live(tuples[j][p]) or tuples[j][p] in occupied):
                p += 1
            if p >= W:
                del ptr[j]                                  # unresolved: it keeps its tuple
                choice[j] = -2
                continue
            ptr[j] = p
            proposals.setdefault(tuples[j][p], []).append(j)
        if not proposals:
            break
        rounds += 1
        for t, who in proposals.items():                    # (against the occupied set as it stood when the round began)
            winner = min(who, key=lambda j: (_err(cand_err[j, ptr[j]]), int(members[j])))
            for j in who:
                if j == winner:
                    idx[int(members[j])] = t
                    choice[j] = ptr[j]
                    del ptr[j]
                else:
                    ptr[j] += 1
        occupied.update(proposals)
    moved = int((choice >= 0).sum())
    return idx, choice, [len(movers), moved, len(movers) - moved, rounds]


def colliding_items(idx, ks):
    """n minus the number of distinct (clamped) tuples"""
    rows = clamp(idx, ks)
    return int(rows.shape[0] - np.unique(rows, axis=0).shape[0]) if rows.shape[0] else 0
