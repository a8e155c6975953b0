"""The rule of lcrec_extend_finish_beam (include/lcrec.h) in numpy with dicts and sets: written from the rule's text, not from the
kernels, and not by calling tests/beam_finish_ref.py.  Tuples are compared as Python tuples of clamped codes; errors as floats with
a NaN counted as +inf; every tie goes to the lowest item id.  Nothing is ever read from err_held, cand or cand_err at the position
of a frozen member: the function does not index them there."""
import numpy as np

from beam_finish_ref import clamp


def _err(x):
    x = float(x)
    return float("inf") if x != x else x


def extend_finish_beam_ref(idx, n_frozen, ks, members, offsets, err_held, cand, cand_err):
    """idx int64 [n, L]; items below n_frozen are frozen; members [M], offsets [G + 1]; err_held float32 [M]; cand int64 [M, W, L];
    cand_err float32 [M, W] -> (new idx, choice int32 [M], counters [movers, moved, unresolved, rounds with a proposal])"""
    idx = np.array(idx, dtype=np.int64)
    n, L = idx.shape
    M, W = cand_err.shape
    n_frozen = int(n_frozen)
    assert 0 <= n_frozen <= n
    ks = [int(k) for k in ks]
    choice = np.full(M, -1, dtype=np.int32)
    # 1. per group: the holders are the members whose id lies in [0, n)
    movers = []
    for g in range(len(offsets) - 1):
        holders = [j for j in range(int(offsets[g]), int(offsets[g + 1])) if 0 <= int(members[j]) < n]
        fresh = [j for j in holders if int(members[j]) >= n_frozen]
        if len(holders) < 2 or not fresh:
            continue                                        # fewer than two holders, or no new holder: no mover
        if len(fresh) < len(holders):
            movers.extend(fresh)                            # a frozen holder: every new holder moves
        else:
            keeper = min(fresh, key=lambda j: (_err(err_held[j]), int(members[j])))
            movers.extend(j for j in fresh if j != keeper)
    # 2. the occupied set: every tuple held by any of the n items, the frozen ones included
    occupied = {tuple(row) for row in clamp(idx, ks).tolist()}
    # 3. rounds: only movers propose
    live = lambda t: all(0 <= c < k for c, k in zip(t, ks))
    ptr = {j: 0 for j in movers}
    at = lambda j, p: tuple(int(c) for c in cand[j, p])
    rounds = 0
    while ptr:
        proposals = {}
        for j in sorted(ptr):
            p = ptr[j]
            while p < W and (not live(at(j, p)) or at(j, p) in occupied):
                p += 1
            if p >= W:
                del ptr[j]                                  # unresolved: it keeps its tuple
                choice[j] = -2
                continue
            ptr[j] = p
            proposals.setdefault(at(j, p), []).append(j)
        if not proposals:
            break
        rounds += 1
        for t, who in proposals.items():                    # (against the occupied set as it stood when the round began)
            winner = min(who, key=lambda j: (_err(cand_err[j, ptr[j]]), int(members[j])))
            idx[int(members[winner])] = t
            choice[winner] = ptr[winner]
            for j in who:
                if j == winner:
                    del ptr[j]
                else:
                    ptr[j] += 1
        occupied.update(proposals)
    moved = int((choice >= 0).sum())
    return idx, choice, [len(movers), moved, len(movers) - moved, rounds]
