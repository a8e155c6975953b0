"""What lcrec_collision_groups must report, stated in numpy over the tuples themselves: no key is packed here, so this cannot share
a packing mistake with csrc/collide.hip.  Rows are compared as rows (one stable lexicographic sort).

The rule (include/lcrec.h, lcrec_collision_groups):
  - a code outside [0, K[l]) is clamped into it first: v < 0 -> 0, v >= K[l] -> K[l] - 1;
  - `unique` is the number of distinct clamped tuples, `max_count` the largest number of items on one tuple;
  - a group is the set of items of a tuple that two or more items hold; groups come in the order of the first occurrence of their
    tuple in item order, item ids ascend inside a group (generate_indices.get_collision_item's order);
  - members = the groups' ids one group after the other, offsets[g] = where group g starts, offsets[n_groups] = len(members)."""
import numpy as np


def clamp(idx, ks):
    idx = np.asarray(idx, dtype=np.int64)
    ks = np.asarray(ks, dtype=np.int64)
    assert idx.ndim == 2 and idx.shape[1] == len(ks) >= 1 and (ks >= 1).all()
    return np.clip(idx, 0, ks - 1)


def collide_ref(idx, ks):
    """dict(unique, max_count, n_groups, members int64 [items in groups], offsets int64 [n_groups + 1], firsts int64 [unique]: the
    lowest id on each distinct tuple, ascending) of an int64 [n, L] matrix."""
    rows = clamp(idx, ks)
    n = len(rows)
    if n == 0:
        return dict(unique=0, max_count=0, n_groups=0, members=np.zeros(0, np.int64), offsets=np.zeros(1, np.int64),
                    firsts=np.zeros(0, np.int64))
    order = np.lexsort(rows.T[::-1])                      # stable; column 0 is the primary key: equal rows lie together, ids ascending
    srt = rows[order]
    head = np.ones(n, dtype=bool)
    head[1:] = (srt[1:] != srt[:-1]).any(axis=1)
    seg = np.cumsum(head) - 1                             # the tuple number of every sorted position
    counts = np.bincount(seg)
    first = order[head]                                   # the lowest id on each tuple
    first_of = np.empty(n, dtype=np.int64)                # per item: the lowest id on its tuple
    first_of[order] = first[seg]
    count_of = np.empty(n, dtype=np.int64)
    count_of[order] = counts[seg]
    ids = np.flatnonzero(count_of > 1)                    # ascending
    members = ids[np.argsort(first_of[ids], kind="stable")]
    starts = np.sort(first[counts > 1])                   # the first id of every group, in group order
    offsets = np.concatenate([[0], np.cumsum(count_of[starts])]).astype(np.int64)
    return dict(unique=int(len(counts)), max_count=int(counts.max()), n_groups=int(len(starts)), members=members.astype(np.int64),
                offsets=offsets, firsts=np.sort(first).astype(np.int64))


def groups_of(ref):
    """The groups as lists of ids (the form generate_indices.get_collision_item returns)."""
    m, o = ref["members"].tolist(), ref["offsets"].tolist()
    return [m[o[g]:o[g + 1]] for g in range(ref["n_groups"])]
