"""The three rules of the index trie (include/lcrec.h, lcrec_index_trie) in numpy: build is np.lexsort plus a prefix diff, find is a
dict walk, mask is set membership.  Everything is integer-exact; the mask works on the uint32 bits of the logits."""
import numpy as np

NEG_INF_BITS = np.uint32(0xFF800000)


def clamp(idx, ks):
    idx = np.asarray(idx, dtype=np.int64).reshape(-1, len(ks))
    return np.clip(idx, 0, np.asarray(ks, dtype=np.int64) - 1)


def build_ref(idx, ks):
    """dict(n, L, ks, order [n], counts [L+1], child: L arrays, code: L arrays, first) -- each array trimmed to the prefix the rule
    writes: child[d] has counts[d] + 1 entries, code[d-1] has counts[d], first has counts[L] + 1.  n == 0: child[d] = [0], first = [0]."""
    L = len(ks)
    c = clamp(idx, ks)
    n = c.shape[0]
    if n == 0:
        return dict(n=0, L=L, ks=list(ks), order=np.zeros(0, np.int64), counts=np.array([1] + [0] * L, dtype=np.int64),
                    child=[np.zeros(1, np.int64) for _ in range(L)], code=[np.zeros(0, np.int32) for _ in range(L)],
                    first=np.zeros(1, np.int64), sorted=c)
    order = np.lexsort([np.arange(n)] + [c[:, l] for l in range(L - 1, -1, -1)]).astype(np.int64)   # the last key is the primary one
    s = c[order]
    differs = s[1:] != s[:-1]                                              # [n-1, L]
    cpl = np.concatenate([[-1], np.where(differs.any(1), differs.argmax(1), L)])
    counts = np.array([(cpl < d).sum() for d in range(L + 1)], dtype=np.int64)
    number = [np.cumsum(cpl < d) - 1 for d in range(L + 1)]                # node of depth d that sorted position i lies under
    heads = [np.flatnonzero(cpl < d) for d in range(L + 1)]
    child = [np.concatenate([number[d + 1][heads[d]], [counts[d + 1]]]).astype(np.int64) for d in range(L)]
    code = [s[heads[d], d - 1].astype(np.int32) for d in range(1, L + 1)]
    first = np.concatenate([heads[L], [n]]).astype(np.int64)
    return dict(n=n, L=L, ks=list(ks), order=order, counts=counts, child=child, code=code, first=first, sorted=s)


def brute_force(idx, ks):
    """The same numbering from a dict of tuples: per depth the sorted distinct clamped prefixes.  -> (nodes: list of {prefix: number},
    holders: {tuple: ascending item ids})"""
    c = clamp(idx, ks)
    L = len(ks)
    nodes = [{p: j for j, p in enumerate(sorted({tuple(int(v) for v in row[:d]) for row in c}))} for d in range(L + 1)]
    if not len(c):
        nodes[0] = {(): 0}
    holders = {}
    for i, row in enumerate(c):
        holders.setdefault(tuple(int(v) for v in row), []).append(i)
    return nodes, holders


def walk_table(trie):
    """{(depth, node, code): child node} of a build_ref result"""
    table = {}
    for d in range(trie["L"]):
        kids = trie["child"][d]
        for j in range(int(trie["counts"][d]) if trie["n"] else 0):
            for k in range(int(kids[j]), int(kids[j + 1])):
                table[(d, j, int(trie["code"][d][k]))] = k
    return table


def find_ref(trie, prefixes, depth, table=None):
    """(node int64 [B], depth reached int32 [B]) of the longest-prefix descent; query codes are not clamped"""
    table = walk_table(trie) if table is None else table
    prefixes = np.asarray(prefixes, dtype=np.int64).reshape(-1, max(depth, 0)) if depth else np.zeros((len(prefixes), 0), np.int64)
    nodes, depths = np.zeros(len(prefixes), np.int64), np.zeros(len(prefixes), np.int32)
    for b, row in enumerate(prefixes):
        node, d = 0, 0
        while d < depth:
            c = int(row[d])
            if not 0 <= c < trie["ks"][d] or (d, node, c) not in table:
                break
            node, d = table[(d, node, c)], d + 1
        nodes[b], depths[b] = node, d
    return nodes, depths


def exact_only(nodes, depths, depth):
    """node_out of a call without depth_out"""
    return np.where(depths == depth, nodes, -1).astype(np.int64)


def allowed_ref(trie, node, depth, token_ids, eos):
    """the allowed token set of one row (token ids outside the vocabulary included: the mask never touches them)"""
    live = depth < trie["L"] and 0 <= node < trie["counts"][depth]
    if not live:
        return {int(eos)} if eos >= 0 else set()
    if trie["n"] == 0:
        return set()
    kids = trie["child"][depth]
    codes = trie["code"][depth][int(kids[node]):int(kids[node + 1])]
    return {int(c) if token_ids is None else int(token_ids[c]) for c in codes}


def mask_ref(trie, node, depth, token_ids, eos, bits, V):
    """`bits` uint32 [B, ld] (the logits' bits) masked by the rule: a copy; columns [V, ld) and allowed columns keep their bits"""
    out = np.array(bits, dtype=np.uint32, copy=True)
    for b in range(out.shape[0]):
        keep = np.zeros(V, dtype=bool)
        ok = [t for t in allowed_ref(trie, int(node[b]), depth, token_ids, eos) if 0 <= t < V]
        keep[ok] = True
        out[b, :V][~keep] = NEG_INF_BITS
    return out


def span_ref(trie, node, depth):
    """the half-open range of sorted positions under node `node` of depth `depth`"""
    a, b = int(node), int(node) + 1
    for d in range(depth, trie["L"]):
        a, b = int(trie["child"][d][a]), int(trie["child"][d][b])
    return int(trie["first"][a]), int(trie["first"][b])


def stats_ref(trie):
    L = trie["L"]
    leaf = np.diff(trie["first"]) if trie["n"] else np.zeros(0, np.int64)
    kids = [np.diff(trie["child"][d]) if trie["n"] else np.zeros(0, np.int64) for d in range(L)]
    return {"items": int(trie["n"]), "nodes": [int(v) for v in trie["counts"]], "largest_leaf": int(leaf.max()) if leaf.size else 0,
            "mean_children": [float(k.mean()) if k.size else 0.0 for k in kids],
            "max_children": [int(k.max()) if k.size else 0 for k in kids]}
