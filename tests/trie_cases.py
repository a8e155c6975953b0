"""The case table of the index trie: the build rows, the find rows on each of those tries and the mask rows.  Shared by
tests/test_trie_host.py (the numpy rule against a brute-force dict of tuples) and tests/test_gpu_trie.py (the kernels against the
rule).  Every input is seeded; the references are computed once and shared read-only."""
import functools

import numpy as np

import finish_cases as fc
from trie_ref import build_ref, walk_table

MASK_CHUNK = 4096                     # columns per workgroup of the mask kernel (include/lcrec.h states it)
FIND_BATCHES = (0, 1, 65, 4097)
F6_COUNTS = [1, 48, 521, 2931]


def _pooled(rs, n, ks, pool=12):
    """tuples that share prefixes of every length: each item copies one of `pool` base tuples up to a random level and draws the rest;
    the top code of a level is drawn often, so that the highest bits of wide keys are set"""
    L = len(ks)
    draw = lambda rows: np.stack([np.where(rs.rand(rows) < 0.25, k - 1, rs.randint(0, k, rows)) for k in ks], 1).astype(np.int64)
    base, out = draw(pool), draw(n)
    keep = rs.randint(0, L + 1, n)                                         # levels copied from the base tuple (L: a shared tuple)
    src = base[rs.randint(0, pool, n)]
    cols = np.arange(L)[None, :]
    return np.where(cols < keep[:, None], src, out)


def _uniform(rs, n, ks):
    return np.stack([rs.randint(0, k, n) for k in ks], 1).astype(np.int64)


def _distinct(rs, n, ks):
    all_tuples = np.stack(np.meshgrid(*[np.arange(k) for k in ks], indexing="ij"), -1).reshape(-1, len(ks))
    return all_tuples[rs.permutation(len(all_tuples))[:n]].astype(np.int64)


def _out_of_range(rs, n, ks):
    return np.stack([rs.randint(-3, k + 3, n) for k in ks], 1).astype(np.int64)


# name -> (n, ks, maker, idx_stride or 0)
BUILD = {
    "n0": (0, [4, 4], _uniform, 0),
    "n1": (1, [5, 3, 2], _uniform, 0),
    "L1K1": (7, [1], _uniform, 0),
    "one_tuple": (50, [8, 8, 8], lambda rs, n, ks: np.tile(np.array([[3, 7, 0]], dtype=np.int64), (n, 1)), 0),
    "distinct": (60, [4, 4, 4], _distinct, 0),
    "k48": (500, [48, 48, 48], _pooled, 0),
    "clamped": (200, [6, 5, 7], _out_of_range, 0),
    "bits64": (300, [256] * 8, _pooled, 0),
    "bits65": (300, [256] * 8 + [2], _pooled, 0),
    "bits128": (300, [256] * 16, _pooled, 0),
    "n63": (63, [6, 6, 6], _uniform, 0),
    "n64": (64, [6, 6, 6], _uniform, 0),
    "n65": (65, [6, 6, 6], _uniform, 0),
    "n1025": (1025, [16, 16, 16], _uniform, 0),
    "n70001": (70001, [48, 48, 48], _uniform, 0),
    "stride": (100, [5, 5, 5], _uniform, 6),
    "f6": (3000, [48, 48, 48], None, 0),
}
SMALL = [name for name in BUILD if name != "n70001"]                       # the rows a python dict walk is quick on


@functools.lru_cache(maxsize=None)
def build_case(name):
    """(idx int64 [n, L] read-only, ks, idx_stride, reference trie) of a build row"""
    n, ks, maker, stride = BUILD[name]
    if name == "f6":
        idx = np.array(fc.f6_case()[0], dtype=np.int64)
    else:
        idx = maker(np.random.RandomState(sorted(BUILD).index(name) + 100), n, ks).reshape(n, len(ks))
    idx.setflags(write=False)
    return idx, list(ks), stride, build_ref(idx, ks)


def wide(idx, stride):
    """idx laid out at a row stride > L: the matrix whose first L columns it is (the other columns hold codes no rule may read)"""
    out = np.full((len(idx), stride), 1 << 40, dtype=np.int64)
    out[:, :idx.shape[1]] = idx
    return out


@functools.lru_cache(maxsize=None)
def table_of(name):
    return walk_table(build_case(name)[3])


@functools.lru_cache(maxsize=None)
def find_queries(name, depth, B):
    """int64 [B, depth] queries on a build row's trie, a mixture: held tuples' prefixes (every held tuple when B allows), absent tuples
    that diverge at each level, and codes outside [0, K) -- among them the raw out-of-range codes of the row's own items, which the
    build clamps and the query must not match."""
    idx, ks, _, trie = build_case(name)
    rs = np.random.RandomState(7 * depth + B + 1)
    if depth == 0:
        return np.zeros((B, 0), dtype=np.int64)
    q = np.stack([rs.randint(0, k, B) for k in ks[:depth]], 1).astype(np.int64)            # mostly absent, diverging anywhere
    if len(idx):
        held = idx[np.resize(np.arange(len(idx)), B)][:, :depth].copy()                    # raw codes, out-of-range ones included
        kind = np.arange(B) % 4
        q[kind == 0] = held[kind == 0]
        q[kind == 1] = np.clip(held[kind == 1], 0, np.array(ks[:depth]) - 1)               # the clamped tuple itself: found
        lvl = rs.randint(0, depth, B)                                                      # a held prefix that diverges at one level
        div = np.clip(held, 0, np.array(ks[:depth]) - 1)
        div[np.arange(B), lvl] = (div[np.arange(B), lvl] + 1 + rs.randint(0, 3, B)) % np.array(ks[:depth])[lvl]
        q[kind == 2] = div[kind == 2]
    odd = np.flatnonzero(np.arange(B) % 16 == 3)                                           # plainly out of range, either side
    if odd.size:
        lvl = rs.randint(0, depth, odd.size)
        q[odd, lvl] = np.where(rs.rand(odd.size) < 0.5, -1 - rs.randint(0, 3, odd.size), np.array(ks[:depth])[lvl] + rs.randint(0, 3, odd.size))
    q.setflags(write=False)
    return q


# ---- the mask rows: (name, build row, depth, V, ld - V, row offset in floats, B, token map, eos) ---------------------------------
# token map: None = identity; "dup" = several codes on one token and ids outside [0, V) (negative, V, far beyond)
def _mask_rows():
    rows = []
    for V in (1, 3, 4, 5, 4097):
        rows.append((f"V{V}", "distinct", 1, V, 0, 0, 6, None, V - 1 if V > 1 else -1))   # (V = 1: column 0 is a child's; dead rows lose it)
    three = 3 * MASK_CHUNK + 1
    rows.append(("three_chunks_ld_V", "k48", 1, three, 0, 0, 5, "dup", MASK_CHUNK))            # eos on a chunk edge
    for off in (1, 2, 3):
        rows.append((f"odd_ld_offset{off}", "k48", 2, three, 3, off, 7, "dup", MASK_CHUNK - 1))   # rows at every alignment mod 16 B
    rows.append(("odd_ld_small", "k48", 0, 301, 1, 0, 9, None, 0))                              # K children of the root; eos at column 0
    rows.append(("one_child", "one_tuple", 1, 70, 5, 1, 4, None, -1))                           # nodes with one child, no eos
    rows.append(("k_children", "distinct", 2, 64, 1, 0, 19, None, 63))                          # every node has all K children
    rows.append(("leaf_depth", "k48", 3, 200, 3, 2, 6, "dup", 199))                             # depth == L: eos alone
    rows.append(("leaf_depth_no_eos", "k48", 3, 200, 0, 0, 3, None, -1))
    rows.append(("identity_beyond_V", "k48", 1, 20, 1, 0, 8, None, 7))                          # child codes >= V are ids outside [0, V)
    rows.append(("empty_trie", "n0", 0, 33, 0, 0, 3, None, 5))
    rows.append(("B0", "k48", 1, 100, 0, 0, 0, None, 3))
    rows.append(("clamped_items", "clamped", 2, 40, 3, 3, 11, "dup", 39))
    return rows


MASK = _mask_rows()


@functools.lru_cache(maxsize=None)
def mask_case(name):
    """(trie row, depth, V, ld, offset, B, token_ids int32 or None, eos, node int64 [B], bits uint32 [offset + B * ld]) of a mask row.
    The nodes cycle through live nodes and, on rows 1 and 2 (B allowing), the two dead values -1 and counts[depth].  The logits'
    bits are a pattern in which every word is a NaN, so "allowed bits stay" is a bit-for-bit statement."""
    row = next(r for r in MASK if r[0] == name)
    _, build, depth, V, pad, off, B, tokens, eos = row
    _, ks, _, trie = build_case(build)
    rs = np.random.RandomState(len(name) + V)
    live = int(trie["counts"][depth])
    node = rs.randint(0, max(live, 1), B).astype(np.int64)
    if B > 1:
        node[1] = -1
    if B > 2:
        node[2] = live
    if B > 3:
        node[3] = live - 1                                                  # the last node: its children end at the sentinel
    token_ids = None
    if tokens == "dup" and depth < len(ks):
        K = ks[depth]
        token_ids = rs.randint(0, V, K).astype(np.int32)
        token_ids[1::5] = token_ids[0::5][:len(token_ids[1::5])]            # duplicates
        token_ids[2::7] = np.resize(np.array([-1, V, V + 5, 1 << 30, -(1 << 30)], dtype=np.int32), len(token_ids[2::7]))
        token_ids[K - 1] = V - 1
    ld = V + pad
    bits = (np.uint32(0x7FC00000) | (rs.randint(1, 1 << 22, off + B * ld).astype(np.uint32))).astype(np.uint32)
    for a in (node, bits) + (() if token_ids is None else (token_ids,)):
        a.setflags(write=False)
    return build, depth, V, ld, off, B, token_ids, eos, node, bits
