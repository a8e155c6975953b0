"""The case table of collision grouping -- csrc/collide.hip behind lcrec_collision_groups -- shared by tests/test_collide_host.py
(CPU: every row has the properties it is listed for, asked of the row's own data and of the library's plan; the reference against
the restated helpers) and tests/test_gpu_collide_forms.py (GPU: every row against tests/collide_ref.py, integer-exact).

A row is (name, n, Ks, how its rows are generated -- a generator of this file with a fixed seed --, covers, plan).  `covers` names
properties; each property is a predicate (PROPERTIES) over the row's data, its reference result and the plan the library reports, so
a row cannot claim a path it does not reach.  `plan` holds the fields of lcrec_collision_plan the row claims.  REQUIRED lists the
properties that some row must keep claiming.

Sort regimes.  rocPRIM's radix_sort_pairs (rocprim/device/device_radix_sort.hpp, radix_sort_impl) takes one of three routes by size:
  - one block, for size <= block_size * items_per_thread of its block-sort config.  For (uint64 key, int64 value) that is
    kernel_config<min(256, 128 * 2), min(4, 4)> (radix_sort_block_sort_config_base in device/detail/device_config_helper.hpp with
    item_scale 8): SINGLE_BLOCK = 1024 items;
  - a merge sort up to radix_sort_config<>::merge_sort_limit: MERGE_LIMIT = 1024 * 1024 items;
  - onesweep above.
That a row runs in a regime is read from that code, not observed: the predicates below compare n with these two numbers."""
import functools
from collections import namedtuple

import numpy as np

from collide_ref import clamp, collide_ref

MAX_LEVELS = 16                    # LCREC_MAX_LEVELS
SINGLE_BLOCK = 1024
MERGE_LIMIT = 1024 * 1024
BIG = MERGE_LIMIT + 1
I64_MIN = -2 ** 63

Case = namedtuple("Case", "name n ks gen seed covers plan")


def bits_of(ks):
    """ceil(log2 K) per level: the key layout of include/lcrec.h, restated for the generators and predicates (the reference in
    collide_ref.py packs nothing)."""
    return [int(k - 1).bit_length() for k in ks]


def low_bits_of(ks):
    """The key bit at which each level starts (level 0 lies highest)."""
    b = bits_of(ks)
    return [sum(b[l + 1:]) for l in range(len(ks))]


def straddler(ks):
    """(level, bits of it below bit 64) of the level that has bits in both words, or None."""
    for l, (b, lo) in enumerate(zip(bits_of(ks), low_bits_of(ks))):
        if lo < 64 < lo + b:
            return l, 64 - lo
    return None


# ---------------------------------------------------------------- generators: (n, ks, RandomState) -> int64 [n, L]

def gen_uniform(n, ks, rs, span=None):
    """Independent codes in [0, min(K, span))."""
    return np.stack([rs.randint(0, min(k, span or k), size=n) for k in ks], axis=1).astype(np.int64)


def gen_edge_codes(n, ks, rs):
    """Codes from {0, 1, K-2, K-1} of every level: few tuples, the top code of each level among them."""
    cols = []
    for k in ks:
        codes = np.array(sorted({0, min(1, k - 1), max(k - 2, 0), k - 1}))
        cols.append(codes[rs.randint(0, len(codes), size=n)])
    return np.stack(cols, axis=1).astype(np.int64)


def gen_pool(n, ks, rs, of=gen_uniform):
    """n draws from a pool of n // 8 (at least 8) tuples made by `of`: every tuple is held by about eight items."""
    pool = of(max(8, n // 8), ks, rs)
    return pool[rs.randint(0, len(pool), size=n)]


def gen_variants(n, ks, rs):
    """A few base tuples (the first two with the top code and with 2^(bits-1) on level 0, so the key's highest bit is set); of each,
    variants that differ in exactly one level -- its top bit flipped, its lowest bit flipped, some of its lower bits, some of its
    upper bits, both; for the level that straddles bit 64 `lower` means the part in the low word -- 1 to 4 copies of every tuple,
    shuffled, cut or padded (by further copies) to n."""
    bits, strad = bits_of(ks), straddler(ks)
    kinds = sum(0 if b == 0 else 2 if b == 1 else 5 for b in bits)
    n_bases = max(8, int(n / (2.5 * (1 + kinds))) + 1)
    bases = np.stack([rs.randint(0, k, size=n_bases) for k in ks], axis=1).astype(np.int64)
    bases[0, 0], bases[1, 0] = ks[0] - 1, (1 << bits[0]) >> 1
    tuples = [bases]
    for l, (k, b) in enumerate(zip(ks, bits)):
        if b == 0:
            continue
        split = strad[1] if strad and strad[0] == l else max(1, b // 2)
        masks = [np.full(n_bases, 1 << (b - 1)), np.full(n_bases, 1)]
        if b >= 2:
            low = rs.randint(1, 1 << split, size=n_bases)
            high = rs.randint(1, 1 << (b - split), size=n_bases) << split
            masks += [low, high, low | high]
        for m in masks:
            t = bases.copy()
            c = t[:, l] ^ m
            t[:, l] = np.where(c < k, c, (t[:, l] + 1) % k)
            tuples.append(t)
    tuples = np.concatenate(tuples)
    rows = np.repeat(tuples, rs.randint(1, 5, size=len(tuples)), axis=0)
    rows = rows[rs.permutation(len(rows))]
    if len(rows) < n:
        rows = np.concatenate([rows, rows[rs.randint(0, len(rows), size=n - len(rows))]])
    return np.ascontiguousarray(rows[:n])


def _digits(values, ks):
    """The tuple of every mixed-radix value, level 0 the most significant digit."""
    out, v = [], np.asarray(values, dtype=np.int64)
    for k in ks[::-1]:
        out.append(v % k)
        v = v // k
    assert (v == 0).all()
    return np.stack(out[::-1], axis=1).astype(np.int64)


def gen_reversed(n, ks, rs):
    """n // 3 groups whose tuples descend as their first occurrences ascend: items 0 .. G-1 open the groups, largest tuple first;
    every group's other members follow in a shuffled order; what is left are single tuples below all of them."""
    G = n // 3
    assert G >= 3
    space = int(np.prod(ks))
    vals = np.sort(rs.choice(np.arange(space // 2, space), size=G, replace=False))[::-1]
    rest = np.concatenate([vals, vals[rs.randint(0, G, size=n - 2 * G - (n - 3 * G))]])
    singles = rs.choice(np.arange(0, space // 2), size=n - 3 * G, replace=False)
    tail = np.concatenate([rest, singles])
    return _digits(np.concatenate([vals, tail[rs.permutation(len(tail))]]), ks)


def gen_distinct(n, ks, rs):
    return _digits(rs.choice(int(np.prod(ks)), size=n, replace=False), ks)


def gen_first_last(n, ks, rs):
    """All tuples distinct, except that item n-1 repeats item 0 and two more pairs lie inside."""
    rows = gen_distinct(n, ks, rs)
    rows[n - 1] = rows[0]
    rows[n // 2] = rows[3]
    rows[n // 2 + 7] = rows[n // 2 - 9]
    return rows


def gen_last_pair(n, ks, rs):
    """Items n-2 and n-1 share the smallest tuple; items 0 and 5 share the largest; every other tuple is single."""
    space = int(np.prod(ks))
    vals = 1 + rs.choice(space - 2, size=n, replace=False)
    vals[[0, 5]] = space - 1
    vals[[n - 2, n - 1]] = 0
    return _digits(vals, ks)


def gen_identical(n, ks, rs):
    return np.tile(_digits([rs.randint(1, int(np.prod(ks)))], ks), (n, 1))


def gen_pairs(n, ks, rs):
    """Every item shares its tuple with exactly one other (n odd: one tuple has three), positions shuffled."""
    tuples = np.unique(gen_uniform(4 * n, ks, rs), axis=0)
    tuples = tuples[rs.permutation(len(tuples))[:n // 2]]
    assert len(tuples) == n // 2
    return np.concatenate([tuples, tuples, tuples[:n % 2]])[rs.permutation(n)]


def gen_clamped(n, ks, rs):
    """gen_pool of gen_edge_codes, then about half of the codes 0 become -1 or INT64_MIN and about half of the codes K-1 become K or 2^40: every
    such row must collide with the rows that kept the in-range code."""
    rows = gen_pool(n, ks, rs, of=gen_edge_codes)
    karr = np.asarray(ks, dtype=np.int64)[None, :]
    pick = rs.randint(0, 4, size=rows.shape)
    below = np.where(pick == 0, -1, I64_MIN)
    above = np.where(pick == 1, karr, 2 ** 40)
    out = np.where((rows == 0) & (pick % 2 == 0), below, rows)
    out = np.where((rows == karr - 1) & (karr > 1) & (pick % 2 == 1), above, out)
    return out.astype(np.int64)


# ---------------------------------------------------------------- the table

def _plan(n, ks):
    """The plan fields a row claims, from its shape by the rule of include/lcrec.h."""
    total = sum(bits_of(ks))
    return dict(total_bits=total, lo_bits=min(64, max(total, 1)), hi_bits=max(0, total - 64), id_bits=max(1, int(n - 1).bit_length()),
                stride=-(-n * 8 // 256) * 256)


def _case(name, n, ks, gen, seed, covers, **claims):
    plan = _plan(n, ks)
    for k, v in claims.items():                 # a row may spell a claim out: it must agree with the rule
        assert plan[k] == v, (name, k, plan[k], v)
    return Case(name, n, tuple(ks), gen, seed, tuple(covers), tuple(sorted(plan.items())))


K16, WIDE = [16, 16, 16], [1024] * 8
ROWS = [
    # key width
    _case("0 bits, one item", 1, [1, 1, 1], gen_uniform, 1, ["zero_bits", "n=1"], lo_bits=1, hi_bits=0, id_bits=1),
    _case("0 bits, five items", 5, [1, 1, 1], gen_uniform, 2, ["zero_bits", "all_identical"], lo_bits=1, hi_bits=0),
    _case("narrow", 700, K16, functools.partial(gen_uniform, span=5), 3, ["heavy_duplication"], lo_bits=12),
    _case("non-powers of two", 300, [3, 7, 100], gen_edge_codes, 4, ["nonpow2_top_codes"], lo_bits=12),
    _case("64 bits", 600, [65536] * 4, gen_variants, 5, ["bit63", "top_bit_pairs"], lo_bits=64, hi_bits=0),
    _case("65 bits", 600, [65536] * 4 + [2], gen_variants, 6, ["lo_equal_hi_differs", "top_bit_pairs", "straddle"], lo_bits=64, hi_bits=1),
    _case("80 bits", 700, WIDE, gen_variants, 7,
          ["lo_equal_hi_differs", "hi_equal_lo_differs", "top_bit_pairs", "straddle", "straddle_upper_only", "straddle_lower_only",
           "straddle_both"], lo_bits=64, hi_bits=16),
    _case("128 bits", 700, [65536] * 8, gen_variants, 8, ["bit127", "lo_equal_hi_differs", "hi_equal_lo_differs", "top_bit_pairs"],
          lo_bits=64, hi_bits=64),
    _case("16 levels, 128 bits", 900, [200] * 16, gen_variants, 9, ["max_levels", "bit127", "lo_equal_hi_differs", "hi_equal_lo_differs"],
          hi_bits=64),
    _case("16 levels, mixed small K", 400, [5, 3, 2, 1, 16, 7, 100, 2, 9, 4, 1, 33, 8, 3, 2, 6], gen_pool, 10,
          ["max_levels", "heavy_duplication"], lo_bits=42, hi_bits=0),
    # order
    _case("first occurrences against key order", 300, K16, gen_reversed, 11, ["order_reversed"]),
    _case("a group {0, n-1}", 300, K16, gen_first_last, 12, ["group_first_and_last"]),
    _case("the last two items pair up, an early group has the largest key", 300, K16, gen_last_pair, 13, ["last_pair_after_large_key"]),
    _case("all identical", 300, K16, gen_identical, 14, ["all_identical"]),
    _case("all distinct", 300, K16, gen_distinct, 15, ["all_distinct"]),
    _case("every item in a pair, n even", 258, K16, gen_pairs, 16, ["max_groups_even"]),
    _case("every item in a pair or the one triple, n odd", 259, K16, gen_pairs, 17, ["max_groups_odd"]),
    _case("every item in a pair, 80 bits", 258, WIDE, gen_pairs, 18, ["max_groups_even"], hi_bits=16),
    # sizes: block edges, id_bits edges, rocPRIM's single-block threshold, onesweep
    _case("n = 2, one pair", 2, K16, gen_identical, 19, ["n=2", "max_groups_even"], id_bits=1),
    _case("n = 255", 255, K16, functools.partial(gen_uniform, span=6), 20, ["n=255"], id_bits=8),
    _case("n = 256", 256, [3, 7, 100], functools.partial(gen_uniform, span=7), 21, ["n=256"], id_bits=8),
    _case("n = 257", 257, K16, functools.partial(gen_uniform, span=6), 22, ["n=257"], id_bits=9),
    _case("n = 512", 512, K16, gen_uniform, 23, ["id_bits_9_late_group"], id_bits=9),
    # (n = 2^k + 1: item 2^k alone needs the top bit of id_bits, and the last item opens no group -- a last sort one bit short is
    # invisible at 257 and 513 by construction; 255, 256, 512 and 1024 are the rows that see it)
    _case("n = 513", 513, K16, gen_uniform, 24, ["id_bits_10_late_group"], id_bits=10),
    _case("n = 1024", SINGLE_BLOCK, [256] * 2, functools.partial(gen_uniform, span=40), 25, ["sort_single_block"], id_bits=10),
    _case("n = 1025", SINGLE_BLOCK + 1, [256] * 2, functools.partial(gen_uniform, span=40), 26, ["sort_merge"], id_bits=11),
    _case("n = 1025, 80 bits", SINGLE_BLOCK + 1, WIDE, gen_variants, 27, ["sort_merge", "lo_equal_hi_differs", "hi_equal_lo_differs"], hi_bits=16),
    _case("n = 2^20 + 1, 24 bits", BIG, [256] * 3, gen_uniform, 28, ["sort_onesweep"], lo_bits=24, id_bits=21),
    _case("n = 2^20 + 1, 80 bits", BIG, WIDE, gen_variants, 29, ["sort_onesweep", "lo_equal_hi_differs", "hi_equal_lo_differs"],
          hi_bits=16, id_bits=21),
    # the clamp
    _case("clamp, narrow", 300, [16, 100, 7], gen_clamped, 30, ["clamp"], lo_bits=14),
    _case("clamp, 80 bits", 300, WIDE, gen_clamped, 31, ["clamp"], hi_bits=16),
]
REFUSED_BITS = [([65536] * 8 + [2], 129), ([1024] * 16, 160)]          # more than 128 bits: LCREC_EUNSUPPORTED

REQUIRED = ["lo_equal_hi_differs", "hi_equal_lo_differs", "straddle", "straddle_upper_only", "straddle_lower_only", "straddle_both",
            "bit63", "bit127", "zero_bits", "max_levels", "max_groups_even", "max_groups_odd", "id_bits_9_late_group",
            "id_bits_10_late_group", "sort_single_block", "sort_merge", "sort_onesweep", "clamp", "top_bit_pairs", "nonpow2_top_codes",
            "order_reversed", "group_first_and_last", "last_pair_after_large_key", "all_identical", "all_distinct", "heavy_duplication",
            "n=1", "n=2", "n=255", "n=256", "n=257"]
SMALL = 5000                       # rows up to this size are also run through the dict-based helpers


def case_id(c):
    return c.name.replace(" ", "_")


@functools.lru_cache(maxsize=None)
def data(c):
    """The row's int64 [n, L] matrix (shared: read only)."""
    rows = np.ascontiguousarray(c.gen(c.n, list(c.ks), np.random.RandomState(1000 + c.seed)), dtype=np.int64)
    assert rows.shape == (c.n, len(c.ks))
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def expected(c):
    """collide_ref of the row, computed once (shared: read only)."""
    ref = collide_ref(data(c), c.ks)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


# ---------------------------------------------------------------- properties: name -> predicate(row, data, reference, library plan)

def _distinct(c):
    """The row's distinct clamped tuples."""
    return clamp(data(c), c.ks)[expected(c)["firsts"]]


def _words(c):
    """(low word, high word) uint64 of every distinct tuple, by the key layout of include/lcrec.h."""
    t = _distinct(c).astype(np.uint64)
    lo, hi = np.zeros(len(t), np.uint64), np.zeros(len(t), np.uint64)
    for l, b in enumerate(bits_of(c.ks)):
        if b:
            hi = (hi << np.uint64(b)) | (lo >> np.uint64(64 - b))
            lo = (lo << np.uint64(b)) | t[:, l]
    return lo, hi


def _shared(a, b):
    """How many values of a occur with two or more values of b; the (a, b) pairs are distinct, being the words of distinct tuples."""
    assert len(np.unique(np.stack([a, b]), axis=1)[0]) == len(a)
    _, inv = np.unique(a, return_inverse=True)
    return int((np.bincount(inv.ravel()) >= 2).sum())


def _level_pairs(c, level):
    """XOR of the codes at `level` of pairs of distinct tuples that agree everywhere else."""
    t = _distinct(c)
    cols = [t[:, l] for l in range(t.shape[1]) if l != level]
    order = np.lexsort([t[:, level]] + cols[::-1])
    s = t[order]
    others = np.delete(s, level, axis=1)
    start = np.ones(len(s), dtype=bool)
    start[1:] = (others[1:] != others[:-1]).any(axis=1)
    first = np.maximum.accumulate(np.where(start, np.arange(len(s)), 0))
    x = np.concatenate([(s[:, level] ^ s[first, level])[~start], (s[1:, level] ^ s[:-1, level])[~start[1:]]])
    return x[x != 0]


def _straddle_parts(c):
    level, low = straddler(c.ks)
    x = _level_pairs(c, level)
    return (x >> low) != 0, (x & ((1 << low) - 1)) != 0


def _top_bit_pairs(c):
    """Tuples that differ in the key's highest bit alone, each held by two or more items whose ids interleave with the other's: a
    sort that leaves that bit out no longer keeps either tuple's items together."""
    b0 = bits_of(c.ks)[0]
    rows = clamp(data(c), c.ks)
    flipped = rows.copy()
    flipped[:, 0] ^= 1 << (b0 - 1)
    both = np.concatenate([rows, flipped])
    _, inv = np.unique(both, axis=0, return_inverse=True)
    inv = inv.ravel()
    mine, other = inv[:len(rows)], inv[len(rows):]
    present = np.zeros(inv.max() + 1, dtype=bool)
    present[mine] = True
    found = 0
    for t in np.unique(mine[present[other]]):
        a = np.flatnonzero(mine == t)
        b = np.flatnonzero(other == t)
        if len(a) >= 2 and len(b) >= 1 and a[0] < b[0] < a[-1]:
            found += 1
    return found >= 2


def _groups(c):
    e = expected(c)
    return np.split(e["members"], e["offsets"][1:-1]) if e["n_groups"] else []


def _group_tuples(c):
    e = expected(c)
    return clamp(data(c), c.ks)[e["members"][e["offsets"][:-1]]]


def _descending(t):
    """Every row of t lexicographically below the one before it."""
    d = t[1:] - t[:-1]
    nz = d != 0
    return bool(nz.any(axis=1).all() and (d[np.arange(len(d)), nz.argmax(axis=1)] < 0).all())


def _late_group(c):
    e = expected(c)
    return e["n_groups"] > 0 and int(e["members"][e["offsets"][-2]]) >= 256


def _last_pair(c):
    gs, t = _groups(c), _group_tuples(c)
    return len(gs) >= 2 and gs[-1].tolist() == [c.n - 2, c.n - 1] and gs[0][0] < 8 and tuple(t[0]) > tuple(t[-1])


def _clamp(c):
    raw, ks = data(c), np.asarray(c.ks, dtype=np.int64)
    kinds = [(raw == -1).any(), (raw == I64_MIN).any(), (raw == ks[None, :]).any(), (raw == 2 ** 40).any()]
    outside = ((raw < 0) | (raw >= ks[None, :])).any(axis=1)
    # some groups hold both a row with an out-of-range code and a row without: the clamp, and nothing else, joined them
    mixed = sum(1 for g in _groups(c) if outside[g].any() and not outside[g].all())
    return all(kinds) and mixed >= 4 and expected(c)["unique"] < len(np.unique(raw, axis=0))


PROPERTIES = {
    "zero_bits": lambda c, p: p["total_bits"] == 0 and p["lo_bits"] == 1 and p["hi_bits"] == 0,
    "heavy_duplication": lambda c, p: expected(c)["unique"] * 3 < c.n and expected(c)["max_count"] >= 4,
    "nonpow2_top_codes": lambda c, p: all(k & (k - 1) and (data(c)[:, l] == k - 1).any() for l, k in enumerate(c.ks)),
    "bit63": lambda c, p: p["total_bits"] == 64 and p["lo_bits"] == 64 and p["hi_bits"] == 0 and bool((_words(c)[0] >> np.uint64(63)).any())
    and bool((data(c)[:, 0] == c.ks[0] // 2).any()) and bool((data(c)[:, 0] > c.ks[0] // 2).any()),
    "bit127": lambda c, p: p["total_bits"] == 128 and p["hi_bits"] == 64 and bool((_words(c)[1] >> np.uint64(63)).any()),
    "max_levels": lambda c, p: len(c.ks) == MAX_LEVELS and p["total_bits"] <= 128,
    "lo_equal_hi_differs": lambda c, p: p["hi_bits"] > 0 and _shared(*_words(c)) >= 8,
    "hi_equal_lo_differs": lambda c, p: p["hi_bits"] > 0 and _shared(*_words(c)[::-1]) >= 8,
    "straddle": lambda c, p: p["hi_bits"] > 0 and straddler(c.ks) is not None and len(_level_pairs(c, straddler(c.ks)[0])) > 0,
    "straddle_upper_only": lambda c, p: straddler(c.ks) is not None and bool((_straddle_parts(c)[0] & ~_straddle_parts(c)[1]).any()),
    "straddle_lower_only": lambda c, p: straddler(c.ks) is not None and bool((~_straddle_parts(c)[0] & _straddle_parts(c)[1]).any()),
    "straddle_both": lambda c, p: straddler(c.ks) is not None and bool((_straddle_parts(c)[0] & _straddle_parts(c)[1]).any()),
    "top_bit_pairs": lambda c, p: p["total_bits"] >= 64 and _top_bit_pairs(c),
    "order_reversed": lambda c, p: expected(c)["n_groups"] >= 3 and _descending(_group_tuples(c)),
    "group_first_and_last": lambda c, p: any(g.tolist() == [0, c.n - 1] for g in _groups(c)) and expected(c)["n_groups"] >= 2,
    "last_pair_after_large_key": lambda c, p: _last_pair(c),
    "all_identical": lambda c, p: c.n >= 2 and expected(c)["n_groups"] == 1 and expected(c)["max_count"] == c.n and expected(c)["unique"] == 1,
    "all_distinct": lambda c, p: c.n >= 2 and expected(c)["n_groups"] == 0 and expected(c)["offsets"].tolist() == [0] and expected(c)["unique"] == c.n,
    "max_groups_even": lambda c, p: c.n % 2 == 0 and expected(c)["n_groups"] == c.n // 2 and len(expected(c)["members"]) == c.n,
    "max_groups_odd": lambda c, p: c.n % 2 == 1 and c.n >= 3 and expected(c)["n_groups"] == c.n // 2 and len(expected(c)["members"]) == c.n,
    "id_bits_9_late_group": lambda c, p: c.n == 512 and p["id_bits"] == 9 and _late_group(c),
    "id_bits_10_late_group": lambda c, p: c.n == 513 and p["id_bits"] == 10 and _late_group(c),
    "sort_single_block": lambda c, p: c.n == SINGLE_BLOCK,
    "sort_merge": lambda c, p: SINGLE_BLOCK < c.n <= MERGE_LIMIT and c.n == SINGLE_BLOCK + 1,
    "sort_onesweep": lambda c, p: c.n > MERGE_LIMIT,
    "clamp": lambda c, p: _clamp(c),
}
for _n in (1, 2, 255, 256, 257):
    PROPERTIES[f"n={_n}"] = (lambda v: lambda c, p: c.n == v)(_n)
