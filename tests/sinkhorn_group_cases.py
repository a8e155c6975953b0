"""The case table of the grouped Sinkhorn solver (lcrec_sinkhorn_assign with group_offsets: sk_small_kernel<E, GLOBALQ, THREADS> of
csrc/vq_train.hip, launched per size class by sk_groups_plan), shared by tests/test_sinkhorn_groups_plan_host.py (CPU: every row's
launch plan is the expected one and reaches the paths it claims, its inputs are judgeable, the judge refuses wrong solves) and
tests/test_gpu_sinkhorn_groups.py (GPU: every row of every group against the reference: winner, runner-up, second / best).

A row is (K, e, sizes, eps, iters, context, stride, head, tail, seed): `sizes` the rows of each group in offset order (0: an empty
group), `head` / `tail` rows in front of the first and behind the last group that belong to no group and must keep their sentinel,
`context` whether the call is made with a context (ring upload, helper streams) or with NULL.  Each row carries the plan
lcrec_debug_sinkhorn_groups_plan must give for it (`expect`) and the paths it exists for (`covers`, names of PROPERTIES: predicates
over the row and its plan, so a row cannot claim a path its shape does not reach); REQUIRED lists the paths some row must claim.

Values.  With fewer rows than codes at eps = 0.003 the reference solve saturates: a column dominated by one row is divided by a
column sum that equals it bit for bit, the row holds several entries of exactly 1 / K, and the winner is the first of them.  Those
ties are structural -- they do not depend on the order of summation -- but a longdouble solve resolves deficits below 2^-53 that
fp64 rounds away and names other winners.  So winners and runner-ups are held to the reference's own precision, fp64, on EVERY row,
under a stability condition established under the reference alone (conditions()): three fp64 evaluations of the reference's loop
-- numpy, numpy with reversed sequential sums and every exp moved by -1 / 0 / +1 ulp, and oracle/torch_ref.sinkhorn -- agree on
every row's winner and runner-up.  A seed that misses the condition is replaced by the next, never the condition.  The second /
best ratios keep the rule of tests/sinkhorn_cases.py: SLACK x max(the fp64 reference's own distance from the longdouble solve on
that group, FLOOR); and a ratio that is exactly 1.0 in all three fp64 evaluations must be exactly 1.0."""
import functools
from collections import namedtuple

import numpy as np

import sinkhorn_cases as sk

SLACK, FLOOR = sk.SLACK, sk.FLOOR
# largest distance, over the groups of CASES, of oracle/torch_ref.sinkhorn in fp64 from the longdouble solve of the same group:
# 6.21e-14, on the row with K = 100; 1.6e-14 .. 5.8e-14 on the other rows at eps = 0.003, 7e-16 .. 1.5e-15 at eps = 0.05
# (recomputed and compared by tests/test_sinkhorn_groups_plan_host.py).  A group is judged by its OWN distance.
MEASURED = 6.3e-14
ARGUMENT, RING, SYNCHRONOUS = 1, 2, 3
SLAB, BATCH = 4, 5
LDS_LIMIT = 160 * 1024               # bytes of LDS a workgroup can have, static part included
LDS_STATIC = 64                      # of sk_small_kernel<E, false, 256>

Case = namedtuple("Case", "K e sizes eps iters context stride head tail seed expect covers")


def _case(K, e, sizes, covers, eps=0.003, iters=50, context=True, stride=1, head=0, tail=0, seed=0, **expect):
    return Case(K, e, tuple(sizes), eps, iters, context, stride, head, tail, seed, expect, tuple(covers))


def case_id(c):
    return (f"K{c.K}-e{c.e}-{len(c.sizes)}groups-{sum(c.sizes)}rows-eps{c.eps}-it{c.iters}-{'ctx' if c.context else 'noctx'}"
            + (f"-stride{c.stride}" if c.stride != 1 else "") + (f"-seed{c.seed}" if c.seed else ""))


def offsets(case):
    return np.concatenate([[case.head], case.head + np.cumsum(case.sizes)]).astype(np.int64)


def rows(case):
    return case.head + sum(case.sizes) + case.tail


def plan(case, routes=True):
    """lcrec_debug_sinkhorn_groups_plan for the row: the dict of lcrec_amd.ops.sinkhorn_groups_plan.  Host code, no GPU."""
    import lcrec_amd
    return lcrec_amd.ops.sinkhorn_groups_plan(case.K, offsets(case), has_context=case.context, routes=routes)


def sk_class(g, K):
    """The size class of a group, restated: what the table's shapes were chosen by (the plan is the authority)."""
    q = g * K
    for cls, bound in enumerate((2048, 4096, 8192)):
        if q <= bound:
            return cls
    if q <= 16384 and (q + ((g + 1) & ~1) + K) * 8 + LDS_STATIC <= LDS_LIMIT:
        return 3
    return SLAB if g <= 4096 else BATCH


# ---- the path properties: name -> predicate(case, plan)
def _sizes_in(c, p, cls):
    return [g for g, (k, _pos, _off) in zip(c.sizes, p["routes"]) if k == cls]


def _lds_sizes(c, p):
    return [g for g, (k, _pos, _off) in zip(c.sizes, p["routes"]) if 0 <= k <= 3]


def _any_lds(pred):
    return lambda c, p: any(pred(g, c.K) for g in _lds_sizes(c, p))


PROPERTIES = {}
for _e in (16, 32, 64):
    PROPERTIES[f"lds_e{_e}"] = lambda c, p, _e=_e: c.e == _e and bool(_lds_sizes(c, p))          # sk_small_kernel<E, false, 256>
    PROPERTIES[f"slab_e{_e}"] = lambda c, p, _e=_e: c.e == _e and p["cls"][SLAB]["groups"] > 0   # sk_small_kernel<E, true, 1024>
for _cls in range(4):
    PROPERTIES[f"class_{_cls}"] = lambda c, p, _cls=_cls: p["cls"][_cls]["groups"] > 0
    # the class's largest group is not its first: LDS is sized by maxg, not by the group's own size
    PROPERTIES[f"class_{_cls}_largest_not_first"] = (lambda c, p, _cls=_cls: len(_sizes_in(c, p, _cls)) >= 2
                                                     and _sizes_in(c, p, _cls)[0] < max(_sizes_in(c, p, _cls)))
for _b in (2048, 4096, 8192, 16384):
    PROPERTIES[f"at_bound_{_b}"] = lambda c, p, _b=_b: any(g * c.K == _b for g in c.sizes)
    PROPERTIES[f"one_row_above_{_b}"] = lambda c, p, _b=_b: any((g - 1) * c.K == _b for g in c.sizes)
PROPERTIES.update({
    # code counts
    "K16_most_threads_idle": lambda c, p: c.K == 16 and bool(_lds_sizes(c, p)),
    "K100_no_multiple_of_64": lambda c, p: c.K == 100 and bool(_lds_sizes(c, p)),
    "K256": lambda c, p: c.K == 256 and bool(_lds_sizes(c, p)),
    "K1024_lds_four_columns_a_thread": lambda c, p: c.K == 1024 and bool(_lds_sizes(c, p)),
    "K1100_slab_two_columns_a_thread": lambda c, p: c.K == 1100 and p["cls"][SLAB]["groups"] > 0,
    # group sizes of the LDS form (256 threads: four waves; the column loop takes eight rows at a time, then a tail)
    "g1_degenerate": _any_lds(lambda g, K: g == 1),
    "g2": _any_lds(lambda g, K: g == 2),
    "g3": _any_lds(lambda g, K: g == 3),
    "fewer_rows_than_waves": _any_lds(lambda g, K: g < 4),
    "more_rows_than_waves": _any_lds(lambda g, K: g > 4),
    "g_8m": _any_lds(lambda g, K: g >= 8 and g % 8 == 0),
    "g_8m_plus_1": _any_lds(lambda g, K: g > 8 and g % 8 == 1),
    "g_8m_plus_7": _any_lds(lambda g, K: g > 8 and g % 8 == 7),
    "g_odd": _any_lds(lambda g, K: g > 1 and g % 2 == 1),
    "fewer_entries_than_threads": _any_lds(lambda g, K: g * K < 256),
    "entries_no_multiple_of_threads": _any_lds(lambda g, K: g * K > 256 and g * K % 256 != 0),
    # table order
    "classes_interleaved": lambda c, p: any(a > b >= 0 for (a, _p, _o), (b, _q, _r) in zip(p["routes"], p["routes"][1:]) if a <= SLAB),
    "empty_group_between": lambda c, p: any(g == 0 for g in c.sizes[1:-1]),
    "first_offset_positive": lambda c, p: c.head > 0,
    "last_offset_below_n": lambda c, p: c.tail > 0,
    # the slab form (1024 threads: sixteen waves)
    "slab_two_or_more": lambda c, p: p["slab_ok"] == 1 and p["cls"][SLAB]["groups"] >= 2,
    "slab_smallest_K256": lambda c, p: c.K == 256 and 65 in _sizes_in(c, p, SLAB),
    "slab_smallest_K1100": lambda c, p: c.K == 1100 and 15 in _sizes_in(c, p, SLAB),
    "slab_whole_eights": lambda c, p: any(g % 8 == 0 for g in _sizes_in(c, p, SLAB)),
    "slab_tail_of_1": lambda c, p: any(g % 8 == 1 for g in _sizes_in(c, p, SLAB)),
    "slab_tail_of_7": lambda c, p: any(g % 8 == 7 for g in _sizes_in(c, p, SLAB)),
    "slab_more_rows_than_waves": lambda c, p: any(g > 16 for g in _sizes_in(c, p, SLAB)),
    "slab_second_slice_offset": lambda c, p: any(k == SLAB and off > 0 for k, _pos, off in p["routes"]),
    "lone_slab_sized_group_takes_batch_path": lambda c, p: (p["slab_ok"] == 0 and p["batch_groups"] == 1
                                                            and sk_class(p["batch_biggest"], c.K) == SLAB),
    "lds_slab_and_batch_sized": lambda c, p: (bool(_lds_sizes(c, p)) and p["cls"][SLAB]["groups"] > 0 and p["batch_groups"] > 0
                                              and p["batch_biggest"] > 4096),
    # transports of the group table
    "table_as_argument": lambda c, p: p["transport"] == ARGUMENT,
    "table_as_argument_four_groups": lambda c, p: p["transport"] == ARGUMENT and p["table_groups"] == 4,
    "table_by_ring": lambda c, p: p["transport"] == RING and c.context,
    "table_by_ring_five_groups": lambda c, p: p["transport"] == RING and p["table_groups"] == 5,
    "table_synchronous": lambda c, p: p["transport"] == SYNCHRONOUS and not c.context,
    # helper streams
    "fork_none_with_context": lambda c, p: c.context and p["fork_mask"] == 0 and p["table_groups"] > 0,
    "fork_slab_only": lambda c, p: p["fork_mask"] == 1,
    "fork_mid_only": lambda c, p: p["fork_mask"] == 2,
    "fork_both": lambda c, p: p["fork_mask"] == 3,
    "no_context": lambda c, p: not c.context and p["fork_mask"] == 0,
    # the launches
    "lds_attribute_raised": lambda c, p: any(k["set_attribute"] for k in p["cls"][:4]),
    "lds_attribute_not_needed": lambda c, p: any(k["groups"] and not k["set_attribute"] for k in p["cls"][:4]),
    "label_tiny": lambda c, p: any(k["label"] == "sinkhorn_tiny" for k in p["cls"]),
    "label_small": lambda c, p: any(k["label"] == "sinkhorn_small" for k in p["cls"]),
    "label_slab": lambda c, p: any(k["label"] == "sinkhorn_slab" for k in p["cls"]),
    # output and settings
    "idx_stride_3": lambda c, p: c.stride == 3,
    "eps_0.003": lambda c, p: c.eps == 0.003,
    "eps_0.05": lambda c, p: c.eps == 0.05,
    "iters_50": lambda c, p: c.iters == 50,
    "iters_3": lambda c, p: c.iters == 3,
    "iters_1": lambda c, p: c.iters == 1,
})
REQUIRED = frozenset(PROPERTIES)

# ---- the table.  expect: groups / maxg per class 0 .. 4, batch = (groups, largest), transport, fork, slab_ok
_ALL_LDS_256 = [2, 8, 0, 9, 3, 16, 17, 0, 32, 1, 33, 64, 5, 7, 15, 23]      # K = 256: every class, its bound and one row above it
_MIXED_256 = [65, 2, 72, 12, 71, 65]                                      # K = 256: three classes and the slab, interleaved
_ITER_256 = [2, 3, 9, 17, 40, 65, 66]
CASES = [
    _case(256, 32, _ALL_LDS_256, head=3, tail=2, stride=3,
          covers=["lds_e32", "K256", "class_0", "class_1", "class_2", "class_3", "class_0_largest_not_first", "class_1_largest_not_first",
                  "class_2_largest_not_first", "class_3_largest_not_first", "at_bound_2048", "one_row_above_2048", "at_bound_4096",
                  "one_row_above_4096", "at_bound_8192", "one_row_above_8192", "at_bound_16384", "g1_degenerate", "g2", "g3",
                  "fewer_rows_than_waves", "more_rows_than_waves", "g_8m", "g_8m_plus_1", "g_8m_plus_7", "g_odd", "classes_interleaved",
                  "empty_group_between", "first_offset_positive", "last_offset_below_n", "table_by_ring", "fork_mid_only",
                  "lds_attribute_raised", "lds_attribute_not_needed", "label_tiny", "label_small", "idx_stride_3", "eps_0.003", "iters_50"],
          groups=(6, 3, 3, 2, 0), maxg=(8, 16, 32, 64, 0), batch=(0, 0), transport=RING, fork=2, slab_ok=0),
    _case(256, 32, _ALL_LDS_256, head=3, tail=2, stride=3, context=False,
          covers=["table_synchronous", "no_context", "lds_e32"],
          groups=(6, 3, 3, 2, 0), maxg=(8, 16, 32, 64, 0), batch=(0, 0), transport=SYNCHRONOUS, fork=0, slab_ok=0),
    _case(256, 32, _MIXED_256, head=1,
          covers=["slab_e32", "slab_two_or_more", "slab_smallest_K256", "slab_whole_eights", "slab_tail_of_1", "slab_tail_of_7",
                  "slab_more_rows_than_waves", "slab_second_slice_offset", "one_row_above_16384", "fork_both", "table_by_ring",
                  "classes_interleaved", "label_slab"],
          groups=(1, 1, 0, 0, 4), maxg=(2, 12, 0, 0, 72), batch=(0, 0), transport=RING, fork=3, slab_ok=1),
    _case(256, 32, _MIXED_256, head=1, context=False,
          covers=["slab_e32", "table_synchronous", "no_context"],
          groups=(1, 1, 0, 0, 4), maxg=(2, 12, 0, 0, 72), batch=(0, 0), transport=SYNCHRONOUS, fork=0, slab_ok=1),
    _case(256, 32, [65, 65], covers=["slab_smallest_K256", "slab_two_or_more", "table_as_argument", "fork_none_with_context"],
          groups=(0, 0, 0, 0, 2), maxg=(0, 0, 0, 0, 65), batch=(0, 0), transport=ARGUMENT, fork=0, slab_ok=1),
    _case(256, 32, [65, 2, 65, 3], tail=1, covers=["fork_slab_only", "table_as_argument_four_groups"],
          groups=(2, 0, 0, 0, 2), maxg=(3, 0, 0, 0, 65), batch=(0, 0), transport=ARGUMENT, fork=1, slab_ok=1),
    _case(256, 32, [65, 2, 65, 3, 4], tail=1, covers=["fork_slab_only", "table_by_ring_five_groups"],
          groups=(3, 0, 0, 0, 2), maxg=(4, 0, 0, 0, 65), batch=(0, 0), transport=RING, fork=1, slab_ok=1),
    _case(256, 32, [70, 3], covers=["lone_slab_sized_group_takes_batch_path", "table_as_argument"],
          groups=(1, 0, 0, 0, 0), maxg=(3, 0, 0, 0, 0), batch=(1, 70), transport=ARGUMENT, fork=0, slab_ok=0),
    # K = 16: a group of up to 15 rows has fewer entries than the workgroup has threads; 128 / 256 / 512 / 1024 rows are the bounds;
    # 4097 rows is the smallest batch-sized group of all
    _case(16, 16, [4097, 1025, 129, 1030, 128, 1, 257, 256, 513, 512, 1024, 5, 100], head=2, tail=3,
          covers=["lds_e16", "slab_e16", "K16_most_threads_idle", "lds_slab_and_batch_sized", "fewer_entries_than_threads", "at_bound_2048",
                  "one_row_above_2048", "at_bound_4096", "one_row_above_4096", "at_bound_8192", "one_row_above_8192", "at_bound_16384",
                  "one_row_above_16384", "slab_more_rows_than_waves", "fork_both", "table_by_ring", "slab_tail_of_1"],
          groups=(4, 2, 2, 2, 2), maxg=(128, 256, 512, 1024, 1030), batch=(1, 4097), transport=RING, fork=3, slab_ok=1),
    # K = 1024 in LDS: a thread owns four columns; from 17 rows the slab
    _case(1024, 64, [1, 2, 3, 4, 5, 8, 9, 16, 17, 20, 24], eps=0.05, head=1,
          covers=["lds_e64", "slab_e64", "K1024_lds_four_columns_a_thread", "eps_0.05", "at_bound_2048", "one_row_above_2048",
                  "at_bound_4096", "one_row_above_4096", "at_bound_8192", "one_row_above_8192", "at_bound_16384", "one_row_above_16384",
                  "fork_both"],
          groups=(2, 2, 2, 2, 3), maxg=(2, 4, 8, 16, 24), batch=(0, 0), transport=RING, fork=3, slab_ok=1),
    _case(1024, 64, [1, 2, 3, 4, 5, 8, 9, 16, 17, 20, 24], head=1, covers=["lds_e64", "slab_e64", "eps_0.003"],
          groups=(2, 2, 2, 2, 3), maxg=(2, 4, 8, 16, 24), batch=(0, 0), transport=RING, fork=3, slab_ok=1),
    # K = 1100 in the slab: a thread owns two columns (76 of them: one), slices of 17 616, 17 616 and 26 424 doubles
    # (seed 1: with seed 0 one row of the 14-row group has its second and third place within a rounding error of each other)
    _case(1100, 32, [15, 3, 15, 14, 23, 1, 7], tail=2, seed=1,
          covers=["K1100_slab_two_columns_a_thread", "slab_smallest_K1100", "slab_two_or_more", "slab_tail_of_7", "slab_second_slice_offset",
                  "entries_no_multiple_of_threads", "lds_attribute_raised"],
          groups=(1, 1, 1, 1, 3), maxg=(1, 3, 7, 14, 23), batch=(0, 0), transport=RING, fork=3, slab_ok=1),
    # K = 100: no multiple of the wave; g K no multiple of the workgroup
    _case(100, 16, [1, 2, 3, 20, 21, 40, 41, 81, 82, 163, 164, 170], head=5,
          covers=["K100_no_multiple_of_64", "lds_e16", "entries_no_multiple_of_threads", "fewer_entries_than_threads", "g_8m_plus_1",
                  "g_odd", "slab_e16"],
          groups=(4, 2, 2, 2, 2), maxg=(20, 40, 81, 163, 170), batch=(0, 0), transport=RING, fork=3, slab_ok=1),
]
for _eps, _it in ((0.003, 3), (0.003, 1), (0.05, 50), (0.05, 3), (0.05, 1)):
    CASES.append(_case(256, 32, _ITER_256, eps=_eps, iters=_it, covers=[f"iters_{_it}", f"eps_{_eps}"],
                       groups=(2, 1, 1, 1, 2), maxg=(3, 9, 17, 40, 66), batch=(0, 0), transport=RING, fork=3, slab_ok=1))

# the six calls made back to back with no synchronisation between them (the context's ring has four slots): rows whose table
# goes through the ring, all different
BACK_TO_BACK = [0, 2, 6, 8, 11, 12]


def check_claims(case, p):
    """What of `case`'s expect / covers does NOT hold for plan `p`: a list of messages that name the field."""
    got = {"groups": tuple(k["groups"] for k in p["cls"]), "maxg": tuple(k["maxg"] for k in p["cls"]),
           "batch": (p["batch_groups"], p["batch_biggest"]), "transport": p["transport"], "fork": p["fork_mask"], "slab_ok": p["slab_ok"]}
    bad = [f"{key}: the plan gives {got.get(key)}, the row says {want}" for key, want in case.expect.items() if got.get(key) != want]
    for name in case.covers:
        if not PROPERTIES[name](case, p):
            bad.append(f"property {name} does not hold")
    return bad


# ---- inputs and the reference
def inputs(case):
    """(z [n, e], codebook [K, e]) fp32: Gaussian rows and a Gaussian codebook; every second group is a tight cluster
    z[first] + 1e-3 noise, as colliding items are."""
    offs, n = offsets(case), rows(case)
    rs = np.random.RandomState(1000 * case.seed + case.K + case.e + n + len(case.sizes))
    z = rs.standard_normal((n, case.e)).astype(np.float32)
    for g in range(0, len(case.sizes), 2):
        lo, hi = offs[g], offs[g + 1]
        if hi > lo:
            z[lo:hi] = z[lo] + 1e-3 * rs.standard_normal((hi - lo, case.e)).astype(np.float32)
    cb = (0.8 * rs.standard_normal((case.K, case.e))).astype(np.float32)
    return z, cb


def solve(cen, eps, iters, skip_tail=0, jitter=None):
    """layers.py:85-108 in fp64 with sequential sums taken from the far end (np.cumsum adds in order).  jitter: a RandomState; every
    exp(.) is moved by -1 / 0 / +1 ulp.  skip_tail (to perturb): the last `skip_tail` rows are left out of every column sum."""
    g, K = cen.shape
    Q = np.exp(-cen.astype(np.float64) / np.float64(eps))
    if jitter is not None:
        k = jitter.randint(-1, 2, size=Q.shape)
        Q = np.where(k > 0, np.nextafter(Q, np.inf), np.where(k < 0, np.nextafter(Q, 0.0), Q))
    Q = Q / Q.ravel()[::-1].cumsum()[-1]
    for _ in range(iters):
        Q = Q / Q[:, ::-1].cumsum(axis=1)[:, -1:]
        Q = Q / np.float64(g)
        Q = Q / Q[:g - skip_tail][::-1].cumsum(axis=0)[-1:]
        Q = Q / np.float64(K)
    return Q * np.float64(g)


def top_last(Q):
    """sk.top with the HIGHEST index taken among tied maxima (to perturb)."""
    K = Q.shape[1]
    t = sk.top(np.asarray(Q)[:, ::-1])
    return sk.Top(K - 1 - t.winner, K - 1 - t.runner, t.ratio, t.margin, t.gap)


Reference = namedtuple("Reference", "winner runner ratio ratio64 exact_one tol grouped evaluations reference_distance")


def _tops(cen, eps, iters, seed):
    """The three fp64 evaluations of one group, and the longdouble solve's Top."""
    import torch
    from oracle import torch_ref
    a = sk.top(sk.solve(cen, eps, iters, np.float64))
    b = sk.top(solve(cen, eps, iters, jitter=np.random.RandomState(seed)))
    c = sk.top(torch_ref.sinkhorn(torch.from_numpy(cen).double(), eps, iters).numpy())
    return (a, b, c), sk.top(sk.solve(cen, eps, iters))


@functools.lru_cache(maxsize=None)
def _reference(K, e, sizes, eps, iters, head, tail, seed):
    case = Case(K, e, sizes, eps, iters, True, 1, head, tail, seed, {}, ())
    z, cb = inputs(case)
    offs, n = offsets(case), rows(case)
    winner, runner = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    ratio, ratio64, tol = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    exact_one, grouped = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    evaluations, worst = [], 0.0
    for g, size in enumerate(sizes):
        if size == 0:
            continue
        lo, hi = offs[g], offs[g + 1]
        (a, b, c), yard = _tops(sk.centred(z[lo:hi], cb), eps, iters, 7919 * seed + g)
        dist = sk.distance(c.ratio, yard.ratio)
        worst = max(worst, dist)
        winner[lo:hi], runner[lo:hi], ratio[lo:hi], ratio64[lo:hi] = c.winner, c.runner, yard.ratio, c.ratio
        tol[lo:hi] = SLACK * max(dist, FLOOR)
        exact_one[lo:hi] = (a.ratio == 1.0) & (b.ratio == 1.0) & (c.ratio == 1.0)
        grouped[lo:hi] = True
        evaluations.append((g, a, b, c))
    return Reference(winner, runner, ratio, ratio64, exact_one, tol, grouped, evaluations, worst)


def reference(case):
    """Per row of the input: the fp64 reference's winner and runner-up (oracle/torch_ref.sinkhorn on the row's group), the
    longdouble solve's second / best (ratio) and the fp64 reference's (ratio64), whether the ratio is exactly 1.0 in all three fp64 evaluations, the ratio tolerance of the
    row's group, and whether the row belongs to a group at all.  Computed once per problem and shared: treat as read-only."""
    return _reference(case.K, case.e, case.sizes, case.eps, case.iters, case.head, case.tail, case.seed)


def conditions(case):
    """What of the row's inputs makes a verdict depend on rounding, under the reference alone: a list of messages (empty: the
    three fp64 evaluations agree on every row's winner and runner-up, and every ratio is a positive finite number)."""
    ref = reference(case)
    bad = []
    for g, a, b, c in ref.evaluations:
        for name, other in (("reversed sums, jittered exp", b), ("numpy fp64", a)):
            for what, x, y in (("winner", other.winner, c.winner), ("runner-up", other.runner, c.runner)):
                if not np.array_equal(x, y):
                    bad.append(f"group {g} ({case.sizes[g]} rows): the {what} of {int((x != y).sum())} rows differs between "
                               f"torch_ref.sinkhorn and the evaluation with {name}")
    r = ref.ratio[ref.grouped]
    if not (np.isfinite(r).all() and (r > sk.MIN_RATIO).all()):
        bad.append(f"second / best of the longdouble solve is not in ({sk.MIN_RATIO}, inf) on every row: min {np.nanmin(r)!r}")
    return bad


def judge(case, winner, runner, ratio):
    """A solve of the row (arrays over all n rows of the input) against the reference: None when every grouped row's winner and
    runner-up are the fp64 reference's, its ratio is within the group's tolerance of the longdouble solve's and exactly 1.0
    where the reference's is, and every row of no group still holds its sentinel (-1, -1, NaN); else a message."""
    ref = reference(case)
    offs = offsets(case)
    winner, runner, ratio = np.asarray(winner), np.asarray(runner), np.asarray(ratio, dtype=np.float64)
    in_g = ref.grouped
    msg = []

    def where(row):
        g = int(np.searchsorted(offs, row, side="right") - 1)
        size = case.sizes[g]
        return (f"row {row} = row {row - offs[g]} of group {g} ({size} rows, class {sk_class(size, case.K)}, {size * case.K} entries, "
                f"{size % 8} rows in the column loop's tail)")
    for what, got, want in (("winners", winner, ref.winner), ("runner-ups", runner, ref.runner)):
        bad = np.flatnonzero((got != want) & in_g)
        if len(bad):
            msg.append(f"{what} differ on {len(bad)} of {int(in_g.sum())} grouped rows, first {where(int(bad[0]))}: got "
                       f"{int(got[bad[0]])}, want {int(want[bad[0]])}")
    err = np.where(in_g, np.abs(ratio - np.where(in_g, ref.ratio, 1.0)) / np.where(in_g, ref.ratio, 1.0), 0.0)
    err = np.where(np.isfinite(err), err, np.inf)
    bad = np.flatnonzero(err > np.where(in_g, ref.tol, 0.0))
    if len(bad):
        w = int(bad[err[bad].argmax()])
        msg.append(f"second / best is beyond the tolerance on {len(bad)} rows, worst {where(w)}: got {ratio[w]!r}, want "
                   f"{ref.ratio[w]!r}, off by {err[w]:.3e} relative, tolerance {ref.tol[w]:.3e}")
    bad = np.flatnonzero(ref.exact_one & (ratio != 1.0))
    if len(bad):
        msg.append(f"second / best is not exactly 1.0 on {len(bad)} of {int(ref.exact_one.sum())} rows where every fp64 evaluation "
                   f"gives 1.0, first {where(int(bad[0]))}: got {ratio[bad[0]]!r}")
    out = ~in_g
    touched = np.flatnonzero(out & ((winner != -1) | (runner != -1) | ~np.isnan(ratio)))
    if len(touched):
        msg.append(f"{len(touched)} rows that belong to no group were written, first row {int(touched[0])}")
    return None if not msg else "\n  ".join([case_id(case)] + msg)


# ---- the hazards: name -> the groups of a row the perturbation applies to (empty: the row is not exposed)
def _two_largest(case):
    order = sorted((g for g, s in enumerate(case.sizes) if s >= 2), key=lambda g: -case.sizes[g])
    return order[:2] if len(order) >= 2 else []


HAZARDS = {
    # (the rows with 3 iterations and with 1 are there for this.  After 50 the iteration has contracted to a rounding error on many
    # groups -- the tight clusters, and everything at eps = 0.05, as tests/sinkhorn_cases.py finds for the batch-sized table --
    # so a solve that stops one short is not wrong there, and no judge of values could say it is.)
    "one_iteration_fewer": lambda case: [g for g, s in enumerate(case.sizes) if s >= 2] if case.iters <= 3 else [],
    "tail_rows_left_out_of_column_sums": lambda case: [g for g, s in enumerate(case.sizes) if s > 8 and s % 8],
    "highest_tied_index": lambda case: [g for g, a, b, c in reference(case).evaluations if (c.ratio == 1.0).any()],
    "two_groups_swapped": _two_largest,
}


def perturbed(case, hazard, groups):
    """(winner, runner, ratio) over all n rows: the fp64 reference with `groups` solved wrongly the way `hazard` names."""
    ref = reference(case)
    z, cb = inputs(case)
    offs = offsets(case)
    winner, runner, ratio = ref.winner.copy(), ref.runner.copy(), ref.ratio64.copy()
    if hazard == "two_groups_swapped":
        # the first rows of the two groups carry each other's result
        a, b = offs[groups[0]], offs[groups[1]]
        for arr in (winner, runner, ratio):
            arr[a], arr[b] = arr[b], arr[a]
        return winner, runner, ratio
    for g in groups:
        lo, hi = offs[g], offs[g + 1]
        cen = sk.centred(z[lo:hi], cb)
        if hazard == "one_iteration_fewer":
            t = sk.top(sk.solve(cen, case.eps, case.iters - 1, np.float64))
        elif hazard == "tail_rows_left_out_of_column_sums":
            t = sk.top(solve(cen, case.eps, case.iters, skip_tail=case.sizes[g] % 8))
        elif hazard == "highest_tied_index":
            t = top_last(sk.solve(cen, case.eps, case.iters, np.float64))
        else:
            raise KeyError(hazard)
        winner[lo:hi], runner[lo:hi], ratio[lo:hi] = t.winner, t.runner, t.ratio
    return winner, runner, ratio
