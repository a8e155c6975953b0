"""The case table of the batch-sized Sinkhorn solvers (sinkhorn_big of csrc/vq_train.hip: sk_scaling_kernel, sk_persistent_kernel
and the multi-launch sk_init / sk_iter / sk_final kernels), shared by tests/test_sinkhorn_plan_host.py (CPU: every row reaches the
kernel and the paths it claims, its inputs are judgeable, and the judge refuses wrong solves) and tests/test_gpu_sinkhorn_forms.py
(GPU: every row's winners, runner-ups and second / best ratios against the reference).

A row is (B, K, e, eps, iters, form) -- form as in include/lcrec.h (0 production's choice, 1 scaling with XCD-local sets, 2 scaling
at agent scope, 3 persistent, 4 multi-launch) -- with the plan lcrec_debug_sinkhorn_plan must give for it (`expect`) and the kernel
paths it exists for (`covers`, names of PROPERTIES).  Each property is a predicate over the row and its plan, so a row cannot claim
a path its shape does not reach, and REQUIRED lists the paths some row must keep claiming.  Shapes are the smallest that reach
their path; the dispatch, not this file, decides what a shape reaches.

Values: the yardstick is the reference's loop (index/models/layers.py:85-108) in numpy.longdouble over the same fp32 centred
distances the kernels start from; a solver's second / best ratios may sit SLACK times further from it than the fp64 reference
(oracle/torch_ref.sinkhorn) does on that row, but not closer than FLOOR is asked of it (tests/f11_check.py's rule)."""
import functools
from collections import namedtuple

import numpy as np

AUTO, SCALING_LOCAL, SCALING_AGENT, PERSISTENT, MULTI = 0, 1, 2, 3, 4
SCALING = (SCALING_LOCAL, SCALING_AGENT)
FORM_NAMES = {SCALING_LOCAL: "scaling form, eight XCD-local sets (sk_scaling_kernel)",
              SCALING_AGENT: "scaling form, one set at agent scope (sk_scaling_kernel)",
              PERSISTENT: "persistent in-place form (sk_persistent_kernel)",
              MULTI: "multi-launch solver (sk_init_kernel / sk_iter_kernel / sk_final_kernel)"}
TRACE_LABEL = "sinkhorn"             # the trace label of every batch-sized solver

# ---- the tolerance: measured, not chosen (recomputed and compared by tests/test_sinkhorn_plan_host.py)
SLACK = 4.0                          # tests/f11_check.py: this many times further from the yardstick than the fp64 reference is
# largest distance, over the rows of CASES, of oracle/torch_ref.sinkhorn in fp64 from the longdouble yardstick: 9.08e-14, on
# 1100 x 1000; 4e-14 .. 9e-14 on every row at eps = 0.003, 1e-15 .. 5e-15 at eps = 0.05 (exp(-d / eps) carries the rounding of
# d / eps times |d / eps| <= 333).  A row is judged by its OWN distance; this is the largest of them.
MEASURED = 9.1e-14
# largest distance, over the rows of CASES, between the in-place form and the scaling form, both in numpy fp64: what two correct
# fp64 solvers differ by, so no solver is asked to be closer than this to anything: 1.68e-14, on 3230 x 100
FLOOR = 1.7e-14

# the conditions a row's inputs meet under the reference alone, so that the GPU test excludes no row
MIN_MARGIN = 1e-6                    # smallest relative top-2 margin, and smallest relative gap between second and third place
MIN_RATIO = 1e-250                   # no second / best ratio near the denormals

Case = namedtuple("Case", "B K e eps iters form stride seed expect covers")


def _case(B, K, e, eps, iters, ask, covers, stride=1, seed=0, **expect):
    return Case(B, K, e, eps, iters, ask, stride, seed, expect, tuple(covers))


def case_id(c):
    return f"{c.B}x{c.K}-e{c.e}-eps{c.eps}-it{c.iters}-f{c.form}" + (f"-stride{c.stride}" if c.stride != 1 else "")


# ---- the path properties: name -> predicate(case, plan)
def _is(form, cpl=None, rw=None):
    forms = form if isinstance(form, tuple) else (form,)
    return lambda c, p: p["form"] in forms and (cpl is None or (p["cpl"], p["rw"]) == (cpl, rw))


SCALING_PAIRS = [(1, 2), (1, 4), (1, 8), (2, 2), (2, 4), (2, 8), (2, 16), (4, 2), (4, 4), (4, 8), (4, 16), (8, 2), (8, 4), (8, 8),
                 (16, 2), (16, 4)]
# sk_persistent_kernel<4, 1> is instantiated too: only LCREC_SK_RW=1 (a tuning knob) reaches it, and no row does
PERSISTENT_PAIRS = [(1, 4), (2, 4), (4, 2), (4, 4), (8, 2), (16, 1)]
PERSISTENT_KNOB_ONLY = [(4, 1)]

PROPERTIES = {}
for _c, _r in SCALING_PAIRS:
    PROPERTIES[f"scaling_{_c}_{_r}"] = _is(SCALING, _c, _r)                                # sk_scaling_kernel<CPL, RW>
for _c, _r in PERSISTENT_PAIRS:
    PROPERTIES[f"persistent_{_c}_{_r}"] = _is(PERSISTENT, _c, _r)                          # sk_persistent_kernel<CPL, RW>
    # ... as lcrec_sinkhorn_assign reaches it on its own: any codebook size that is no multiple of 64
    PROPERTIES[f"persistent_{_c}_{_r}_by_default"] = (lambda c, p, _c=_c, _r=_r: c.form == AUTO and p["batch_route"] == 1
                                                      and _is(PERSISTENT, _c, _r)(c, p))
PROPERTIES.update({
    # sk_scaling_kernel
    "scaling_eight_sets": lambda c, p: p["form"] == SCALING_LOCAL and p["sets"] == 8,       # ranks by XCC_ID, plain stores, `done`
    "scaling_one_set": lambda c, p: p["form"] == SCALING_AGENT and p["sets"] == 1,
    "scaling_256_workgroups": lambda c, p: p["form"] == SCALING_LOCAL and p["sets"] * p["workgroups"] == 256,
    "scaling_64_workgroups_one_set": lambda c, p: p["form"] == SCALING_AGENT and p["workgroups"] == 64,
    "scaling_padded_cpl4": lambda c, p: p["form"] in SCALING and p["cpl"] == 4 and p["padded_columns"] > 0,     # `j < K` guards
    "scaling_padded_cpl8": lambda c, p: p["form"] in SCALING and p["cpl"] == 8 and p["padded_columns"] > 0,
    "scaling_padded_cpl16": lambda c, p: p["form"] in SCALING and p["cpl"] == 16 and p["padded_columns"] > 0,
    "scaling_ragged_wave": lambda c, p: p["form"] in SCALING and p["ragged_wave"] == 1,     # a_mine = 0 for rows past B
    "scaling_ragged_workgroup": lambda c, p: p["form"] in SCALING and p["ragged_workgroup"] == 1,
    "scaling_whole_workgroups": lambda c, p: p["form"] in SCALING and p["ragged_workgroup"] == 0,
    "scaling_gather_split": lambda c, p: p["form"] in SCALING and c.K < 512,                # several threads share a column
    "scaling_gather_unsplit": lambda c, p: p["form"] in SCALING and c.K >= 512,
    "scaling_gather_rounds": lambda c, p: (p["form"] in SCALING                             # more than one round of eight polls
                                           and -(-p["workgroups"] // max(1, 512 // c.K)) > 8),
    "scaling_not_routed_by_assign": lambda c, p: p["form"] in SCALING and p["batch_route"] == 0,   # <1, 2>: see CASES
    # sk_persistent_kernel
    "persistent_padded": lambda c, p: p["form"] == PERSISTENT and p["padded_columns"] > 0,
    "persistent_idle_owners": lambda c, p: p["form"] == PERSISTENT and c.K < p["workgroups"],      # owned == 0
    "persistent_several_owned": lambda c, p: p["form"] == PERSISTENT and c.K >= 2 * p["workgroups"],
    "persistent_unequal_owned": lambda c, p: p["form"] == PERSISTENT and c.K > p["workgroups"] and c.K % p["workgroups"] != 0,
    "persistent_ragged_wave": lambda c, p: p["form"] == PERSISTENT and p["ragged_wave"] == 1,
    "persistent_ragged_workgroup": lambda c, p: p["form"] == PERSISTENT and p["ragged_workgroup"] == 1,
    "persistent_128_workgroups": lambda c, p: p["form"] == PERSISTENT and p["workgroups"] == 128,  # SKP_MAX_BLOCKS, skp_fits
    "persistent_owner_sum_16": lambda c, p: p["form"] == PERSISTENT and p["workgroups"] >= 16 and p["workgroups"] % 16 != 0,
    "persistent_forced_fallback": lambda c, p: c.form == PERSISTENT,          # what runs when the scaling launch is refused
    # the multi-launch solver
    "multi_by_default": lambda c, p: c.form == AUTO and p["form"] == MULTI and p["batch_route"] == 1,
    "multi_forced": lambda c, p: c.form == MULTI,
    "multi_padded": lambda c, p: p["form"] == MULTI and p["padded_columns"] > 0,
    "multi_ragged_workgroup": lambda c, p: p["form"] == MULTI and p["ragged_workgroup"] == 1,
    # the output
    "idx_stride_3": lambda c, p: c.stride == 3,
})
for _f, _forms in (("scaling", (SCALING_LOCAL,)), ("persistent", (PERSISTENT,))):
    # a one-iteration solve (`it == 0` on its own), the first re-arms of the three rotating exchange buffers, the reference's
    # own default of 100 iterations; and an epsilon at which nothing is sharp
    for _it in (1, 2, 3, 4, 100):
        PROPERTIES[f"{_f}_iters_{_it}"] = lambda c, p, _it=_it, _forms=_forms: p["form"] in _forms and c.iters == _it
    PROPERTIES[f"{_f}_eps_0.05"] = lambda c, p, _forms=_forms: p["form"] in _forms and c.eps == 0.05
for _f, _form in (("scaling_agent", SCALING_AGENT), ("multi", MULTI)):
    # the same first iterations on the other two solvers: the agent-scope stores of the scaling form; sk_iter_kernel's mode 0
    # alone, then the first and second toggle of its two column-partial buffers
    for _it in (1, 2, 3):
        PROPERTIES[f"{_f}_iters_{_it}"] = lambda c, p, _it=_it, _form=_form: p["form"] == _form and c.iters == _it
REQUIRED = frozenset(PROPERTIES)     # every path above must be claimed by at least one row of CASES

# ---- the hazards: what a wrong solver could do that an argmax over Gaussian inputs does not show.  name -> predicate(case,
# plan): the rows on which the judge must refuse the reference perturbed that way (tests/test_sinkhorn_plan_host.py).
HAZARDS = {
    # (at eps = 0.05 the iteration contracts fast: after 50 of them one more moves no ratio by a rounding error, so a solve
    # that stops one short is not wrong there, and no judge of values could say it is)
    "one_iteration_fewer": lambda c, p: c.eps < 0.01 or c.iters <= 4,
    "epsilon_off_by_1e-6": lambda c, p: True,
    "amplitude_without_1e-5": lambda c, p: True,
    "workgroup_partial_dropped": lambda c, p: p["workgroups"] >= 2,
    # (from the second iteration on: a padded column's scale is still 1 when the first row sums are formed, where its E = 1
    # disappears beside the real entries; its own column normalisation is what makes it heavy afterwards)
    "padded_columns_included": lambda c, p: p["padded_columns"] > 0 and c.iters >= 2,
}

# ---- the table.  expect: form, kernel = (CPL, RW), workgroups (per set), sets; and where the row is there for them, padded
# (columns), ragged = (last wave, last workgroup)
_S, _P = "scaling", "persistent"
CASES = [
    # sk_scaling_kernel: K % 64 == 0; RW 2 / 4 / 8 / 16 for B <= 256 / 512 / 1024 / 2048; eight sets from 257 rows up (RW = 2
    # never: 24 workgroups' worth of rows would be needed for 16).  Every shape that admits both set counts has both.
    # <1, 2>: K = 64 with B <= 256 is at most 16 384 entries, which lcrec_sinkhorn_assign solves in one workgroup's LDS -- the
    # dispatch can choose this instantiation but only the debug entry brings it a problem
    _case(130, 64, 16, 0.003, 50, SCALING_AGENT, ["scaling_1_2", "scaling_one_set", "scaling_not_routed_by_assign", "scaling_gather_split"],
          form=SCALING_AGENT, kernel=(1, 2), workgroups=9, sets=1, ragged=(0, 1)),
    _case(257, 64, 32, 0.003, 50, AUTO, ["scaling_1_4", "scaling_eight_sets", "scaling_ragged_wave", "scaling_ragged_workgroup"],
          form=SCALING_LOCAL, kernel=(1, 4), workgroups=9, sets=8, ragged=(1, 1)),            # the smallest shape with eight sets
    _case(257, 64, 32, 0.003, 50, SCALING_AGENT, ["scaling_1_4", "scaling_one_set", "scaling_ragged_wave"],
          form=SCALING_AGENT, kernel=(1, 4), workgroups=9, sets=1, ragged=(1, 1)),
    _case(600, 64, 16, 0.003, 50, AUTO, ["scaling_1_8", "scaling_eight_sets"],
          form=SCALING_LOCAL, kernel=(1, 8), workgroups=10, sets=8, ragged=(0, 1)),
    _case(600, 64, 16, 0.003, 50, SCALING_AGENT, ["scaling_1_8", "scaling_one_set"],
          form=SCALING_AGENT, kernel=(1, 8), workgroups=10, sets=1, ragged=(0, 1)),
    _case(130, 128, 16, 0.003, 50, AUTO, ["scaling_2_2", "scaling_one_set", "scaling_ragged_workgroup"],
          form=SCALING_AGENT, kernel=(2, 2), workgroups=9, sets=1, ragged=(0, 1)),
    _case(300, 128, 64, 0.003, 50, AUTO, ["scaling_2_4", "scaling_eight_sets"],
          form=SCALING_LOCAL, kernel=(2, 4), workgroups=10, sets=8, ragged=(0, 1)),
    _case(300, 128, 64, 0.003, 50, SCALING_AGENT, ["scaling_2_4", "scaling_one_set"],
          form=SCALING_AGENT, kernel=(2, 4), workgroups=10, sets=1, ragged=(0, 1)),
    _case(700, 128, 16, 0.003, 50, AUTO, ["scaling_2_8", "scaling_eight_sets", "scaling_ragged_wave"],
          form=SCALING_LOCAL, kernel=(2, 8), workgroups=11, sets=8, ragged=(1, 1)),
    _case(700, 128, 16, 0.003, 50, SCALING_AGENT, ["scaling_2_8", "scaling_one_set"],
          form=SCALING_AGENT, kernel=(2, 8), workgroups=11, sets=1, ragged=(1, 1)),
    _case(1030, 128, 16, 0.003, 50, AUTO, ["scaling_2_16", "scaling_eight_sets", "scaling_ragged_wave"],
          form=SCALING_LOCAL, kernel=(2, 16), workgroups=9, sets=8, ragged=(1, 1)),
    _case(1030, 128, 16, 0.003, 50, SCALING_AGENT, ["scaling_2_16", "scaling_one_set"],
          form=SCALING_AGENT, kernel=(2, 16), workgroups=9, sets=1, ragged=(1, 1)),
    # K = 192 / 320 / 576: one / three / seven of the lane's columns are padding.  (Fewer rows than columns at eps = 0.003
    # saturates -- a column that one row dominates ends at exactly 1 / K in that row, and a row holds several such: exact ties
    # in the reference itself -- so the rows with B < K, here and below, use eps = 0.05.)
    _case(130, 192, 16, 0.003, 50, AUTO, ["scaling_4_2", "scaling_padded_cpl4", "scaling_one_set"],
          form=SCALING_AGENT, kernel=(4, 2), workgroups=9, sets=1, padded=64, ragged=(0, 1)),
    _case(300, 192, 16, 0.003, 50, AUTO, ["scaling_4_4", "scaling_padded_cpl4", "scaling_eight_sets"],
          form=SCALING_LOCAL, kernel=(4, 4), workgroups=10, sets=8, padded=64, ragged=(0, 1)),
    _case(300, 192, 16, 0.003, 50, SCALING_AGENT, ["scaling_4_4", "scaling_padded_cpl4", "scaling_one_set"],
          form=SCALING_AGENT, kernel=(4, 4), workgroups=10, sets=1, padded=64, ragged=(0, 1)),
    _case(300, 192, 16, 0.003, 50, AUTO, ["idx_stride_3", "scaling_4_4"], stride=3,
          form=SCALING_LOCAL, kernel=(4, 4), workgroups=10, sets=8, padded=64, ragged=(0, 1)),
    _case(600, 192, 16, 0.003, 50, AUTO, ["scaling_4_8", "scaling_padded_cpl4", "scaling_eight_sets"],
          form=SCALING_LOCAL, kernel=(4, 8), workgroups=10, sets=8, padded=64, ragged=(0, 1)),
    _case(600, 192, 16, 0.003, 50, SCALING_AGENT, ["scaling_4_8", "scaling_padded_cpl4", "scaling_one_set"],
          form=SCALING_AGENT, kernel=(4, 8), workgroups=10, sets=1, padded=64, ragged=(0, 1)),
    _case(1030, 192, 16, 0.003, 50, AUTO, ["scaling_4_16", "scaling_padded_cpl4", "scaling_eight_sets", "scaling_ragged_wave"],
          form=SCALING_LOCAL, kernel=(4, 16), workgroups=9, sets=8, padded=64, ragged=(1, 1)),
    _case(1030, 192, 16, 0.003, 50, SCALING_AGENT, ["scaling_4_16", "scaling_padded_cpl4", "scaling_one_set"],
          form=SCALING_AGENT, kernel=(4, 16), workgroups=9, sets=1, padded=64, ragged=(1, 1)),
    _case(130, 320, 16, 0.05, 50, AUTO, ["scaling_8_2", "scaling_padded_cpl8", "scaling_one_set"],
          form=SCALING_AGENT, kernel=(8, 2), workgroups=9, sets=1, padded=192, ragged=(0, 1)),
    _case(300, 320, 32, 0.003, 50, AUTO, ["scaling_8_4", "scaling_padded_cpl8", "scaling_eight_sets"],
          form=SCALING_LOCAL, kernel=(8, 4), workgroups=10, sets=8, padded=192, ragged=(0, 1)),
    _case(300, 320, 32, 0.003, 50, SCALING_AGENT, ["scaling_8_4", "scaling_padded_cpl8", "scaling_one_set"],
          form=SCALING_AGENT, kernel=(8, 4), workgroups=10, sets=1, padded=192, ragged=(0, 1)),
    _case(600, 320, 16, 0.003, 50, AUTO, ["scaling_8_8", "scaling_padded_cpl8", "scaling_eight_sets"],
          form=SCALING_LOCAL, kernel=(8, 8), workgroups=10, sets=8, padded=192, ragged=(0, 1)),
    _case(600, 320, 16, 0.003, 50, SCALING_AGENT, ["scaling_8_8", "scaling_padded_cpl8", "scaling_one_set"],
          form=SCALING_AGENT, kernel=(8, 8), workgroups=10, sets=1, padded=192, ragged=(0, 1)),
    _case(130, 576, 16, 0.05, 50, AUTO, ["scaling_16_2", "scaling_padded_cpl16", "scaling_one_set", "scaling_gather_unsplit"],
          form=SCALING_AGENT, kernel=(16, 2), workgroups=9, sets=1, padded=448, ragged=(0, 1)),
    _case(300, 576, 16, 0.05, 50, AUTO, ["scaling_16_4", "scaling_padded_cpl16", "scaling_eight_sets", "scaling_gather_rounds"],
          form=SCALING_LOCAL, kernel=(16, 4), workgroups=10, sets=8, padded=448, ragged=(0, 1)),
    _case(300, 576, 16, 0.05, 50, SCALING_AGENT, ["scaling_16_4", "scaling_padded_cpl16", "scaling_one_set"],
          form=SCALING_AGENT, kernel=(16, 4), workgroups=10, sets=1, padded=448, ragged=(0, 1)),
    # the training step's own shape, and the two largest launches the form makes
    _case(1024, 256, 32, 0.003, 50, AUTO, ["scaling_4_8", "scaling_eight_sets", "scaling_whole_workgroups"],
          form=SCALING_LOCAL, kernel=(4, 8), workgroups=16, sets=8, padded=0, ragged=(0, 0)),
    _case(1000, 1024, 16, 0.003, 50, AUTO, ["scaling_256_workgroups", "scaling_16_4", "scaling_gather_rounds", "scaling_gather_unsplit"],
          form=SCALING_LOCAL, kernel=(16, 4), workgroups=32, sets=8, padded=0, ragged=(0, 1)),
    _case(2048, 1024, 16, 0.003, 50, AUTO, ["scaling_64_workgroups_one_set", "scaling_16_4", "scaling_gather_rounds",
                                            "scaling_whole_workgroups"],
          form=SCALING_AGENT, kernel=(16, 4), workgroups=64, sets=1, padded=0, ragged=(0, 0)),

    # sk_persistent_kernel as lcrec_sinkhorn_assign reaches it: any K that is no multiple of 64.  K = 48 and 100 with more
    # workgroups than columns (some own no column sum); K >= 130 cannot have that (at most 128 workgroups)
    _case(1600, 48, 16, 0.003, 50, AUTO, ["persistent_1_4", "persistent_1_4_by_default", "persistent_padded", "persistent_idle_owners"],
          form=PERSISTENT, kernel=(1, 4), workgroups=50, sets=1, padded=16, ragged=(0, 0)),
    _case(3230, 100, 16, 0.003, 50, AUTO, ["persistent_2_4", "persistent_2_4_by_default", "persistent_idle_owners", "persistent_ragged_wave",
                                           "persistent_owner_sum_16"],
          form=PERSISTENT, kernel=(2, 4), workgroups=101, sets=1, padded=28, ragged=(1, 1)),
    _case(300, 100, 16, 0.003, 50, AUTO, ["persistent_2_4", "persistent_2_4_by_default", "persistent_padded", "persistent_several_owned"],
          form=PERSISTENT, kernel=(2, 4), workgroups=10, sets=1, padded=28, ragged=(0, 1)),
    _case(300, 200, 32, 0.003, 50, AUTO, ["persistent_4_2", "persistent_4_2_by_default", "persistent_padded", "persistent_unequal_owned",
                                          "persistent_owner_sum_16"],
          form=PERSISTENT, kernel=(4, 2), workgroups=19, sets=1, padded=56, ragged=(0, 1)),
    _case(2049, 130, 16, 0.003, 50, AUTO, ["persistent_4_4", "persistent_4_4_by_default", "persistent_padded", "persistent_ragged_wave",
                                           "persistent_ragged_workgroup"],
          form=PERSISTENT, kernel=(4, 4), workgroups=65, sets=1, padded=126, ragged=(1, 1)),
    _case(100, 300, 64, 0.05, 50, AUTO, ["persistent_8_2", "persistent_8_2_by_default", "persistent_padded", "persistent_several_owned"],
          form=PERSISTENT, kernel=(8, 2), workgroups=7, sets=1, padded=212, ragged=(0, 1)),
    _case(60, 1000, 16, 0.05, 50, AUTO, ["persistent_16_1", "persistent_16_1_by_default", "persistent_padded", "persistent_several_owned"],
          form=PERSISTENT, kernel=(16, 1), workgroups=8, sets=1, padded=24, ragged=(0, 1)),
    _case(1024, 1000, 16, 0.003, 50, AUTO, ["persistent_16_1", "persistent_128_workgroups", "persistent_padded"],
          form=PERSISTENT, kernel=(16, 1), workgroups=128, sets=1, padded=24, ragged=(0, 0)),
    # ... and as the fallback that runs when the scaling launch is refused
    _case(1024, 256, 32, 0.003, 50, PERSISTENT, ["persistent_forced_fallback", "persistent_4_2"],
          form=PERSISTENT, kernel=(4, 2), workgroups=64, sets=1, padded=0, ragged=(0, 0)),
    _case(600, 1024, 16, 0.05, 50, PERSISTENT, ["persistent_forced_fallback", "persistent_16_1", "persistent_owner_sum_16"],
          form=PERSISTENT, kernel=(16, 1), workgroups=75, sets=1, padded=0, ragged=(0, 0)),

    # the multi-launch solver: more rows than 128 workgroups of the persistent kernel hold, K no multiple of 64
    _case(1100, 1000, 16, 0.003, 50, AUTO, ["multi_by_default", "multi_padded", "multi_ragged_workgroup"],
          form=MULTI, kernel=(16, 4), workgroups=35, sets=1, padded=24, ragged=(0, 1)),
    _case(4100, 48, 16, 0.003, 50, AUTO, ["multi_by_default", "multi_padded"],
          form=MULTI, kernel=(1, 4), workgroups=129, sets=1, padded=16, ragged=(0, 1)),
    _case(1024, 256, 32, 0.003, 50, MULTI, ["multi_forced"],
          form=MULTI, kernel=(4, 4), workgroups=32, sets=1, padded=0, ragged=(0, 0)),
]
# iteration and epsilon edges on one scaling shape (300 x 192: eight sets, a padded lane column, a ragged last workgroup) and one
# persistent shape (300 x 100).  eps >= 0.0015 always: exp(1 / eps) must stay finite in fp64.
for _eps in (0.003, 0.05):
    for _it in (1, 2, 3, 4, 100):
        _extra = ["_eps_0.05"] if _eps == 0.05 else []
        # (seed 1: with seed 0 row 169 of the one- to four-iteration solves is within 1e-8 of a tie)
        CASES.append(_case(300, 192, 16, _eps, _it, AUTO, [f"{_S}_iters_{_it}"] + [_S + x for x in _extra], seed=1,
                           form=SCALING_LOCAL, kernel=(4, 4), workgroups=10, sets=8, padded=64, ragged=(0, 1)))
        CASES.append(_case(300, 100, 16, _eps, _it, AUTO, [f"{_P}_iters_{_it}"] + [_P + x for x in _extra],
                           form=PERSISTENT, kernel=(2, 4), workgroups=10, sets=1, padded=28, ragged=(0, 1)))
for _it in (1, 2, 3):
    CASES.append(_case(300, 192, 16, 0.003, _it, SCALING_AGENT, [f"scaling_agent_iters_{_it}"], seed=1,
                       form=SCALING_AGENT, kernel=(4, 4), workgroups=10, sets=1, padded=64, ragged=(0, 1)))
    CASES.append(_case(300, 100, 16, 0.003, _it, MULTI, [f"multi_iters_{_it}"],
                       form=MULTI, kernel=(2, 4), workgroups=10, sets=1, padded=28, ragged=(0, 1)))


def plan(case):
    """lcrec_debug_sinkhorn_plan for the row: the dict of lcrec_amd.ops.sinkhorn_plan.  Host code of the library, no GPU."""
    import lcrec_amd
    return lcrec_amd.ops.sinkhorn_plan(case.B, case.K, case.iters, case.form)


def check_claims(case, p):
    """What of `case`'s expect / covers does NOT hold for plan `p`: a list of messages that name the field (empty: the row
    tests what it says)."""
    got = {"form": p["form"], "kernel": (p["cpl"], p["rw"]), "workgroups": p["workgroups"], "sets": p["sets"],
           "padded": p["padded_columns"], "ragged": (p["ragged_wave"], p["ragged_workgroup"])}
    bad = [f"{key}: the plan gives {got.get(key)}, the row says {want}" for key, want in case.expect.items() if got.get(key) != want]
    for name in case.covers:
        if not PROPERTIES[name](case, p):
            bad.append(f"property {name} does not hold")
    return bad


# ---- inputs and the reference
def inputs(case):
    """(z [B, e], codebook [K, e]) fp32: Gaussian latents and a Gaussian codebook, seeded per shape and the row's `seed` (a
    seed whose inputs miss a condition of conditions() is replaced by the next, never the condition)."""
    rs = np.random.RandomState(1000 * case.seed + case.B + case.K + case.e)
    z = rs.standard_normal((case.B, case.e)).astype(np.float32)
    cb = (0.8 * rs.standard_normal((case.K, case.e))).astype(np.float32)
    return z, cb


def centred(z, cb, plus=1e-5):
    """vq.py:51-61 in fp32 over the C oracle's fp32 distances: what every solver exponentiates.  `plus`: the 1e-5 of the
    amplitude (0 only to perturb)."""
    from oracle import cpu_oracle
    d = cpu_oracle.distances(z, cb)
    hi, lo = d.max(), d.min()
    mid = (hi + lo) / np.float32(2)
    amp = hi - mid + np.float32(plus)
    return ((d - mid) / amp).astype(np.float32)


def solve(cen, eps, iters, dtype=np.longdouble, drop=None, extra_ones=0):
    """layers.py:85-108 as written -- Q = exp(-d / eps); Q /= sum; iters x {Q /= rowsum; Q /= B; Q /= colsum; Q /= K}; Q *= B --
    in `dtype`.  To perturb: drop = (row slice, column): the last iteration's sum of that column misses those rows;
    extra_ones: that many more columns with exp(.) = 1 take part (B and K as divisors stay), cut off the result."""
    B, K = cen.shape
    Q = np.exp(-cen.astype(dtype) / dtype(eps))
    if extra_ones:
        Q = np.concatenate([Q, np.ones((B, extra_ones), dtype=dtype)], axis=1)
    Q /= Q.sum(axis=1, keepdims=True).sum(axis=0, keepdims=True)
    for it in range(iters):
        Q /= Q.sum(axis=1, keepdims=True)
        Q /= dtype(B)
        col = Q.sum(axis=0, keepdims=True)
        if drop is not None and it == iters - 1:
            col[0, drop[1]] -= Q[drop[0], drop[1]].sum()
        Q /= col
        Q /= dtype(K)
    Q *= dtype(B)
    return Q[:, :K]


def solve_scaling(cen, eps, iters):
    """The scaling form of the same loop in numpy fp64: E fixed, a_i = 1 / (B sum_j E_ij b_j), b_j = 1 / (K sum_i a_i E_ij);
    E_ij b_j differs from the in-place Q_ij by a factor per row, so the rows' order and second / best are the same."""
    B, K = cen.shape
    E = np.exp(-cen.astype(np.float64) / np.float64(eps))
    b = np.ones(K)
    for _ in range(iters):
        a = 1.0 / (B * (E @ b))
        b = 1.0 / (K * (a @ E))
    return E * b[None, :]


Top = namedtuple("Top", "winner runner ratio margin gap")


def top(Q):
    """Per row of Q: winner (first maximum), runner-up (first maximum of the rest), second / best as fp64, and the relative
    gaps first-second and second-third."""
    Q = np.array(Q)
    rows = np.arange(Q.shape[0])
    w = Q.argmax(axis=1)
    best = Q[rows, w].copy()
    Q[rows, w] = -1
    r = Q.argmax(axis=1)
    second = Q[rows, r].copy()
    Q[rows, r] = -1
    third = Q.max(axis=1)
    return Top(w.astype(np.int64), r.astype(np.int64), (second / best).astype(np.float64),
               ((best - second) / best).astype(np.float64), ((second - third) / second).astype(np.float64))


def distance(ratio, want):
    """How far a solve's second / best ratios are from `want`'s: the largest relative difference over the rows."""
    return float(np.max(np.abs(np.asarray(ratio, dtype=np.float64) - want) / want))


Reference = namedtuple("Reference", "yardstick reference_distance floor_distance")


@functools.lru_cache(maxsize=None)
def _reference(B, K, e, eps, iters, seed):
    import torch
    from oracle import torch_ref
    case = Case(B, K, e, eps, iters, 0, 1, seed, {}, ())
    cen = centred(*inputs(case))
    yard = top(solve(cen, eps, iters))
    # the measure: the fp64 reference as the oracle restates it (checked against the imported reference by
    # tests/test_oracle_golden.py), over the reference's own fp32 centring
    from oracle import cpu_oracle
    cen_t = torch_ref.centre_distances(torch.from_numpy(cpu_oracle.distances(*inputs(case))))
    assert np.array_equal(cen_t.numpy(), cen), "centred() must restate torch_ref.centre_distances bit for bit"
    ref = top(torch_ref.sinkhorn(cen_t.double(), eps, iters).numpy())
    floor = distance(top(solve_scaling(cen, eps, iters)).ratio, top(solve(cen, eps, iters, np.float64)).ratio)
    return Reference(yard, distance(ref.ratio, yard.ratio), floor)


def reference(case):
    """The yardstick's Top for the row's inputs (longdouble), the fp64 reference's distance from it, and the distance between
    the two fp64 forms; computed once per distinct problem and shared (treat as read-only)."""
    return _reference(case.B, case.K, case.e, case.eps, case.iters, case.seed)


def conditions(case):
    """What of the row's inputs makes a verdict depend on rounding, under the reference alone: a list of messages (empty: every
    row of the problem can be judged, none is excluded)."""
    y = reference(case).yardstick
    bad = []
    if not y.margin.min() > MIN_MARGIN:
        bad.append(f"smallest top-2 margin {y.margin.min():.3e} (row {int(y.margin.argmin())}) is not above {MIN_MARGIN}")
    if not y.gap.min() > MIN_MARGIN:
        bad.append(f"smallest gap between second and third {y.gap.min():.3e} (row {int(y.gap.argmin())}) is not above {MIN_MARGIN}")
    if not y.ratio.min() > MIN_RATIO:
        bad.append(f"smallest ratio {y.ratio.min():.3e} is not above {MIN_RATIO}")
    return bad


def tolerance(case):
    return SLACK * max(reference(case).reference_distance, FLOOR)


def judge(case, p, winner, runner, ratio):
    """A solve of the row against the yardstick: None when its winners and runner-ups are the yardstick's on every row and its
    ratios are within tolerance(case); else a message that says which, how far, and where the worst row sits in plan `p`."""
    y = reference(case).yardstick
    winner, runner, ratio = np.asarray(winner), np.asarray(runner), np.asarray(ratio, dtype=np.float64)
    tol = tolerance(case)
    msg = []
    worst = None
    if not np.array_equal(winner, y.winner):
        rows = np.flatnonzero(winner != y.winner)
        worst = int(rows[0])
        msg.append(f"winners differ on {len(rows)} of {case.B} rows, first row {worst}: got {int(winner[worst])}, want "
                   f"{int(y.winner[worst])} (the yardstick's margin there: {y.margin[worst]:.3e})")
    if not np.array_equal(runner, y.runner):
        rows = np.flatnonzero(runner != y.runner)
        worst = int(rows[0]) if worst is None else worst
        msg.append(f"runner-ups differ on {len(rows)} of {case.B} rows, first row {int(rows[0])}: got {int(runner[rows[0]])}, want "
                   f"{int(y.runner[rows[0]])} (the yardstick's second-third gap there: {y.gap[rows[0]]:.3e})")
    err = np.abs(ratio - y.ratio) / y.ratio
    err = np.where(np.isfinite(err), err, np.inf)
    if not err.max() <= tol:
        worst = int(err.argmax()) if worst is None else worst
        msg.append(f"second / best is off by {err.max():.3e} relative (row {int(err.argmax())}: got {ratio[err.argmax()]!r}, want "
                   f"{y.ratio[err.argmax()]!r}); {int((err > tol).sum())} rows are beyond the tolerance {tol:.3e} = {SLACK:g} x max(the fp64 "
                   f"reference's own {reference(case).reference_distance:.3e}, floor {FLOOR:.3e})")
    if not msg:
        return None
    return "\n  ".join([f"{case_id(case)}: {FORM_NAMES[p['form']]}"] + msg + [where(case, p, worst, int(runner[worst]))])


def where(case, p, row, runner_col):
    """Row `row` of the problem and the column the solver named its runner-up, in the kernel's own coordinates."""
    rows_wg, rw = p["rows_per_workgroup"], p["rw"]
    wg, in_wg = divmod(row, rows_wg)
    tail = case.B - case.B % rows_wg if p["ragged_workgroup"] else case.B
    col = (f"lane {runner_col % 64}, lane-column {runner_col // 64} of {p['cpl']}" if 0 <= runner_col < 64 * p["cpl"]
           else "outside the lane columns")
    return (f"row {row}: workgroup {wg} of {p['workgroups']}" + (f" (in each of {p['sets']} sets)" if p["sets"] > 1 else "")
            + f", wave {in_wg // rw}, row {in_wg % rw} of the wave's {rw}; runner-up column {runner_col}: {col}, "
            + ("a PADDED column" if runner_col >= case.K else "not a padded column")
            + f"; the row {'sits' if row >= tail else 'does not sit'} in the ragged tail (rows from {tail})")


def perturbed(case, p, hazard):
    """(winner, runner, ratio) of the reference's loop in fp64 made wrong the way `hazard` names."""
    z, cb = inputs(case)
    cen = centred(z, cb)
    if hazard == "one_iteration_fewer":
        Q = solve(cen, case.eps, case.iters - 1, np.float64)
    elif hazard == "epsilon_off_by_1e-6":
        Q = solve(cen, case.eps * (1 + 1e-6), case.iters, np.float64)
    elif hazard == "amplitude_without_1e-5":
        Q = solve(centred(z, cb, plus=0.0), case.eps, case.iters, np.float64)
    elif hazard == "workgroup_partial_dropped":
        # the last workgroup's partial, out of the sum of the column its last row wins
        lo = (p["workgroups"] - 1) * p["rows_per_workgroup"]
        Q = solve(cen, case.eps, case.iters, np.float64, drop=(slice(lo, case.B), int(reference(case).yardstick.winner[-1])))
    elif hazard == "padded_columns_included":
        Q = solve(cen, case.eps, case.iters, np.float64, extra_ones=p["padded_columns"])
    else:
        raise KeyError(hazard)
    t = top(Q)
    return t.winner, t.runner, t.ratio
