"""Rows for the tile hand-over of linear_fwd_pp3_kernel (csrc/gemm_f32.hip) beyond tests/gemm_pp_cases.py: the two epilogue
switch combinations no row there has (each of the eight is an instantiation of its own), a list of three tiles (`prev` handed
over twice in a row), lists of 2..4 tiles over the holes of the XCD-aware numbering -- and one row of special values (NaN,
+-inf, zero rows, -0.0 in front of the ReLU) in the first and the last row panel.

Shared by tests/test_gemm_pp_handover_plan_host.py (CPU: every row's plan is what it claims) and
tests/test_gpu_gemm_pp_handover.py (GPU: every element bit for bit against the oracle).  Case, plan, check_claims, inputs
and localise are those of gemm_pp_cases."""
import numpy as np

import gemm_pp_cases as pp

# properties of a planned launch beyond gemm_pp_cases.PROPERTIES
EXTRA_PROPERTIES = {
    "pp3_hand_over_twice": lambda c, h: h["form"] == pp.PERSISTENT and h["list_min"] >= 3,   # every list: prev -> prev again
    "pp3_steady_twice": lambda c, h: h["form"] == pp.PERSISTENT and h["steady_iterations"] == 2,
    "pp3_no_relu_no_bias": lambda c, h: h["form"] == pp.PERSISTENT and not c.relu and not c.bias,
}

_LIN_NOBIAS = dict(form=pp.PERSISTENT, head=4096, tail=0, k_tiles=14, steady=1, lists=(2, 2), empty=0, last_panel=256)

CASES = [
    # the two (relu, bn, bias) combinations gemm_pp_cases has no row for
    pp.Case(4096, 448, 4096, False, True, False, _LIN_NOBIAS,
            ("pp3_has_bn", "pp3_no_relu", "pp3_no_bias", "pp3_no_relu_no_bias", "pp3_hand_over", "pp3_steady_once")),
    pp.Case(4096, 448, 4096, False, False, False, _LIN_NOBIAS,
            ("pp3_no_bn", "pp3_no_relu", "pp3_no_bias", "pp3_no_relu_no_bias", "pp3_hand_over", "pp3_steady_once")),
    # 24 panels x 32 column tiles = 768 tiles on 256 workgroups: every list has three, the middle one is handed over from a
    # tile that was itself handed over to
    pp.Case(6144, 512, 4096, True, False, True,
            dict(form=pp.PERSISTENT, head=6144, tail=0, k_tiles=16, steady=2, lists=(3, 3), empty=0, last_panel=256),
            ("pp3_no_bn", "pp3_hand_over", "pp3_hand_over_twice", "pp3_steady_twice")),
    # 12 panels x 64 column tiles: 768 tiles numbered over 16 panels (1 024 virtual tiles), lists of 2..4
    pp.Case(3072, 448, 8192, True, True, True,
            dict(form=pp.PERSISTENT, head=3072, tail=0, k_tiles=14, steady=1, lists=(2, 4), empty=0, last_panel=256),
            ("pp3_has_bn", "pp3_hand_over", "pp3_xcd_holes", "pp3_unequal_lists", "pp3_steady_once")),
]

# the special-value row: relu / bn / bias, lists of two (the first row panel is handed over, the last is stored by finish())
SPECIAL = pp.Case(4096, 448, 4096, True, True, True,
                  dict(form=pp.PERSISTENT, head=4096, tail=0, k_tiles=14, steady=1, lists=(2, 2), empty=0, last_panel=256),
                  ("pp3_has_bn", "pp3_hand_over", "pp3_steady_once"))
# rows of a panel that get special activations: offset in the panel -> what the row holds
SPECIAL_ROWS = {3: "nan", 17: "+inf", 40: "-inf", 77: "zero", 78: "zero", 130: "one +inf", 131: "one -inf", 200: "nan",
                255: "zero"}
NEG_SCALE_ZERO_COLUMNS = slice(5, None, 16)      # bias 0, bn_scale < 0, bn_shift -0.0: a zero row reaches the ReLU as -0.0
NEG_SCALE_COLUMNS = slice(9, None, 16)           # bn_scale < 0 with the row's own bias and shift


def check_claims(case, launches):
    """gemm_pp_cases.check_claims, with the names of EXTRA_PROPERTIES understood too"""
    known = case._replace(covers=tuple(n for n in case.covers if n in pp.PROPERTIES))
    bad = pp.check_claims(known, launches)
    if launches and not bad:
        for name in case.covers:
            if name in EXTRA_PROPERTIES and not EXTRA_PROPERTIES[name](case, launches[0]):
                bad.append(f"property {name} does not hold")
            elif name not in EXTRA_PROPERTIES and name not in pp.PROPERTIES:
                bad.append(f"unknown property {name}")
    return bad


def special_inputs():
    """gemm_pp_cases.inputs(SPECIAL) with SPECIAL_ROWS written into the first and the last row panel of x, and the two column
    sets above into the epilogue vectors.  Returns (x, W, bias, bn_scale, bn_shift, {row: kind})."""
    x, W, b, sc, sh = (a.copy() for a in pp.inputs(SPECIAL))
    rows = {}
    for panel0 in (0, SPECIAL.n - pp.TILE_M):
        for off, kind in SPECIAL_ROWS.items():
            r = panel0 + off
            rows[r] = kind
            if kind == "nan":
                x[r] = np.float32("nan")
            elif kind in ("+inf", "-inf"):
                x[r] = np.float32(kind)
            elif kind == "zero":
                x[r] = 0.0
            else:                                     # one infinite activation: outputs +-inf by the sign of one weight
                x[r, 100] = np.float32(kind.split()[1])
    b[NEG_SCALE_ZERO_COLUMNS] = 0.0
    sc[NEG_SCALE_ZERO_COLUMNS] = -np.abs(sc[NEG_SCALE_ZERO_COLUMNS])
    sh[NEG_SCALE_ZERO_COLUMNS] = np.float32("-0.0")
    sc[NEG_SCALE_COLUMNS] = -np.abs(sc[NEG_SCALE_COLUMNS])
    return x, W, b, sc, sh, rows
