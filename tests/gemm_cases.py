"""The case table of the generic GEMM kernels of csrc/gemm_f32.hip -- linear_tile_body in all its instantiations,
linear_s16_kernel<TB>, linear_dw_grouped_kernel<PRO> and the two split-K reducers -- shared by tests/test_gemm_plan_host.py (CPU:
every row reaches the launches it claims, the reachability sweep) and tests/test_gpu_gemm_forms.py (GPU: every row bit for bit
against the oracle), with the four launch plans (all records of lcrec_gemm_launch), the statistics reference with its bound, and
the localiser.

A row is a call of one entry point (`kind`: fwd = linear_forward, bwd = linear_backward, grp = linear_backward_weights, train =
linear_bn_forward), its sizes, its switches (`opt`), what the plan must say of it on 256 CUs (`expect`) and the paths it exists
for (`covers`, names of PROPERTIES).  Each property is a predicate over the row and its planned launches, so a row cannot claim a
path its plan does not reach; REQUIRED lists the paths some row must keep claiming.  Every row runs under default knobs."""
from collections import namedtuple

import numpy as np

import gemm_pp_cases as pp

CUS = 256
TILES = {"64x64": (2, 2, 1, 1), "128x128": (2, 2, 2, 2), "128x64": (4, 1, 1, 2), "128x32": (4, 1, 1, 1), "64x128": (2, 2, 1, 2)}
RB_TILES = ("64x64", "128x32", "64x128")                 # register-buffered when FAST (DB of linear_tile_body); the training tiles
P2_TILES = ("128x128", "128x64")                         # prefetch distance 2 in every form
U = 2.0 ** -24                                           # float32 unit roundoff


# ---------------------------------------------------------------- the plans, in one shape
def _forward_launches(n, k, out, cus):
    return [dict(l, grouped=False) for l in pp.plan(n, k, out, cus)]


def launches_of(row, ops, cus=CUS):
    """The planned launches of a row, every plan in the fields of lcrec_gemm_launch plus `grouped`; grp rows: the products of
    all problems, then the reducers' records."""
    if row.kind == "fwd":
        return _forward_launches(*row.dims, cus)
    if row.kind == "bwd":
        return [dict(l, grouped=False) for l in ops.linear_backward_plan(*row.dims, row.opt["gx"], row.opt["gw"])]
    if row.kind == "train":
        return [dict(ops.linear_bn_forward_plan(*row.dims, row.opt["pro"], row.opt["stats"]), grouped=False)]
    products, reducers, grids = ops.linear_backward_weights_plan([(n, i, o, f is not None, s) for n, i, o, f, s in row.dims])
    return [dict(l, grouped=True, grids=grids) for l in products + reducers]


def form_of(l):
    """The instantiation a launch runs, by name."""
    if l["family"] == "32x64":
        return "s16_dx" if l["w_kmajor"] else "s16_row"
    if l["family"] == "pp":
        return "pp"
    if l["family"] == "reducer":
        return "reduce_grouped" if l["grouped"] else "reduce"
    tile = f"{l['tile_rows']}x{l['tile_cols']}"
    if l["grouped"]:
        return "grouped_pro" if l["pro"] else "grouped_plain"
    if l["role"] == "forward" and (l["pro"] or l["stats"]):
        return f"train_{tile}_" + "_".join(w for w, on in (("pro", l["pro"]), ("stats", l["stats"])) if on)
    layout = "dw" if l["a_kmajor"] else "dx" if l["w_kmajor"] else "row"
    return f"{tile}_{layout}_{'fast' if l['fast'] else 'guarded'}"


def run_lengths(l):
    """K-tiles of each K-run of a product launch"""
    return [l["k_tiles_per_run"]] * (l["runs"] - 1) + [l["k_tiles_last_run"]]


# every instantiation the library builds, and the forms that cut K
FORMS = ([f"{t}_{lay}" for t in TILES for lay in ("row_fast", "row_guarded", "dx_fast", "dw_fast")] + ["s16_row", "s16_dx"]
         + ["grouped_plain", "grouped_pro"] + [f"train_{t}_{f}" for t in RB_TILES for f in ("pro_stats", "stats", "pro")])
SPLIT_FORMS = [f"{t}_dw_fast" for t in TILES] + ["grouped_plain", "grouped_pro"]
# Not reached by any shape under default knobs (tests/test_gemm_plan_host.py sweeps the rules and asserts exactly this set):
#   128x128_row_fast     everything that large with K % 32 == 0 and more than 64 columns is the ping-pong kernel's, whole or as a
#                        head whose tail is below one round and so never on 128 x 128 tiles
#   (128x128_dw_fast, S > 1), (64x128_dw_fast, S > 1)
#                        a dW on these tiles counts >= 512 tiles (64 x 128 launches as 128 x 32 tiles), and S <= 512 / tiles
UNREACHABLE = {("128x128_row_fast", False), ("128x128_dw_fast", True), ("64x128_dw_fast", True)}


# ---------------------------------------------------------------- rows
Row = namedtuple("Row", "kind dims opt expect covers")
FWD_OPT = dict(relu=False, bn=False, bias=False, inf=False)
BWD_OPT = dict(gx=True, gw=True, inf=False)
TRAIN_OPT = dict(pro=True, in_relu=True, stats=True, affine=True, running=True)


def _row(kind, dims, covers, opt=None, **expect):
    base = {"fwd": FWD_OPT, "bwd": BWD_OPT, "train": TRAIN_OPT, "grp": {}}[kind]
    return Row(kind, tuple(dims), dict(base, **(opt or {})), expect, tuple(covers))


def row_id(r):
    if r.kind == "grp":
        dims = "+".join(f"{n}.{i}.{o}{'' if f is None else f[0]}s{s}" for n, i, o, f, s in r.dims)
    else:
        dims = "-".join(str(v) for v in r.dims)
    opt = "".join(k[0] + str(int(v)) for k, v in sorted(r.opt.items()))
    return f"{r.kind}-{dims}-{opt}"


def _has(form, **want):
    """predicate: some launch of `form` with these fields (a callable value is a test of the field)"""
    def p(row, ls):
        return any(form_of(l) == form and all(v(l[k]) if callable(v) else l[k] == v for k, v in want.items()) for l in ls)
    return p


def _kt(form, count):
    return lambda row, ls: any(form_of(l) == form and count in run_lengths(l) for l in ls)


def _products(ls):
    return [l for l in ls if l["family"] in ("tile_body", "32x64")]


PROPERTIES = {}
for _f in FORMS:
    PROPERTIES[_f] = _has(_f)
# K-tile counts of a run: the prologue / ring edges of the register-buffered pipelines, the short loops of the others
KT_FORMS = {f: 9 for f in [f"{t}_{lay}" for t in RB_TILES for lay in ("row_fast", "dx_fast", "dw_fast")]
            + ["s16_row", "s16_dx", "grouped_plain", "grouped_pro"]}
KT_FORMS.update({f: 5 for f in [f"{t}_row_guarded" for t in TILES] + ["128x64_row_fast"]
                 + [f"{t}_{lay}" for t in P2_TILES for lay in ("dx_fast", "dw_fast")]})
for _f, _most in KT_FORMS.items():
    for _c in range(1, _most + 1):
        PROPERTIES[f"kt{_c}_{_f}"] = _kt(_f, _c)
_dw = lambda l: l["role"] == "dw" and l["family"] == "tile_body"
_any = lambda test: (lambda row, ls: any(test(l) for l in ls))
PROPERTIES.update({
    # dW: the contracted length is the batch
    "dw_n1": _any(lambda l: _dw(l) and l["k"] == 1),
    "dw_n31": _any(lambda l: _dw(l) and l["k"] == 31),
    "dw_n33": _any(lambda l: _dw(l) and l["k"] == 33),
    "dw_ragged_k_long": _any(lambda l: _dw(l) and l["k"] % 32 and l["k_tiles_per_run"] > 4),
    # split K
    "split_2": _any(lambda l: _dw(l) and not l["grouped"] and l["runs"] == 2),
    "split_16": _any(lambda l: _dw(l) and not l["grouped"] and l["runs"] == 16),
    "split_caller_1": lambda row, ls: row.kind == "grp" and any(s == 1 and ls[i]["runs"] == 1 for i, (_, _, _, _, s) in enumerate(row.dims)),
    "split_caller_3": lambda row, ls: row.kind == "grp" and any(s == 3 and ls[i]["runs"] == 3 for i, (_, _, _, _, s) in enumerate(row.dims)),
    "split_short_last_run": _any(lambda l: _dw(l) and l["runs"] > 1 and l["k_tiles_last_run"] < l["k_tiles_per_run"]),
    "split_last_run_one_k_tile": _any(lambda l: _dw(l) and l["runs"] > 1 and l["k_tiles_last_run"] == 1),
    "split_last_run_partial_k_tile": _any(lambda l: _dw(l) and l["runs"] > 1 and l["last_k_valid"] < 32),
    "split_ragged_tile": _any(lambda l: _dw(l) and l["runs"] > 1 and (l["last_panel_rows"] < l["tile_rows"] or l["last_tile_cols"] < l["tile_cols"])),
    "reduce_total4_not_256": _any(lambda l: form_of(l) == "reduce" and l["total4"] % 256),
    "reduce_grouped_total4_not_256": _any(lambda l: form_of(l) == "reduce_grouped" and l["total4"] % 256),
    # edges of the tile (generic kernel)
    "last_panel_1_row": _any(lambda l: l["family"] == "tile_body" and l["last_panel_rows"] == 1),
    "last_panel_bm_minus_1": _any(lambda l: l["family"] == "tile_body" and l["last_panel_rows"] == l["tile_rows"] - 1),
    "last_col_tile_4": _any(lambda l: l["family"] == "tile_body" and l["last_tile_cols"] == 4),
    "last_col_tile_bn_minus_4": _any(lambda l: l["family"] == "tile_body" and l["last_tile_cols"] == l["tile_cols"] - 4),
    "last_col_tile_odd": _any(lambda l: l["family"] == "tile_body" and l["role"] == "forward" and l["last_tile_cols"] % 2 == 1 and not l["vector_stores"]),
    "xcd_holes": _any(lambda l: l["family"] == "tile_body" and l["virtual_tiles"] > l["tiles"]),
    "no_xcd_holes": _any(lambda l: l["family"] == "tile_body" and l["virtual_tiles"] == l["tiles"]),
    "single_tile": _any(lambda l: l["family"] == "tile_body" and l["tiles"] == 1),
    "s16_last_panel_1_row": _any(lambda l: l["family"] == "32x64" and l["last_panel_rows"] == 1),
    "s16_last_col_tile_4": _any(lambda l: l["family"] == "32x64" and l["last_tile_cols"] == 4),
    "s16_single_tile": _any(lambda l: l["family"] == "32x64" and l["tiles"] == 1),
    # grouped dW
    "grouped_16_mixed": lambda row, ls: (row.kind == "grp" and len(row.dims) == 16 and len({l["tiles"] for l in ls[:16]}) >= 3
                                         and len({l["runs"] for l in ls[:16]}) >= 3 and any(l["k"] % 32 for l in ls[:16])),
    "grouped_first_last_one_tile": lambda row, ls: row.kind == "grp" and ls[0]["tiles"] == 1 == ls[len(row.dims) - 1]["tiles"] and len(row.dims) > 2,
    "grouped_fold_mix": lambda row, ls: (row.kind == "grp" and {f for _, _, _, f, _ in row.dims} >= {None, "relu", "lin"}
                                         and any(f is not None and n % 32 for n, _, _, f, _ in row.dims)),
    # training forward
    "train_n2": lambda row, ls: row.kind == "train" and row.dims[0] == 2 and row.opt["stats"],
    "train_last_tile_1_row": lambda row, ls: row.kind == "train" and row.opt["stats"] and ls[0]["last_panel_rows"] == 1 and ls[0]["tiles"] > 1,
    "train_one_row_tile": lambda row, ls: row.kind == "train" and row.opt["stats"] and ls[0]["tiles"] == -(-row.dims[2] // ls[0]["tile_cols"]),
    "train_out_36": lambda row, ls: row.kind == "train" and row.opt["stats"] and row.dims[2] == 36,
    "train_out_4": lambda row, ls: row.kind == "train" and row.opt["stats"] and row.dims[2] == 4,
    "train_in_relu_0": lambda row, ls: row.kind == "train" and row.opt["pro"] and not row.opt["in_relu"],
    "train_in_relu_1": lambda row, ls: row.kind == "train" and row.opt["pro"] and row.opt["in_relu"],
    "train_no_affine": lambda row, ls: row.kind == "train" and row.opt["stats"] and not row.opt["affine"],
    "train_no_running": lambda row, ls: row.kind == "train" and row.opt["stats"] and not row.opt["running"],
    # non-finite operands next to padding
    "inf_last_valid_row": lambda row, ls: row.kind == "fwd" and row.opt["inf"] and _products(ls)[-1]["last_panel_rows"] < _products(ls)[-1]["tile_rows"],
    # a fold whose shift is +inf in one column, on a ragged batch: rows past the batch must stay zero (0 * inf would be NaN)
    "grouped_inf_shift_ragged": lambda row, ls: row.kind == "grp" and any(f == "inf" and n % 32 for n, _, _, f, _ in row.dims),
    "inf_last_valid_k_dw": lambda row, ls: row.kind == "bwd" and row.opt["inf"] and any(_dw(l) and l["k"] % 32 for l in ls),
})
for _t in RB_TILES:
    PROPERTIES[f"train_two_chunks_{_t}"] = _has(f"train_{_t}_pro_stats", chunks=lambda c: c >= 2)
# the epilogue switches, on one generic row-major form and on the 32 x 64 kernel; every other tile: all and none
_EPI = {"none": (False, False, False), "bias": (False, False, True), "bn_relu": (True, True, True), "bn": (False, True, True),
        "relu": (True, False, True), "full": (True, True, True)}


def _epi(form, name):
    relu, bn, bias = _EPI[name]
    return lambda row, ls: (row.kind == "fwd" and (row.opt["relu"], row.opt["bn"], row.opt["bias"]) == (relu, bn, bias)
                            and any(form_of(l) == form for l in ls))


for _n in ("none", "bias", "bn_relu", "bn", "relu"):
    PROPERTIES[f"epi_{_n}_64x64_row_fast"] = _epi("64x64_row_fast", _n)
    PROPERTIES[f"epi_{_n}_s16_row"] = _epi("s16_row", _n)
for _f in ("128x32_row_fast", "64x128_row_fast", "128x64_row_fast", "128x128_row_guarded"):
    PROPERTIES[f"epi_full_{_f}"] = _epi(_f, "full")
    PROPERTIES[f"epi_none_{_f}"] = _epi(_f, "none")
UNREACHABLE_FORMS = {f for f, split in UNREACHABLE if not split}       # not reached at all, with any S
REQUIRED = frozenset(p for p in PROPERTIES if p not in UNREACHABLE_FORMS and not any(p.endswith("_" + f) for f in UNREACHABLE_FORMS))


# ---- the table.  Shapes are the smallest the dispatch rule admits for the form (worked out at each generator).
def _fwd_shape(form, k):
    """[n][k] -> [n][out] that linear_forward runs on `form`"""
    return {"64x64_row_fast": (70, k, 62), "128x32_row_fast": (200, k, 30), "64x128_row_fast": (2048, k, 1024),
            "128x64_row_fast": (32641, k, 64), "s16_row": (70, k, 68),
            "64x64_row_guarded": (70, k, 64), "128x32_row_guarded": (200, k, 32), "64x128_row_guarded": (2048, k, 1024),
            "128x64_row_guarded": (32641, k, 64), "128x128_row_guarded": (65409, k, 128)}[form]


def _bwd_shape(form, kt):
    """(n, in_dim, out_dim, gx, gw) that linear_backward runs on `form` with `kt` K-tiles in one run"""
    k = 32 * kt
    if form.endswith("dx_fast") or form == "s16_dx":
        n, i = {"64x64": (8200, 64), "128x32": (8200, 32), "64x128": (2048, 1024), "128x64": (32641, 64), "128x128": (8192, 1024),
                "s16": (70, 68)}[form.split("_")[0]]
        return (n, i, k), dict(gx=True, gw=False)
    # dW: K is the batch; one run needs fewer than 8 K-tiles or more than 256 tiles
    many = kt >= 8
    o, i = {"64x64": (1088, 1024) if many else (64, 64), "128x32": (32800, 32) if many else (64, 32), "64x128": (2048, 1024),
            "128x64": (32644, 64), "128x128": (4096, 2048)}[form.split("_")[0]]
    return (k, i, o), dict(gx=False, gw=True)


ROWS = []
for _f, _most in KT_FORMS.items():
    if _f.startswith("grouped"):
        continue
    for _c in range(1, _most + 1):
        if "_row_" in _f or _f == "s16_row":
            _k = 32 * _c if _f.endswith("fast") or _f == "s16_row" else 32 * (_c - 1) + 8
            ROWS.append(_row("fwd", _fwd_shape(_f, _k), [_f, f"kt{_c}_{_f}"], form=_f, k_tiles=_c, runs=1))
        else:
            _dims, _opt = _bwd_shape(_f, _c)
            ROWS.append(_row("bwd", _dims, [_f, f"kt{_c}_{_f}"], _opt, form=_f, k_tiles=_c, runs=1))
ROWS += [
    # ---- epilogue switches
    *[_row("fwd", (70, 64, 62), ["64x64_row_fast", f"epi_{nm}_64x64_row_fast"], dict(relu=_EPI[nm][0], bn=_EPI[nm][1], bias=_EPI[nm][2]),
           form="64x64_row_fast", k_tiles=2, runs=1) for nm in ("bias", "bn_relu", "bn", "relu")],
    _row("fwd", (70, 32, 62), ["epi_none_64x64_row_fast", "xcd_holes"],
         form="64x64_row_fast", k_tiles=1, runs=1),
    *[_row("fwd", (70, 64, 68), ["s16_row", f"epi_{nm}_s16_row"], dict(relu=_EPI[nm][0], bn=_EPI[nm][1], bias=_EPI[nm][2]),
           form="s16_row", k_tiles=2, runs=1) for nm in ("none", "bias", "bn_relu", "bn", "relu")],
    *[_row("fwd", _fwd_shape(f, k), [f"epi_{nm}_{f}"], dict(relu=_EPI[nm][0], bn=_EPI[nm][1], bias=_EPI[nm][2]), form=f, k_tiles=-(-k // 32), runs=1)
      for f, k in (("128x32_row_fast", 64), ("64x128_row_fast", 64), ("128x64_row_fast", 64), ("128x128_row_guarded", 40)) for nm in ("full", "none")],
    # ---- edges of the tile: 1 and BM - 1 rows in the last panel, 4 / BN - 4 / odd columns in the last column tile, panel counts
    _row("fwd", (129, 64, 30), ["last_panel_1_row", "xcd_holes", "128x32_row_fast"], form="128x32_row_fast", k_tiles=2, runs=1),
    _row("fwd", (127, 64, 61), ["last_panel_bm_minus_1", "last_col_tile_odd"], form="64x64_row_fast", k_tiles=2, runs=1),
    _row("fwd", (1024, 64, 644), ["last_col_tile_4", "no_xcd_holes"], form="64x64_row_fast", k_tiles=2, runs=1),
    _row("fwd", (1025, 64, 700), ["last_col_tile_bn_minus_4", "last_panel_1_row"], form="64x64_row_fast", k_tiles=2, runs=1),
    _row("fwd", (64, 64, 62), ["single_tile"], form="64x64_row_fast", k_tiles=2, runs=1),
    _row("fwd", (33, 64, 68), ["s16_last_panel_1_row", "s16_last_col_tile_4"], form="s16_row", k_tiles=2, runs=1),
    _row("fwd", (32, 64, 64), ["s16_single_tile"], form="s16_row", k_tiles=2, runs=1),
    # ---- dW: short and ragged batches
    _row("bwd", (1, 64, 64), ["dw_n1"], dict(gx=False), form="64x64_dw_fast", k_tiles=1, runs=1),
    _row("bwd", (31, 64, 64), ["dw_n31"], dict(gx=False), form="64x64_dw_fast", k_tiles=1, runs=1),
    _row("bwd", (33, 2048, 4096), ["dw_n33", "128x128_dw_fast"], dict(gx=False), form="128x128_dw_fast", k_tiles=2, runs=1),
    _row("bwd", (33, 64, 64), ["dw_n33", "s16_dx"], form="64x64_dw_fast", k_tiles=2, runs=1),
    _row("bwd", (170, 32, 64), ["dw_ragged_k_long"], dict(gx=False), form="128x32_dw_fast", k_tiles=6, runs=1),
    # ---- split K: S by the rule (2, 16), short / one-K-tile / partial last runs, ragged tiles, reducer sizes
    _row("bwd", (256, 64, 64), ["split_2"], dict(gx=False), form="64x64_dw_fast", k_tiles=8, runs=2),
    _row("bwd", (2048, 68, 36), ["split_16", "split_ragged_tile", "reduce_total4_not_256"], dict(gx=False), form="64x64_dw_fast", k_tiles=64, runs=16),
    _row("bwd", (257, 64, 64), ["split_last_run_partial_k_tile", "split_short_last_run"], dict(gx=False), form="64x64_dw_fast", k_tiles=9, runs=2),
    _row("bwd", (641, 64, 64), ["split_last_run_one_k_tile", "split_last_run_partial_k_tile", "split_short_last_run"], dict(gx=False),
         form="64x64_dw_fast", k_tiles=21, runs=5),                    # runs of 5, 5, 5, 5 and 1 K-tiles, the last with one valid k
    _row("bwd", (300, 32, 64), ["split_last_run_partial_k_tile"], dict(gx=False), form="128x32_dw_fast", k_tiles=10, runs=2),
    _row("bwd", (256, 64, 32644), ["128x64_dw_fast", "split_2"], dict(gx=False), form="128x64_dw_fast", k_tiles=8, runs=2),
    # ---- grouped dW
    _row("grp", [(40, 64, 64, None, 0), (32, 64, 64, None, 1), (64, 68, 36, None, 1), (96, 128, 132, None, 3), (128, 64, 64, None, 1),
                 (160, 256, 64, None, 1), (192, 64, 64, None, 1), (224, 64, 200, None, 1), (256, 64, 64, None, 1), (288, 64, 64, None, 1),
                 (300, 64, 64, None, 3), (2048, 64, 32, None, 0), (33, 1024, 1088, None, 0), (96, 64, 64, None, 1), (1, 64, 64, None, 0),
                 (31, 4, 4, None, 0)],
         ["grouped_plain", "grouped_16_mixed", "grouped_first_last_one_tile", "split_caller_1", "split_caller_3",
          "reduce_grouped_total4_not_256"] + [f"kt{c}_grouped_plain" for c in range(1, 10)], form="grouped_plain", k_tiles=2, runs=1),
    _row("grp", [(40, 64, 64, "relu", 1), (32, 64, 64, None, 1), (64, 68, 36, "lin", 1), (96, 128, 132, "relu", 3), (128, 64, 64, "lin", 1),
                 (160, 256, 64, "relu", 1), (192, 64, 64, None, 1), (224, 64, 200, "relu", 1), (256, 64, 64, "lin", 1), (288, 64, 64, "relu", 1),
                 (300, 64, 64, "relu", 3), (96, 64, 64, "lin", 1), (31, 4, 4, "relu", 0)],
         ["grouped_pro", "grouped_fold_mix", "grouped_first_last_one_tile"] + [f"kt{c}_grouped_pro" for c in range(1, 10)],
         form="grouped_pro", k_tiles=2, runs=1),
    _row("grp", [(40, 64, 64, "inf", 1), (70, 64, 36, "inf", 2), (64, 64, 64, None, 1)], ["grouped_inf_shift_ragged"], form="grouped_pro", k_tiles=2, runs=1),
    # ---- training forward: the three forms on the three tiles, the merge's second chunk on each, the edges of n and out
    *[_row("train", dims, [f"train_{t}_{f}"] + extra, dict(pro="pro" in f, stats="stats" in f), form=f"train_{t}_{f}", k_tiles=dims[1] // 32, runs=1)
      for t, dims, extra in (("64x64", (130, 64, 68), []), ("64x128", (2048, 32, 1024), []), ("128x32", (200, 64, 32), []))
      for f in ("pro_stats", "stats", "pro")],
    _row("train", (1601, 32, 36), ["train_two_chunks_64x64", "train_out_36", "train_last_tile_1_row", "train_in_relu_1"], form="train_64x64_pro_stats", k_tiles=1, runs=1),
    _row("train", (2048, 32, 1028), ["train_two_chunks_64x128", "train_in_relu_0"], dict(in_relu=False), form="train_64x128_pro_stats", k_tiles=1, runs=1),
    _row("train", (7809, 32, 4), ["train_two_chunks_128x32", "train_out_4", "train_last_tile_1_row"], form="train_128x32_pro_stats", k_tiles=1, runs=1),
    _row("train", (2, 32, 36), ["train_n2", "train_one_row_tile", "train_no_affine"], dict(affine=False), form="train_64x64_pro_stats", k_tiles=1, runs=1),
    _row("train", (100, 96, 32), ["train_one_row_tile", "train_no_running"], dict(running=False), form="train_128x32_pro_stats", k_tiles=3, runs=1),
    # ---- one +inf next to the padding: the last valid row of a ragged panel; the last valid k of a ragged-K dW
    _row("fwd", (70, 64, 62), ["inf_last_valid_row"], dict(inf=True, bias=True), form="64x64_row_fast", k_tiles=2, runs=1),
    _row("fwd", (33, 64, 68), ["inf_last_valid_row"], dict(inf=True), form="s16_row", k_tiles=2, runs=1),
    _row("bwd", (33, 64, 64), ["inf_last_valid_k_dw"], dict(inf=True), form="64x64_dw_fast", k_tiles=2, runs=1),
]


def _merged(rows):
    """rows with the same call (id) are one row that claims what each of them claims"""
    out = {}
    for r in rows:
        key = row_id(r)
        if key in out:
            assert out[key].expect == r.expect, key
            r = r._replace(covers=tuple(dict.fromkeys(out[key].covers + r.covers)))
        out[key] = r
    return list(out.values())


ROWS = _merged(ROWS)


def check_claims(row, launches):
    """What of `row`'s expect / covers does NOT hold for this plan: a list of messages (empty: the row tests what it says).
    expect: form (some launch runs it), and of the first launch of that form k_tiles and runs."""
    bad = []
    mine = [l for l in launches if form_of(l) == row.expect["form"]]
    if not mine:
        return [f"no launch on {row.expect['form']}: the plan runs {[form_of(l) for l in launches]}"]
    got = {"form": row.expect["form"], "k_tiles": mine[0]["k_tiles"], "runs": mine[0]["runs"]}
    for key, want in row.expect.items():
        if got.get(key) != want:
            bad.append(f"{key}: the plan gives {got.get(key)}, the row says {want}")
    for name in row.covers:
        if not PROPERTIES[name](row, launches):
            bad.append(f"property {name} does not hold")
    return bad


# ---------------------------------------------------------------- inputs
def _seed(row):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(row_id(row))) % (2 ** 31)


def fwd_inputs(row):
    """(x, W, bias | None, bn_scale | None, bn_shift | None); opt inf: one +inf in the last valid row of x"""
    n, k, out = row.dims
    rs = np.random.RandomState(_seed(row))
    x = rs.standard_normal((n, k)).astype(np.float32)
    W = (rs.standard_normal((out, k)) / np.sqrt(k)).astype(np.float32)
    b, sc, sh = pp.epilogue_vectors(namedtuple("C", "out")(out), rs)
    if row.opt["inf"]:
        x[n - 1, k // 2] = np.inf
    return x, W, (b if row.opt["bias"] else None), (sc if row.opt["bn"] else None), (sh if row.opt["bn"] else None)


def bwd_inputs(row):
    """(gy, x, W); opt inf: one +inf in the last row of x (the last valid k of the dW product)"""
    n, i, o = row.dims
    rs = np.random.RandomState(_seed(row))
    gy = rs.standard_normal((n, o)).astype(np.float32)
    x = rs.standard_normal((n, i)).astype(np.float32)
    W = (rs.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32)
    if row.opt["inf"]:
        x[n - 1, i // 2] = np.inf
    return gy, x, W


def grp_inputs(row):
    """per problem (gy, x, (scale, shift) | None); fold "inf": no clamp, the shift of column in_dim / 2 is +inf and gy is positive, so
    that this column of the gradient is +inf in the oracle and NaN as soon as a padded row's 0 meets it"""
    rs = np.random.RandomState(_seed(row))
    out = []
    for n, i, o, fold, _ in row.dims:
        gy = rs.standard_normal((n, o)).astype(np.float32)
        x = rs.standard_normal((n, i)).astype(np.float32)
        f = None if fold is None else ((0.5 + rs.uniform(size=i)).astype(np.float32), (0.3 * rs.standard_normal(i)).astype(np.float32))
        if fold == "inf":
            f[1][i // 2] = np.inf
            gy = np.abs(gy) + np.float32(0.125)
        out.append((gy, x, f))
    return out


TRAIN_EPS, TRAIN_MOMENTUM = 1e-5, 0.1
CONST_SHORT, CONST_FULL = np.float32(0.75), np.float32(0.1)


def train_inputs(row):
    """(x, in_scale, in_shift, W, b, gamma, beta, running_mean, running_var).  With statistics the first output columns are the
    adversarial ones (as far as out has room): 0 mean 1e3 with deviation 1e-2; 1 exactly constant, a short mantissa; 2 the first
    row an outlier (a bad pivot: through an input feature of its own); 3 exactly constant, a full mantissa.  Made through W and b: a zero weight row and the bias."""
    n, k, out = row.dims
    rs = np.random.RandomState(_seed(row))
    x = (rs.standard_normal((n, k)) * 1.5 + 0.3).astype(np.float32)
    sc, sh = (0.5 + rs.uniform(size=k)).astype(np.float32), (0.3 * rs.standard_normal(k)).astype(np.float32)
    W = (rs.standard_normal((out, k)) * (2.0 / (k + out)) ** 0.5).astype(np.float32)
    b = (0.1 * rs.standard_normal(out)).astype(np.float32)
    if row.opt["stats"]:
        W[0] *= np.float32(1e-2) / np.float32(np.sqrt((W[0].astype(np.float64) ** 2).sum() * 3.0))
        b[0] = 1e3
        W[1] = 0
        b[1] = CONST_SHORT
        x[:, k - 1] = 0                                      # the last input feature is column 2's alone, and set in row 0 only:
        x[0, k - 1] = 100.0                                  # t[0][2] lies far out, whatever the fold does to the rest
        W[:, k - 1] = 0
        W[2, k - 1] = 1
        W[3] = 0
        b[3] = CONST_FULL
    gamma, beta = (1 + 0.1 * rs.standard_normal(out)).astype(np.float32), (0.1 * rs.standard_normal(out)).astype(np.float32)
    rm, rv = (0.1 * rs.standard_normal(out)).astype(np.float32), (0.5 + rs.uniform(size=out)).astype(np.float32)
    return x, sc, sh, W, b, gamma, beta, rm, rv


# ---------------------------------------------------------------- the statistics of the training forward
# The kernel (linear_tile_body, STATS): per row tile T of n_T <= BM rows and per column, pivot p_T = t[first row of T],
# d_i = fl(t_i - p_T), s1 = sum d_i, s2 = sum d_i^2 (fma), in float32; the strip's last tile merges in tile order:
#   mean = (sum_T fl(n_T * fl(p_T + s1_T / n_T))) / n,   m2 = sum_T [max(s2_T - s1_T * (s1_T / n_T), 0) + n_T * (m_T - mean)^2],
#   rstd = 1 / sqrt(m2 / n + eps).
# Bound, first order in u = 2^-24, per column, with A = max |t_i - p_T(i)|, X = max |t_i|, B row tiles, g_T = m_T - mean exact:
#   d_i carries u A; a float32 sum of n_T terms adds at most (n_T - 1) u sum|d_i| <= n_T (n_T - 1) u A, the division u A more:
#       |dm_T error| <= (BM + 2) u A,   |m_T error| <= (BM + 2) u A + u X =: E_T
#   the B products n_T * m_T round by u n_T X each and their B - 1 additions by u n X each (every partial sum is below n X); the
#   division rounds by u X:
#       E_mean = E_T + (B + 2) u X
#   s2: 2 u A^2 per square from d_i's rounding and (n_T + 1) u sum d_i^2 from the fma chain; s1 * dm = s1^2 / n_T <= n_T A^2 with
#   relative error 2 (BM + 2) u + 2 u; their difference rounds by u n_T A^2: |m2_T error| <= (3 BM + 10) u n_T A^2
#   n_T * g_T^2 with g_T off by E_T + E_mean + u |g_T|: 2 n_T |g_T| (E_T + E_mean) + 4 u n_T g_T^2
#   the 2 B additions into m2 round by u m2 each, the division by n and the addition of eps by u (var + eps) each:
#       E_var = (3 BM + 10) u A^2 + (1 / n) sum_T n_T [2 |g_T| (E_T + E_mean) + 4 u g_T^2] + (2 B + 2) u (var + eps)
#   rstd lies between 1 / sqrt(var +- E_var + eps), widened by the 3 u of the addition, the root and the division.
# A factor 2 on E_mean and E_var covers the second-order terms (n_T u < 2^-17).  On the benign columns (mean ~ 0, variance ~ 1,
# all but the adversarial ones of train_inputs) the tolerances the suite used before hold wherever they are tighter (mean: 1e-5
# |mean| + 1e-6, rstd: 1e-5 rstd): min of the two.  Not on the adversarial columns: those tolerances are relative to the mean and
# to rstd, and a column whose values are 1e5 deviations from its mean apart, or whose one outlier is 60 times its mean, is
# beyond them for ANY float32 algorithm (u X alone exceeds 1e-6 there) -- the float32 restatement below shows it.
ADVERSARIAL_COLUMNS = 4


def stats_reference(t, bm, eps=TRAIN_EPS, adversarial=ADVERSARIAL_COLUMNS):
    """float64 statistics of the oracle's t [n][out] and the bounds above for row tiles of `bm` rows: dict of mean, var, rstd,
    mean_tol, rstd_lo, rstd_hi (all [out], float64).  adversarial: the first columns the earlier tolerances do not cap."""
    t64 = t.astype(np.float64)
    n = t64.shape[0]
    B = -(-n // bm)
    mean, var = t64.mean(0), t64.var(0)
    A = np.zeros_like(mean)
    between = np.zeros_like(mean)
    X = np.abs(t64).max(0)
    tiles = []
    for lo in range(0, n, bm):
        blk = t64[lo:lo + bm]
        A = np.maximum(A, np.abs(blk - blk[0]).max(0))
        tiles.append((blk.shape[0], blk.mean(0) - mean))
    E_T = (bm + 2) * U * A + U * X
    E_mean = E_T + (B + 2) * U * X
    for nt, g in tiles:
        between += nt * (2 * np.abs(g) * (E_T + E_mean) + 4 * U * g * g)
    E_var = (3 * bm + 10) * U * A * A + between / n + (2 * B + 2) * U * (var + eps)
    E_mean, E_var = 2 * E_mean, 2 * E_var
    rstd = 1.0 / np.sqrt(var + eps)
    lo = 1.0 / np.sqrt(var + E_var + eps) * (1 - 3 * U)
    hi = 1.0 / np.sqrt(np.maximum(var - E_var, 0.0) + eps) * (1 + 3 * U)
    benign = np.arange(len(mean)) >= adversarial
    lo, hi = np.where(benign, np.maximum(lo, rstd * (1 - 1e-5)), lo), np.where(benign, np.minimum(hi, rstd * (1 + 1e-5)), hi)
    return dict(mean=mean, var=var, rstd=rstd, mean_tol=np.where(benign, np.minimum(E_mean, 1e-5 * np.abs(mean) + 1e-6), E_mean),
                rstd_lo=lo, rstd_hi=hi, benign=benign)


def stats_model(t, bm, eps=TRAIN_EPS):
    """The kernel's algorithm restated in float32 numpy (sequential sums: one of the orders the bound covers): (mean, rstd, m2)"""
    f = np.float32
    n, out = t.shape
    recs = []
    for lo in range(0, n, bm):
        blk = t[lo:lo + bm]
        d = (blk - blk[0]).astype(f)
        s1, s2 = np.zeros(out, f), np.zeros(out, f)
        for r in range(d.shape[0]):
            s1 = (s1 + d[r]).astype(f)
            s2 = (d[r].astype(np.float64) * d[r] + s2).astype(f)
        recs.append((f(blk.shape[0]), blk[0].astype(f), s1, s2))
    acc = np.zeros(out, f)
    for nt, pv, s1, s2 in recs:
        acc = (acc + (nt * (pv + (s1 / nt).astype(f)).astype(f)).astype(f)).astype(f)
    mean = (acc / f(n)).astype(f)
    m2 = np.zeros(out, f)
    for nt, pv, s1, s2 in recs:
        dm = (s1 / nt).astype(f)
        m2_t = np.maximum((s2 - (s1 * dm).astype(f)).astype(f), f(0))
        d = ((pv + dm).astype(f) - mean).astype(f)
        m2 = (m2 + (m2_t + (nt * (d * d).astype(f)).astype(f)).astype(f)).astype(f)
    rstd = (f(1) / np.sqrt(((m2 / f(n)).astype(f) + f(eps)).astype(f))).astype(f)
    return mean, rstd, m2


def derived_stats(mean, rstd_and_m2, n, gamma, beta, rm0, rv0, eps=TRAIN_EPS, momentum=TRAIN_MOMENTUM):
    """scale, shift and the running statistics from the kernel's own mean, rstd and m2 / n by the expressions of
    linear_tile_body, in float32: (scale, shift, running_mean | None, running_var | None).  running_var is built from m2 / n,
    which rstd = fl(1 / fl(sqrt(fl(m2 / n + eps)))) gives back only to 5 u (var + eps) -- u from the addition, 2 u each from the
    root and the quotient, squared -- so it is returned in float64 and compared within running_var_tol."""
    f = np.float32
    rstd = rstd_and_m2
    g = np.ones_like(mean) if gamma is None else gamma
    be = np.zeros_like(mean) if beta is None else beta
    sc = (g * rstd).astype(f)
    shift = ((-mean).astype(np.float64) * sc.astype(np.float64) + be.astype(np.float64)).astype(f)      # one fma: exact product, one rounding
    rm = None if rm0 is None else ((f(1) - f(momentum)) * rm0 + f(momentum) * mean).astype(f)
    rv = None
    if rv0 is not None:
        var_b = 1.0 / rstd.astype(np.float64) ** 2 - eps                                  # biased variance, to ~3 u (var + eps)
        rv = float(f(1) - f(momentum)) * rv0.astype(np.float64) + float(f(momentum)) * var_b * n / max(n - 1, 1)
    return sc, shift, rm, rv


def running_var_tol(rstd, n, rv0, rv, momentum=TRAIN_MOMENTUM):
    """6 u on the batch term (5 u from rstd, see derived_stats, and the division by n - 1), and 4 u on the result's own float32
    steps: 1 - momentum, its product with the old value, the product with momentum, the sum"""
    return 6 * U * momentum * (1.0 / rstd.astype(np.float64) ** 2) * n / max(n - 1, 1) + 4 * U * (np.abs(rv0) + np.abs(rv))


# ---------------------------------------------------------------- the localiser
def localise(got, want, l, run=None):
    """None when got == want bit for bit; else a message naming the first differing element of the [m][n] output of launch `l` as
    the kernel sees it: tile, wave and its 32 x 32 (16 x 16) block, the K-run (`run`: the partial product compared, None: the
    finished sum) and whether the element lies in a ragged row panel or column tile."""
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    gb, wb = pp._bits(got), pp._bits(want)
    mask = gb != wb
    if not mask.any():
        return None
    r, c = (int(v) for v in np.argwhere(mask)[0])
    msg = [f"{int(mask.sum())} of {mask.size} elements differ, in {int(mask.any(axis=1).sum())} rows and {int(mask.any(axis=0).sum())} "
           f"columns; first at [{r}][{c}]: got {got[r, c]!r} (0x{int(gb[r, c]):08x}), want {want[r, c]!r} (0x{int(wb[r, c]):08x})",
           f"launch: {form_of(l)} ({l['label']}), [{l['m']}][{l['n']}] over k = {l['k']}"]
    if l["family"] == "reducer":
        q = (r * l["n"] + c) // 4
        msg.append(f"float4 {q} of {l['total4']}: thread {q % 256} of reducer workgroup {q // 256}, the sum of {l['runs']} K-runs")
        return "\n  ".join(msg)
    bm, bn = l["tile_rows"], l["tile_cols"]
    tr, tc = r % bm, c % bn
    if l["family"] == "32x64":
        wm, wn = tr // 16, tc // 32
        block = f"wave {wm * 2 + wn} (wm {wm}, wn {wn}), 16 x 16 block {tc % 32 // 16}"
    else:
        waves_m, waves_n, tm, tn = TILES[f"{bm}x{bn}"]
        wm, wn = tr // (tm * 32), tc // (tn * 32)
        block = f"wave {wm * waves_n + wn} (wm {wm}, wn {wn}), 32 x 32 block (i {tr % (tm * 32) // 32}, j {tc % (tn * 32) // 32})"
    msg.append(f"tile (row panel {r // bm}, column tile {c // bn}) of {bm} x {bn}, {block}")
    per = l["k_tiles_per_run"]
    if run is None:
        msg.append(f"the finished output: {l['runs']} K-run(s) of {run_lengths(l)} K-tiles, the last K-tile with {l['last_k_valid']} valid k")
    else:
        msg.append(f"K-run {run} of {l['runs']}: K-tiles {run * per}..{run * per + run_lengths(l)[run]}")
    ragged = [w for w, on in (("row panel", r // bm == -(-l["m"] // bm) - 1 and l["last_panel_rows"] < bm),
                              ("column tile", c // bn == -(-l["n"] // bn) - 1 and l["last_tile_cols"] < bn)) if on]
    msg.append("in a ragged " + " and a ragged ".join(ragged) if ragged else "not in a ragged panel")
    whole, count = pp._whole_blocks(mask, bm, bn)
    msg.append(f"the differing elements fill {'whole' if whole else 'parts of'} {count} tile(s)")
    return "\n  ".join(msg)
