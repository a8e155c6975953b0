"""The case table of the two ping-pong GEMM kernels (linear_fwd_pp3_kernel / linear_fwd_pp2_kernel of csrc/gemm_f32.hip),
shared by tests/test_gemm_pp_plan_host.py (CPU: every row reaches the paths it claims) and tests/test_gpu_gemm_pp.py (GPU:
every row bit for bit against the oracle), with the library's launch plan (ops.linear_forward_plan) and the mismatch localiser.

A row is a shape, its epilogue switches, the launches the dispatch rule must make of it on 256 CUs (`expect`) and the kernel
paths it exists for (`covers`, names of PROPERTIES).  Each property is a predicate over the row and its planned launch, so a
row cannot claim a path its shape does not reach, and REQUIRED lists the paths some row must keep claiming."""
from collections import namedtuple

import numpy as np

PP_LABEL = "linear_fwd_pp_256x128"
PER_TILE, PERSISTENT = 2, 3          # `form` of a ping-pong launch: linear_fwd_pp2_kernel / linear_fwd_pp3_kernel
TILE_M, TILE_N, GROUP_M = 256, 128, 128


def plan(n, k, out, cus):
    """The launches lcrec_linear_forward makes for [n][k] -> [n][out] on `cus` compute units: the dicts of
    lcrec_amd.ops.linear_forward_plan (the fields of lcrec_gemm_launch) plus `rows`, the table's name for `m`.  Host code of
    the library: no GPU is needed."""
    from lcrec_amd import ops
    return [dict(l, rows=l["m"]) for l in ops.linear_forward_plan(n, k, out, cus)]


def plan_labels(launches, repeat=1):
    """{trace label: launch count} of a plan run `repeat` times"""
    labels = {}
    for launch in launches:
        labels[launch["label"]] = labels.get(launch["label"], 0) + repeat
    return labels


Case = namedtuple("Case", "n k out relu bn bias expect covers")


def _case(n, k, out, relu, bn, bias, covers, **expect):
    return Case(n, k, out, relu, bn, bias, expect, tuple(covers))


def case_id(c):
    return f"{c.n}-{c.k}-{c.out}-{'relu' if c.relu else 'lin'}-{'bn' if c.bn else 'nobn'}-{'bias' if c.bias else 'nobias'}"


# ---- the path properties: name -> predicate(case, head launch of its plan).  The head is the row's ping-pong launch.
def _last_col_tile(c):
    return (c.out - 1) % TILE_N + 1


PROPERTIES = {
    # linear_fwd_pp3_kernel
    "pp3_has_bn": lambda c, h: h["form"] == PERSISTENT and c.bn,                        # the <true> instantiation
    "pp3_no_bn": lambda c, h: h["form"] == PERSISTENT and not c.bn,
    "pp3_no_relu": lambda c, h: h["form"] == PERSISTENT and not c.relu,
    "pp3_no_bias": lambda c, h: h["form"] == PERSISTENT and not c.bias,
    "pp3_steady_empty": lambda c, h: h["form"] == PERSISTENT and h["steady_iterations"] == 0,
    "pp3_steady_once": lambda c, h: h["form"] == PERSISTENT and h["steady_iterations"] == 1,
    "pp3_steady_long": lambda c, h: h["form"] == PERSISTENT and h["steady_iterations"] >= 4,
    # a workgroup's only tile: has_next == 0 from the start, finish() with have_prev == 0
    "pp3_only_tile": lambda c, h: h["form"] == PERSISTENT and h["single_tile_workgroups"] > 0,
    "pp3_every_list_one_tile": lambda c, h: h["form"] == PERSISTENT and h["list_min"] == 1 == h["list_max"],
    "pp3_hand_over": lambda c, h: h["form"] == PERSISTENT and h["list_max"] >= 2,      # epi_math into prev, 8 pieces sent
    "pp3_unequal_lists": lambda c, h: h["form"] == PERSISTENT and h["list_min"] != h["list_max"],
    "pp3_empty_workgroups": lambda c, h: h["form"] == PERSISTENT and h["empty_workgroups"] > 0,   # the early return
    "pp3_xcd_holes": lambda c, h: h["form"] == PERSISTENT and h["virtual_tiles"] > h["tiles"],
    # ragged last row panel: as a list's last tile (finish(), cur_ar) / handed over (prv_ar in epi_send)
    # (a ragged-panel tile is some list's last tile unless every one of them is handed over)
    "pp3_ragged_current": lambda c, h: (h["form"] == PERSISTENT and h["last_panel_rows"] < TILE_M
                                        and h["ragged_handed_over"] < -(-c.out // TILE_N)),
    "pp3_ragged_previous": lambda c, h: h["form"] == PERSISTENT and h["ragged_handed_over"] > 0,
    "pp3_group1_empty": lambda c, h: h["form"] == PERSISTENT and h["last_panel_rows"] <= GROUP_M,
    "pp3_group1_partial": lambda c, h: h["form"] == PERSISTENT and GROUP_M < h["last_panel_rows"] < TILE_M,
    # linear_fwd_pp2_kernel
    "pp2_odd_k_tiles": lambda c, h: h["form"] == PER_TILE and h["k_tiles"] > 1 and h["k_tiles"] % 2 == 1,
    "pp2_one_k_tile": lambda c, h: h["form"] == PER_TILE and h["k_tiles"] == 1,
    "pp2_scalar_stores": lambda c, h: h["form"] == PER_TILE and c.out % 4 != 0,
    "pp2_last_column_tile_le_64": lambda c, h: h["form"] == PER_TILE and _last_col_tile(c) <= 64,   # group 1: no weight rows
    "pp2_long_k_ragged_n": lambda c, h: h["form"] == PER_TILE and c.k >= 384 and c.out % TILE_N != 0,
    "pp2_long_k_odd_k_tiles": lambda c, h: h["form"] == PER_TILE and c.k >= 384 and c.k % 64 != 0 and c.out % TILE_N == 0,
    "pp2_no_bias": lambda c, h: h["form"] == PER_TILE and not c.bias,
    "pp2_has_bn": lambda c, h: h["form"] == PER_TILE and c.bn,
    "pp2_ragged_rows": lambda c, h: h["form"] == PER_TILE and h["last_panel_rows"] < TILE_M,
    # the composition of a cut launch
    "head_and_tail": lambda c, h: h["rows"] < c.n,
}
REQUIRED = frozenset(PROPERTIES)     # every path above must be claimed by at least one row of CASES

# ---- the table.  expect: form, head / tail rows (tail_label: the tail's kernel), k_tiles, and for the persistent form
# steady (iterations per tile), lists (shortest, longest), empty (workgroups), last_panel (valid rows of the last row panel)
CASES = [
    # linear_fwd_pp3_kernel: K % 64 == 0, K >= 384, N % 128 == 0
    _case(2048, 384, 4096, True, True, True,
          ["pp3_has_bn", "pp3_steady_empty", "pp3_only_tile", "pp3_every_list_one_tile"],
          form=PERSISTENT, head=2048, tail=0, k_tiles=12, steady=0, lists=(1, 1), empty=0, last_panel=256),
    _case(4096, 448, 4096, True, True, False,
          ["pp3_has_bn", "pp3_steady_once", "pp3_hand_over", "pp3_no_bias"],
          form=PERSISTENT, head=4096, tail=0, k_tiles=14, steady=1, lists=(2, 2), empty=0, last_panel=256),
    _case(4096, 768, 2048, True, True, True,                   # the recipe's first layer at its smallest ping-pong batch
          ["pp3_has_bn", "pp3_steady_long", "pp3_only_tile"],
          form=PERSISTENT, head=4096, tail=0, k_tiles=24, steady=6, lists=(1, 1), empty=0, last_panel=256),
    _case(2048, 1024, 4096, False, False, True,
          ["pp3_no_bn", "pp3_no_relu", "pp3_steady_long"],
          form=PERSISTENT, head=2048, tail=0, k_tiles=32, steady=10, lists=(1, 1), empty=0, last_panel=256),
    _case(3336, 384, 3840, True, False, True,
          ["pp3_no_bn", "pp3_unequal_lists", "pp3_empty_workgroups", "pp3_ragged_current", "pp3_group1_empty", "pp3_xcd_holes",
           "pp3_hand_over", "pp3_only_tile"],
          form=PERSISTENT, head=3336, tail=0, k_tiles=12, steady=0, lists=(0, 2), empty=4, last_panel=8, handed_over=0),
    _case(776, 384, 8192, True, True, True,
          ["pp3_has_bn", "pp3_empty_workgroups", "pp3_ragged_previous", "pp3_ragged_current", "pp3_group1_empty", "pp3_hand_over"],
          form=PERSISTENT, head=776, tail=0, k_tiles=12, steady=0, lists=(0, 2), empty=128, last_panel=8, handed_over=32),
    _case(904, 384, 8192, False, True, True,
          ["pp3_has_bn", "pp3_no_relu", "pp3_ragged_previous", "pp3_group1_partial", "pp3_empty_workgroups"],
          form=PERSISTENT, head=904, tail=0, k_tiles=12, steady=0, lists=(0, 2), empty=128, last_panel=136, handed_over=32),
    _case(7688, 384, 2048, True, False, False,
          ["pp3_no_bn", "pp3_no_bias", "pp3_xcd_holes", "pp3_unequal_lists", "pp3_only_tile", "pp3_ragged_current"],
          form=PERSISTENT, head=7688, tail=0, k_tiles=12, steady=0, lists=(1, 2), empty=0, last_panel=8),
    # 33 row panels: the rule cuts 32 of them (four whole rounds) off for the persistent kernel and hands the 8-row tail on
    _case(8200, 384, 4096, False, False, True,
          ["head_and_tail", "pp3_no_bn", "pp3_no_relu", "pp3_hand_over"],
          form=PERSISTENT, head=8192, tail=8, tail_label="linear_fwd_32x64", k_tiles=12, steady=0, lists=(4, 4), empty=0,
          last_panel=256),
    # linear_fwd_pp2_kernel: every other launch of whole rounds with K % 32 == 0, N > 64
    _case(4096, 96, 2048, True, False, True, ["pp2_odd_k_tiles"],
          form=PER_TILE, head=4096, tail=0, k_tiles=3, last_panel=256),
    _case(4096, 160, 2048, True, True, True, ["pp2_odd_k_tiles", "pp2_has_bn"],
          form=PER_TILE, head=4096, tail=0, k_tiles=5, last_panel=256),
    _case(4096, 64, 2001, True, True, True, ["pp2_scalar_stores", "pp2_has_bn"],          # last column tile: 81 columns
          form=PER_TILE, head=4096, tail=0, k_tiles=2, last_panel=256),
    _case(4096, 64, 1930, True, False, True, ["pp2_last_column_tile_le_64", "pp2_scalar_stores"],   # last column tile: 10
          form=PER_TILE, head=4096, tail=0, k_tiles=2, last_panel=256),
    _case(4096, 384, 2000, True, False, True, ["pp2_long_k_ragged_n"],
          form=PER_TILE, head=4096, tail=0, k_tiles=12, last_panel=256),
    _case(4096, 416, 2048, False, True, True, ["pp2_long_k_odd_k_tiles", "pp2_odd_k_tiles", "pp2_has_bn"],
          form=PER_TILE, head=4096, tail=0, k_tiles=13, last_panel=256),
    _case(7688, 32, 2048, True, False, False, ["pp2_one_k_tile", "pp2_no_bias", "pp2_ragged_rows"],
          form=PER_TILE, head=7688, tail=0, k_tiles=1, last_panel=8),
]


def check_claims(case, launches):
    """What of `case`'s expect / covers does NOT hold for this plan: a list of messages (empty: the row tests what it says)."""
    e, bad = case.expect, []
    if not launches or launches[0]["label"] != PP_LABEL:
        return [f"the first launch is {launches[0]['label'] if launches else None}, not {PP_LABEL}"]
    h = launches[0]
    got = {"form": h["form"], "head": h["rows"], "tail": case.n - h["rows"], "k_tiles": h["k_tiles"],
           "last_panel": h["last_panel_rows"]}
    if h["form"] == PERSISTENT:
        got.update(steady=h["steady_iterations"], lists=(h["list_min"], h["list_max"]), empty=h["empty_workgroups"],
                   handed_over=h["ragged_handed_over"])
    if len(launches) > 1:
        got["tail_label"] = launches[1]["label"]
    for key, want in e.items():
        if got.get(key) != want:
            bad.append(f"{key}: the plan gives {got.get(key)}, the row says {want}")
    if h["row0"] != 0 or sum(l["rows"] for l in launches) != case.n or len(launches) != (2 if e["tail"] else 1):
        bad.append(f"launches {[(l['row0'], l['rows'], l['label']) for l in launches]} do not cover the row as it says")
    for name in case.covers:
        if not PROPERTIES[name](case, h):
            bad.append(f"property {name} does not hold")
    return bad


def _distinct(rs, draw, count):
    """`count` float32 draws, no two equal: a value that repeats an earlier one is drawn again (4096 draws from a narrow
    normal do collide in float32), so that a kernel reading the wrong column's constant cannot get the right one."""
    v = draw(count).astype(np.float32)
    while True:
        _, first = np.unique(v, return_index=True)
        if len(first) == count:
            return v
        again = np.setdiff1d(np.arange(count), first)
        v[again] = draw(len(again)).astype(np.float32)


def epilogue_vectors(case, rs):
    """(bias, bn_scale, bn_shift) of a row, each distinct per column, whether or not the row uses them"""
    b = _distinct(rs, lambda m: 0.1 * rs.standard_normal(m), case.out)
    sc = _distinct(rs, lambda m: 1 + 0.1 * rs.standard_normal(m), case.out)
    sh = _distinct(rs, lambda m: 0.1 * rs.standard_normal(m), case.out)
    return b, sc, sh


def inputs(case):
    """(x, W, bias | None, bn_scale | None, bn_shift | None), seeded per row; the per-column vectors are distinct per column."""
    rs = np.random.RandomState(case.n + case.k + case.out)
    x = rs.standard_normal((case.n, case.k)).astype(np.float32)
    W = (rs.standard_normal((case.out, case.k)) / np.sqrt(case.k)).astype(np.float32)
    b, sc, sh = epilogue_vectors(case, rs)
    return x, W, (b if case.bias else None), (sc if case.bn else None), (sh if case.bn else None)


# ---- the localiser: where a wrong result sits, in the kernel's own coordinates
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _whole_blocks(mask, bh, bw):
    """Do the set elements of `mask` fill every bh x bw block they touch (blocks clipped at the matrix edge)?"""
    n, m = mask.shape
    ph, pw = -(-n // bh) * bh, -(-m // bw) * bw
    pad = np.zeros((ph, pw), dtype=np.int64)
    pad[:n, :m] = mask
    valid = np.zeros((ph, pw), dtype=np.int64)
    valid[:n, :m] = 1
    per = pad.reshape(ph // bh, bh, pw // bw, bw).sum(axis=(1, 3))
    size = valid.reshape(ph // bh, bh, pw // bw, bw).sum(axis=(1, 3))
    touched = per > 0
    return bool(touched.any() and (per[touched] == size[touched]).all()), int(touched.sum())


def list_position(launch, panel, col_tile, bn_blocks):
    """(workgroup, position in its tile list, length of the list) of tile (panel, col_tile) of a persistent launch: the
    walk of linear_fwd_pp3_kernel -- tile numbers blockIdx.x, + gridDim.x, ... with the holes of the XCD-aware order skipped."""
    bm_blocks = -(-launch["rows"] // TILE_M)
    t = ((panel // 8) * bn_blocks + col_tile) * 8 + panel % 8
    wg = t % launch["workgroups"]
    pos = length = 0
    for u in range(wg, launch["virtual_tiles"], launch["workgroups"]):
        xcd, j = u & 7, u >> 3
        if j >= ((bm_blocks - xcd + 7) >> 3) * bn_blocks:
            continue
        pos += u < t
        length += 1
    return wg, pos, length


def localise(got, want, launches):
    """None when got == want bit for bit; else a message naming the first differing element (row-major) as the kernel
    sees it -- launch, tile, position in the workgroup's list (persistent form), group, wave, sub-tile, 16-row piece and the
    K-tile phase that sends it -- and how many elements differ and whether they fill whole pieces, tile rows or tiles."""
    if got.shape != want.shape:
        return f"shape {got.shape} != {want.shape}"
    mask = _bits(got) != _bits(want)
    if not mask.any():
        return None
    n, out = want.shape
    r, c = (int(v) for v in np.argwhere(mask)[0])
    launch = next(l for l in launches if l["row0"] <= r < l["row0"] + l["rows"])
    msg = [f"{int(mask.sum())} of {mask.size} elements differ, in {int(mask.any(axis=1).sum())} rows and "
           f"{int(mask.any(axis=0).sum())} columns; first at [{r}][{c}]: got {got[r, c]!r} (0x{int(_bits(got)[r, c]):08x}), "
           f"want {want[r, c]!r} (0x{int(_bits(want)[r, c]):08x})",
           f"launch: rows {launch['row0']}..{launch['row0'] + launch['rows']} on {launch['label']}"
           + {PERSISTENT: " (persistent form, linear_fwd_pp3_kernel)", PER_TILE: " (per-tile form, linear_fwd_pp2_kernel)"}
           .get(launch["form"], "")]
    lr = r - launch["row0"]
    if launch["label"] != PP_LABEL:
        msg.append(f"tile ({lr // launch['tile_rows']}, {c // launch['tile_cols']}) of {launch['tile_rows']} x {launch['tile_cols']}")
        return "\n  ".join(msg)
    bn_blocks = -(-out // TILE_N)
    panel, col_tile = lr // TILE_M, c // TILE_N
    tr, tc = lr % TILE_M, c % TILE_N
    group, wm, wn = tr // GROUP_M, tr % GROUP_M // 64, tc // 64
    i, j, hf = tr % 64 // 32, tc % 64 // 32, tr % 32 // 16
    piece = (2 * i + j) * 2 + hf
    where = f"tile (panel {panel}, column tile {col_tile})"
    if launch["form"] == PERSISTENT:
        wg, pos, length = list_position(launch, panel, col_tile, bn_blocks)
        where += f" = tile {pos + 1} of {length} in workgroup {wg}'s list"
        if pos + 1 == length:
            phase = "stored by finish() after the list's last K loop"
        else:   # piece p is patched in the compute phase of the next tile's K-tile 1 + p; group 0 sends it in the same K-tile's
            #     second phase, group 1 in the first phase of the K-tile after
            phase = (f"handed over: sent in the staging phase of K-tile {1 + piece + group} of the next tile "
                     f"(phase {2 * (1 + piece + group) + (1 - group)} of its K loop)")
    else:
        phase = "stored by the epilogue after the K loop"
    msg.append(where)
    msg.append(f"group {group}, wave {group * 4 + wm * 2 + wn} (wm {wm}, wn {wn}), sub-tile (i {i}, j {j}), 16-row piece {piece} "
               f"(rows {tr // 16 * 16}..{tr // 16 * 16 + 16} x columns {tc // 32 * 32}..{tc // 32 * 32 + 32} of the tile): {phase}")
    fills = []
    for name, bh, bw in (("16 x 32 pieces", 16, 32), ("tile rows (1 x 128)", 1, TILE_N), ("256 x 128 tiles", TILE_M, TILE_N)):
        whole, count = _whole_blocks(mask[launch["row0"]:launch["row0"] + launch["rows"]], bh, bw)
        fills.append(f"{'whole' if whole else 'parts of'} {count} {name}")
    msg.append("the differing elements of this launch fill " + ", ".join(fills))
    return "\n  ".join(msg)
