"""CPU: every row of tests/gemm_pp_cases.py reaches the kernel and the paths it claims -- asked of the library's own launch
plan (lcrec_debug_linear_forward_plan: the functions lcrec_linear_forward dispatches with, nothing launched) for 256 CUs --
and the mismatch localiser names a corrupted piece, row and tile.  A change of pp_fits / pp_head_rows / the persistent
form's conditions shows here which rows it moved."""
import numpy as np
import pytest

import gemm_pp_cases as pp

CUS = 256


@pytest.mark.parametrize("case", pp.CASES, ids=pp.case_id)
def test_row_reaches_what_it_claims(case):
    launches = pp.plan(case.n, case.k, case.out, CUS)
    bad = pp.check_claims(case, launches)
    assert not bad, f"{pp.case_id(case)} on {CUS} CUs:\n  " + "\n  ".join(bad) + f"\n  plan: {launches}"
    # the numbers the plan reports, against the shape itself
    head = launches[0]
    assert head["k_tiles"] == case.k // 32 and head["tiles"] == -(-head["rows"] // 256) * -(-case.out // 128)
    assert head["last_panel_rows"] == (head["rows"] - 1) % 256 + 1
    if head["form"] == pp.PERSISTENT:
        assert case.k % 64 == 0 and case.k >= 384 and case.out % 128 == 0
        assert head["workgroups"] == min(CUS, head["virtual_tiles"])
        assert head["steady_iterations"] == (head["k_tiles"] - 12) // 2          # HEAD is K-tiles 0..9, TAIL the last two
        assert head["list_max"] <= -(-head["virtual_tiles"] // head["workgroups"])
    else:
        assert head["workgroups"] == head["virtual_tiles"]                       # one workgroup per (virtual) tile


def test_every_path_is_claimed_by_a_row():
    claimed = {name for case in pp.CASES for name in case.covers}
    assert not (claimed - set(pp.PROPERTIES)), claimed - set(pp.PROPERTIES)
    missing = pp.REQUIRED - claimed
    assert not missing, f"no row of gemm_pp_cases.CASES claims {sorted(missing)}: the path has lost its only test"
    for case in pp.CASES:
        assert case.covers, f"{pp.case_id(case)} claims no path"
        for key in ("form", "head", "tail", "k_tiles", "last_panel"):
            assert key in case.expect, (pp.case_id(case), key)
        if case.expect["form"] == pp.PERSISTENT:
            for key in ("steady", "lists", "empty"):
                assert key in case.expect, (pp.case_id(case), key)
    assert len({pp.case_id(c) for c in pp.CASES}) == len(pp.CASES)


@pytest.mark.parametrize("case", pp.CASES, ids=pp.case_id)
def test_row_inputs(case):
    """The inputs the GPU test feeds a row: shapes, dtype, switches honoured, per-column vectors distinct per column, and the
    same on every call."""
    x, W, b, sc, sh = pp.inputs(case)
    assert x.shape == (case.n, case.k) and W.shape == (case.out, case.k) and x.dtype == W.dtype == np.float32
    assert (b is not None) == case.bias and (sc is not None) == case.bn == (sh is not None)
    rs = np.random.RandomState(0)
    for v in pp.epilogue_vectors(case, rs):
        assert v.dtype == np.float32 and v.shape == (case.out,) and len(np.unique(v)) == case.out and np.isfinite(v).all()
    again = pp.inputs(case)
    assert all((p is None and q is None) or np.array_equal(p, q) for p, q in zip((x, W, b, sc, sh), again))


def test_plan_follows_the_cu_count():
    """The persistent form's grid is the CU count rounded down to a multiple of 8 (at least 8) and never above the virtual
    tiles; rows and labels do not depend on it.  The per-tile form and the other kernels ignore it."""
    for cus, want in ((256, 256), (304, 304), (250, 248), (8, 8), (5, 8), (2000, 1024)):
        head, tail = pp.plan(8200, 384, 4096, cus)
        assert (head["rows"], head["form"], head["workgroups"], tail["rows"], tail["label"]) == \
               (8192, pp.PERSISTENT, want, 8, "linear_fwd_32x64"), (cus, head, tail)
        assert head["list_min"] == 1024 // want and head["list_max"] == -(-1024 // want)
    assert pp.plan(0, 384, 4096, 256) == []
    assert [l["label"] for l in pp.plan(1000, 768, 2048, 256)] == ["linear_fwd_64x64"]      # below one round: generic
    assert [l["label"] for l in pp.plan(8192, 72, 1024, 256)] == ["linear_fwd_128x128"]
    with pytest.raises(RuntimeError):
        pp.plan(128, 12, 64, 256)                                           # in_dim % 8 != 0: linear_forward refuses it


# ---- the localiser
def _fake(n, out, seed=0):
    return np.random.RandomState(seed).standard_normal((n, out)).astype(np.float32)


def test_localiser_names_piece_row_and_tile():
    n, k, out = 776, 384, 8192                  # 4 panels x 64 column tiles on 256 workgroups: lists of two, ragged panel 3
    launches = pp.plan(n, k, out, CUS)
    want = _fake(n, out)
    assert pp.localise(want.copy(), want, launches) is None

    # one 16 x 32 piece: panel 1, column tile 5, group 1, wave sub-tile wm 1 / wn 0, (i 1, j 1), lower half -> piece 7
    got = want.copy()
    r0, c0 = 256 + 128 + 64 + 32 + 16, 5 * 128 + 32
    got[r0:r0 + 16, c0:c0 + 32] += 1.0
    msg = pp.localise(got, want, launches)
    assert "512 of" in msg and f"first at [{r0}][{c0}]" in msg
    assert "tile (panel 1, column tile 5) = tile 1 of 2 in workgroup 41's list" in msg       # t = 5 * 8 + 1
    assert "group 1, wave 6 (wm 1, wn 0), sub-tile (i 1, j 1), 16-row piece 7" in msg
    assert "handed over: sent in the staging phase of K-tile 9 of the next tile" in msg      # group 1: K-tile 2 + piece
    assert "whole 1 16 x 32 pieces" in msg and "parts of 16 tile rows" in msg and "parts of 1 256 x 128 tiles" in msg

    # one row of a tile, in a list's last tile (column tile 37 = the second of workgroup 43's two), of the ragged panel
    got = want.copy()
    got[768 + 3, 37 * 128:38 * 128] = 0.0
    msg = pp.localise(got, want, launches)
    assert "128 of" in msg and "in 1 rows and 128 columns" in msg
    assert "tile (panel 3, column tile 37) = tile 2 of 2 in workgroup 43's list" in msg      # t = 37 * 8 + 3 = 299 = 43 + 256
    assert "group 0, wave 0 (wm 0, wn 0), sub-tile (i 0, j 0), 16-row piece 0" in msg and "stored by finish()" in msg
    assert "whole 1 tile rows" in msg and "parts of 4 16 x 32 pieces" in msg

    # one whole tile of the ragged panel (8 valid rows): every piece, row and tile it touches is filled
    got = want.copy()
    got[768:, 128:256] = np.float32("nan")
    msg = pp.localise(got, want, launches)
    assert f"{8 * 128} of" in msg and "tile (panel 3, column tile 1) = tile 1 of 2 in workgroup 11's list" in msg
    assert "whole 4 16 x 32 pieces" in msg and "whole 8 tile rows" in msg and "whole 1 256 x 128 tiles" in msg
    assert "handed over: sent in the staging phase of K-tile 1 of the next tile" in msg      # group 0, piece 0


def test_localiser_per_tile_form_and_tail():
    launches = pp.plan(8200, 384, 4096, CUS)
    want = _fake(8200, 4096, 1)
    got = want.copy()
    got[8195, 70] = 1.0                                              # in the 8-row tail on the 32 x 64 tiles
    msg = pp.localise(got, want, launches)
    assert "rows 8192..8200 on linear_fwd_32x64" in msg and "tile (0, 1) of 32 x 64" in msg
    launches = pp.plan(4096, 64, 1930, CUS)
    want = _fake(4096, 1930, 2)
    got = want.copy()
    got[4095, 1929] = -want[4095, 1929]                              # the last element: last panel, the 10-column tile
    msg = pp.localise(got, want, launches)
    assert "1 of" in msg and "per-tile form, linear_fwd_pp2_kernel" in msg and "tile (panel 15, column tile 15)" in msg
    assert "group 1, wave 6 (wm 1, wn 0), sub-tile (i 1, j 0), 16-row piece 5" in msg and "epilogue after the K loop" in msg
    assert pp.localise(want[:10], want, launches).startswith("shape")
