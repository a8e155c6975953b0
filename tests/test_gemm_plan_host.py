"""CPU: the launch plans of lcrec_linear_forward / _backward / _backward_weights / _bn_forward (the pure functions the launchers of
csrc/gemm_f32.hip launch by; nothing is launched) against tests/gemm_cases.py -- every row reaches what it claims on 256 CUs,
REQUIRED is fully claimed -- against the dispatch rules restated here, and over a grid of shapes: which (instantiation, S > 1)
combinations default knobs reach, each claimed by a row, the rest exactly the named unreachable set.  The statistics bound of the
training forward is checked against a float32 restatement of the kernel's algorithm, and the localiser against planted errors."""
import threading

import numpy as np
import pytest

import gemm_cases as gc


@pytest.fixture(scope="module")
def ops():
    import lcrec_amd
    lcrec_amd._lib.load()
    return lcrec_amd.ops


@pytest.mark.parametrize("row", gc.ROWS, ids=gc.row_id)
def test_row_reaches_what_it_claims(ops, row):
    launches = gc.launches_of(row, ops)
    bad = gc.check_claims(row, launches)
    assert not bad, f"{gc.row_id(row)} on {gc.CUS} CUs:\n  " + "\n  ".join(bad) + f"\n  plan: {launches}"
    assert row.covers and set(row.expect) == {"form", "k_tiles", "runs"}
    for l in launches:                                   # the numbers the plan reports, against the shape itself
        if l["family"] == "reducer":
            assert l["total4"] == l["m"] * l["n"] // 4 and l["workgroups"] == -(-l["total4"] // 256)
            continue
        assert l["k_tiles"] == -(-l["k"] // 32) and sum(gc.run_lengths(l)) == l["k_tiles"] and min(gc.run_lengths(l)) >= 1
        assert l["last_k_valid"] == (l["k"] - 1) % 32 + 1
        bm_blocks, bn_blocks = -(-l["m"] // l["tile_rows"]), -(-l["n"] // l["tile_cols"])
        assert l["tiles"] == bm_blocks * bn_blocks
        assert l["last_panel_rows"] == (l["m"] - 1) % l["tile_rows"] + 1 and l["last_tile_cols"] == (l["n"] - 1) % l["tile_cols"] + 1
        if l["family"] == "tile_body":
            assert l["virtual_tiles"] == -(-bm_blocks // 8) * 8 * bn_blocks
            assert l["register_buffered"] == int(bool(l["fast"]) and f"{l['tile_rows']}x{l['tile_cols']}" in gc.RB_TILES)
        if l["family"] != "pp" and not l["grouped"]:
            assert l["workgroups"] == l["virtual_tiles"] * l["runs"]


def test_every_path_is_claimed_by_a_row():
    claimed = {name for row in gc.ROWS for name in row.covers}
    assert not (claimed - set(gc.PROPERTIES)), claimed - set(gc.PROPERTIES)
    missing = gc.REQUIRED - claimed
    assert not missing, f"no row of gemm_cases.ROWS claims {sorted(missing)}"
    assert len({gc.row_id(r) for r in gc.ROWS}) == len(gc.ROWS)
    assert set(gc.PROPERTIES) - gc.REQUIRED == {p for p in gc.PROPERTIES if p.endswith("128x128_row_fast")}


# ---------------------------------------------------------------- the rule, restated
def _cdiv(a, b):
    return -(-a // b)


def _tile(M, N):
    if N > 64:
        if _cdiv(M, 128) * _cdiv(N, 128) >= 512:
            return "128x128"
        return "64x128" if _cdiv(M, 64) * _cdiv(N, 128) >= 256 else "64x64"
    if N > 32:
        return "64x64" if _cdiv(M, 128) < 256 else "128x64"
    return "128x32"


def _s16(M, N, K):
    return K % 32 == 0 and K >= 32 and N % 4 == 0 and _cdiv(M, 64) * _cdiv(N, 64) <= 128


def _splits(n, in_dim, out_dim):
    shape = _tile(out_dim, in_dim)
    bm, bn = (128, 32) if shape == "64x128" else tuple(int(v) for v in shape.split("x"))
    nk = _cdiv(n, 32)
    s = min(512 // (_cdiv(out_dim, bm) * _cdiv(in_dim, bn)), nk // 4, 16)
    return 1 if s < 2 else _cdiv(nk, _cdiv(nk, s))


def _pp_fits(n, out):
    tiles = _cdiv(n, 256) * _cdiv(out, 128)
    rounds = _cdiv(tiles, 256)
    return tiles >= 256 and (rounds >= 8 or tiles * 5 >= rounds * 256 * 4)


def _pp_head(n, out):
    ntile = _cdiv(out, 128)
    tiles = _cdiv(n, 256) * ntile
    rounds, last = _cdiv(tiles, 256), tiles % 256
    if rounds >= 8 or last == 0 or last * 10 >= 256 * 9:
        return 0
    p = n // 256
    while p >= 1 and p * ntile >= 256 and p >= n // 256 - 256 // ntile:
        l = p * ntile % 256
        if l == 0 or l * 10 >= 256 * 9:
            return p * 256 if p * 256 < n else 0
        p -= 1
    return 0


def _forward_forms(n, k, out):
    """the forms lcrec_linear_forward runs [n][k] -> [n][out] on, in launch order"""
    forms = []
    pp_ok = out > 64 and k % 32 == 0
    while n > 0:
        head = _pp_head(n, out) if pp_ok and len(forms) + 1 < 4 else 0
        if head:
            forms.append("pp")
            n -= head
            continue
        if pp_ok and _pp_fits(n, out):
            forms.append("pp")
        elif _s16(n, out, k):
            forms.append("s16_row")
        else:
            forms.append(f"{_tile(n, out)}_row_{'fast' if k % 32 == 0 else 'guarded'}")
        break
    return forms


def _backward_forms(n, i, o):
    dx = "s16_dx" if _s16(n, i, o) else f"{_tile(n, i)}_dx_fast"
    s = _splits(n, i, o)
    return [dx, f"{_tile(o, i)}_dw_fast"] + (["reduce"] if s > 1 else []), s


def _train_form(n, k, out, pro, stats):
    tile = ("64x128" if _cdiv(n, 64) * _cdiv(out, 128) >= 256 else "64x64") if out > 64 else "64x64" if out > 32 else "128x32"
    return f"train_{tile}_" + "_".join(w for w, on in (("pro", pro), ("stats", stats)) if on)


NS = (1, 2, 31, 33, 64, 70, 256, 1000, 1024, 2048, 4096, 8192, 8200, 16859, 32640, 32641, 65408, 65409, 131072)
WIDTHS = (4, 32, 36, 64, 68, 128, 132, 1024, 2048, 4096)
KS = (8, 32, 40, 64, 384)


def test_plans_follow_the_restated_rule_and_reach_exactly_the_named_forms(ops):
    """The four plans over a grid against the rule above, and the reachability sweep: every (form, S > 1) the grid reaches is
    claimed by a row of the table, and what it does not reach is exactly gemm_cases.UNREACHABLE -- a change of the rule that
    makes one of those reachable, or strands a form, fails here."""
    reached = set()
    for n in NS:
        for out in WIDTHS + (30, 62, 16384, 32768):
            for k in KS:
                if n * out > 2 ** 29 or n * k > 2 ** 27:
                    continue
                got = [gc.form_of(l) for l in gc._forward_launches(n, k, out, gc.CUS)]
                assert got == _forward_forms(n, k, out), (n, k, out, got)
                reached |= {(f, False) for f in got}
    for n in NS:
        for i in WIDTHS:
            for o in WIDTHS + (32768,):
                if o % 32 or (n + 64) * max(i, o) * 4 >= 2 ** 31 or o * i * 4 >= 2 ** 31:
                    continue
                ls = [dict(l, grouped=False) for l in ops.linear_backward_plan(n, i, o)]
                want, s = _backward_forms(n, i, o)
                assert [gc.form_of(l) for l in ls] == want and ls[1]["runs"] == s == ops.linear_backward_splits(n, i, o), (n, i, o, ls)
                reached |= {(gc.form_of(ls[0]), False), (gc.form_of(ls[1]), s > 1)}
    for n in (2, 70, 1024, 2048, 8200, 16859):
        for out in WIDTHS:
            if not ops.linear_bn_supported(n, 64, out):
                continue
            for pro, stats in ((1, 1), (0, 1), (1, 0)):
                l = dict(ops.linear_bn_forward_plan(n, 64, out, pro, stats), grouped=False)
                assert gc.form_of(l) == _train_form(n, 64, out, pro, stats), (n, out, l)
                assert l["chunk_row_tiles"] == (((l["tile_rows"] + l["tile_cols"]) * 36) // (3 * l["tile_cols"]) if stats else 0)
                reached.add((gc.form_of(l), False))
    for folded in (False, True):
        for splits in (0, 1, 3):
            products, reducers, grids = ops.linear_backward_weights_plan([(n, 64, 64, folded, splits) for n in (1, 33, 300, 2048)])
            for (n, l) in zip((1, 33, 300, 2048), products):
                nk = _cdiv(n, 32)
                want = _splits(n, 64, 64) if splits == 0 else _cdiv(nk, _cdiv(nk, min(splits, nk)))
                assert l["runs"] == want and (l["tile_rows"], l["tile_cols"], l["pro"]) == (64, 64, 2 * folded), (n, splits, l)
                reached.add((gc.form_of(dict(l, grouped=True)), want > 1))
            assert grids[0] == sum(l["workgroups"] for l in products) and grids[1] == sum(l["workgroups"] for l in reducers)
            assert [l["wg_start"] for l in products] == list(np.cumsum([0] + [l["workgroups"] for l in products[:-1]]))
    reached = {(f, s) for f, s in reached if f not in ("pp", "reduce")}
    universe = {(f, False) for f in gc.FORMS} | {(f, True) for f in gc.SPLIT_FORMS}
    assert reached <= universe, reached - universe
    assert universe - reached == gc.UNREACHABLE, (sorted(universe - reached), sorted(gc.UNREACHABLE))
    # every reachable combination is some row's
    rows = set()
    for row in gc.ROWS:
        for l in gc.launches_of(row, ops):
            rows.add((gc.form_of(l), l["family"] == "tile_body" and l["runs"] > 1))
    assert reached <= rows, sorted(reached - rows)


def test_the_forms_the_issue_names(ops):
    """Literal spot checks, so that the restated rule and the library cannot drift together."""
    f = lambda n, k, out: [gc.form_of(l) for l in gc._forward_launches(n, k, out, 256)]
    assert f(200, 64, 30) == ["128x32_row_fast"] and f(8200, 32, 32) == ["128x32_row_fast"] and f(1024, 64, 640) == ["64x64_row_fast"]
    assert f(2048, 64, 1024) == ["64x128_row_fast"] and f(32641, 32, 64) == ["128x64_row_fast"] and f(32640, 32, 64) == ["64x64_row_fast"]
    assert f(8192, 72, 1024) == ["128x128_row_guarded"] and f(65409, 8, 128) == ["128x128_row_guarded"] and f(65408, 8, 128) == ["64x128_row_guarded"]
    assert f(8192, 64, 1024) == ["pp"] and f(70, 64, 68) == ["s16_row"]
    b = lambda n, i, o: [gc.form_of(dict(l, grouped=False)) for l in ops.linear_backward_plan(n, i, o)]
    assert b(8192, 1024, 32) == ["128x128_dx_fast", "128x32_dw_fast"] or b(8192, 1024, 32)[0] == "128x128_dx_fast"
    assert b(33, 2048, 4096)[1] == "128x128_dw_fast" and b(1024, 64, 32)[0] == "s16_dx"
    t = ops.linear_bn_forward_plan
    assert (t(1601, 32, 36, 1, 1)["chunk_row_tiles"], t(1601, 32, 36, 1, 1)["chunks"]) == (24, 2)
    assert (t(2048, 32, 1028, 1, 1)["chunk_row_tiles"], t(2048, 32, 1028, 1, 1)["chunks"]) == (18, 2)
    assert (t(7809, 32, 4, 1, 1)["chunk_row_tiles"], t(7809, 32, 4, 1, 1)["chunks"]) == (60, 2)
    assert t(100, 32, 32, 0, 0) is None


def test_plans_refuse_what_the_entry_points_refuse(ops):
    """(In a thread of its own: the library's last-error text is per thread, and other tests expect this thread's to be empty.)"""
    seen = []

    def calls():
        for bad in (lambda: ops.linear_backward_plan(64, 30, 32), lambda: ops.linear_backward_plan(64, 32, 48),
                    lambda: ops.linear_backward_plan(-1, 32, 32), lambda: ops.linear_backward_plan(2 ** 22, 4096, 32),
                    lambda: ops.linear_bn_forward_plan(64, 40, 32, 1, 1), lambda: ops.linear_bn_forward_plan(1, 32, 32, 0, 1),
                    lambda: ops.linear_bn_forward_plan(2 ** 17, 32, 1024, 1, 1), lambda: ops.linear_bn_forward_plan(0, 32, 32, 1, 1),
                    lambda: ops.linear_backward_weights_plan([(64, 30, 32, False, 0)]),
                    lambda: ops.linear_backward_weights_plan([(0, 32, 32, False, 0)]),
                    lambda: ops.linear_backward_weights_plan([(64, 32, 32, False, 0)] * 17)):
            try:
                bad()
                seen.append(None)
            except Exception as exc:              # noqa: BLE001
                seen.append(str(exc))
        seen.append(ops.linear_backward_plan(64, 32, 48, need_gx=False))    # out_dim % 32 matters to dX only

    worker = threading.Thread(target=calls)
    worker.start()
    worker.join()
    assert all(isinstance(s, str) for s in seen[:-1]), seen
    assert "multiple of 32" in seen[1] and "17 problems" in seen[10] and "more than 1 row" in seen[5]
    assert [l["role"] for l in seen[-1]] == ["dw"]


# ---------------------------------------------------------------- the statistics bound
@pytest.mark.parametrize("row", [r for r in gc.ROWS if r.kind == "train" and r.opt["stats"]], ids=gc.row_id)
def test_statistics_bound_holds_for_a_float32_restatement(oracle, ops, row):
    """The bound of gemm_cases.stats_reference, on every statistics row: the kernel's algorithm in float32 numpy stays inside
    it, the adversarial columns are what they claim, and the bound is never looser than the tolerances used before."""
    x, sc, sh, W, b, *_ = gc.train_inputs(row)
    u = oracle.affine_relu(x, sc, sh, relu=row.opt["in_relu"]) if row.opt["pro"] else x
    t = oracle.linear(u, W, b, threads=8)
    bm = ops.linear_bn_forward_plan(*row.dims, row.opt["pro"], True)["tile_rows"]
    ref = gc.stats_reference(t, bm)
    mean, rstd, _ = gc.stats_model(t, bm)
    assert (np.abs(mean - ref["mean"]) <= ref["mean_tol"]).all(), np.abs(mean - ref["mean"]) / ref["mean_tol"]
    assert ((rstd >= ref["rstd_lo"]) & (rstd <= ref["rstd_hi"])).all()
    ok = ref["benign"]
    assert (ref["mean_tol"] <= 1e-5 * np.abs(ref["mean"]) + 1e-6)[ok].all()
    assert (ref["rstd_hi"] <= ref["rstd"] * (1 + 1e-5) * (1 + 1e-12))[ok].all() and (ref["rstd_lo"] >= ref["rstd"] * (1 - 1e-5) * (1 - 1e-12))[ok].all()
    print(f"{gc.row_id(row)}: adversarial columns: |mean error| / bound {np.abs(mean - ref['mean'])[:4] / np.maximum(ref['mean_tol'][:4], 1e-300)}, "
          f"rstd interval {ref['rstd_lo'][:4]} .. {ref['rstd_hi'][:4]}, float32 model {rstd[:4]}")
    n, out = t.shape
    assert abs(ref["mean"][0] - 1e3) < 1e-2 and (n < 8 or 1e-3 < np.sqrt(ref["var"][0]) < 1e-1)
    if out > 1:
        assert (t[:, 1] == gc.CONST_SHORT).all() and mean[1] == gc.CONST_SHORT and rstd[1] == np.float32(1) / np.sqrt(np.float32(gc.TRAIN_EPS))
    if out > 3:
        assert (t[:, 3] == gc.CONST_FULL).all() and rstd[3] == np.float32(1) / np.sqrt(np.float32(gc.TRAIN_EPS))
    if out > 2 and n >= 8:
        assert np.abs(t[0, 2] - ref["mean"][2]) > 6 * np.sqrt(ref["var"][2] - (t[0, 2] - ref["mean"][2]) ** 2 / n)
    # a sum of squares without the pivot loses column 0 altogether: E[t^2] - mean^2 in float32 is off by more than the bound
    t32 = t[:, 0]
    naive = np.float32(np.sum(t32 * t32, dtype=np.float32) / np.float32(n)) - np.float32(np.mean(t32, dtype=np.float32)) ** 2
    if n >= 64:
        bad = np.float32(1) / np.sqrt(max(naive, 0) + np.float32(gc.TRAIN_EPS))
        assert not (ref["rstd_lo"][0] <= bad <= ref["rstd_hi"][0])


# ---------------------------------------------------------------- the localiser
def test_localiser_names_tile_wave_run_and_ragged_panel(ops):
    l = dict(ops.linear_backward_plan(257, 64, 64, need_gx=False)[0], grouped=False)
    want = np.random.RandomState(0).standard_normal((64, 64)).astype(np.float32)
    assert gc.localise(want.copy(), want, l) is None
    got = want.copy()
    got[40, 33] += 1
    msg = gc.localise(got, want, l, run=1)
    assert "first at [40][33]" in msg and "tile (row panel 0, column tile 0) of 64 x 64, wave 3 (wm 1, wn 1), 32 x 32 block (i 0, j 0)" in msg
    assert "K-run 1 of 2: K-tiles 5..9" in msg and "not in a ragged panel" in msg
    l = dict(ops.linear_backward_plan(2048, 68, 36, need_gx=False)[0], grouped=False)
    want = np.zeros((36, 68), np.float32)
    got = want.copy()
    got[35, 67] = 1
    msg = gc.localise(got, want, l)
    assert "column tile 1" in msg and "in a ragged row panel and a ragged column tile" in msg and "16 K-run(s)" in msg
    red = dict(ops.linear_backward_plan(2048, 68, 36, need_gx=False)[1], grouped=False)
    assert "float4 611 of 612: thread 99 of reducer workgroup 2" in gc.localise(got, want, red)
    assert gc.localise(want[:3], want, l).startswith("shape")
