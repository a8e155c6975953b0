"""CPU: the launch plan of the step-tail calls (lcrec_debug_step_tail_plan: the function the launchers of csrc/train_ops.hip and
csrc/vq_train.hip launch by, nothing launched) against the rules restated in tests/step_tail_cases.py; every launch the plan can
report is some row's; every input builder keeps what its row promises; and the references of tests/step_tail_ref.py satisfy, on
their own, every bound the GPU test imposes."""
import math

import numpy as np
import pytest

import step_tail_cases as tc
import step_tail_ref as ref


@pytest.fixture(scope="module")
def ops():
    import lcrec_amd
    lcrec_amd._lib.load()
    return lcrec_amd.ops


PLANNED = tc.RECON + tc.NORM + tc.RELU + tc.QG + tc.APPLY


@pytest.mark.parametrize("row", PLANNED, ids=tc.row_id)
def test_row_gets_the_launch_it_is_listed_for(ops, row):
    call, n, width, aligned, K = tc.plan_args(row)
    assert ops.step_tail_plan(call, n, width, aligned, K) == tc.form_of(row), row.why
    assert row.why


@pytest.mark.parametrize("row", tc.STATS, ids=tc.row_id)
def test_code_stats_row_gets_the_launches_it_is_listed_for(ops, row):
    single, levels = tc.stats_forms(row)
    assert ops.step_tail_plan("code_stats", row.n, row.e, True, row.K) == single, row.why
    assert ops.step_tail_plan("code_stats_levels", row.n, row.e, True, row.K) == levels, row.why


def test_plan_is_the_rule_on_a_grid(ops):
    """Around every threshold of the rules, both alignments: the library against form_of() / stats_forms() on made-up rows."""
    for count in (1, 3, 4, 4095, 4096, 4097, 16384, 16385, 1044480, 1044481, 4177920, 4177921, 5000000):
        for off in (0, 1):
            for row in (tc.Recon(count, 0, off, 0, 0, True, 1, ""), tc.Norm(count, off, 1.0, "")):
                assert ops.step_tail_plan(*tc.plan_args(row)) == tc.form_of(row), row
    for n in (1, 63, 64, 65, 448, 449, 511, 512, 513, 1024, 5000):
        for F in (1, 15, 16, 17, 112, 128, 200, 2048):
            row = tc.Relu(n, F, "relu", 0, "")
            assert ops.step_tail_plan(*tc.plan_args(row)) == tc.form_of(row), row
    for e in (16, 32, 48, 64, 128):
        for n in (1, 5, 1024 // e, 4 * (1024 // e), 4 * (1024 // e) + 1, 65536 // e, 65536 // e + 1, 3000000):
            row = tc.Qg(n, e, 1, 0, "")
            assert ops.step_tail_plan(*tc.plan_args(row)) == tc.form_of(row), row
    for e in (4, 16, 64, 256):
        for n in (1, 77, 4096, 8200, 100000):
            row = tc.Apply(n, e, False, 1, False, "valid", "")
            assert ops.step_tail_plan(*tc.plan_args(row)) == tc.form_of(row), row
    for e in (16, 32, 64):
        for n in (1, 255, 8192, 8193, 100000):
            for K in (1, 7, 256, 1024, 1025, 4096):
                single, levels = tc.stats_forms(tc.Stats(n, e, K, "spread", ""))
                assert ops.step_tail_plan("code_stats", n, e, True, K) == single, (n, e, K)
                assert ops.step_tail_plan("code_stats_levels", n, e, True, K) == levels, (n, e, K)


def test_the_forms_the_issue_names(ops):
    """Literal spot checks, so that form_of() and the library cannot drift together."""
    p = ops.step_tail_plan
    assert p("recon_loss_grad", 3, 0, True)["tail"] == 3 and p("recon_loss_grad", 4099, 0, True)["grid"] == 2
    assert p("recon_loss_grad", 1044480, 0, True)["grid"] == 255 and p("recon_loss_grad", 1100003, 0, True)["grid"] == 256
    assert p("recon_loss_grad", 1100003, 0, False)["tail"] == 1100003 and p("recon_loss_grad", 1100003, 0, False)["vec16"] == 0
    assert p("grad_norm_clip", 4177920, 0, True)["grid"] == 255 and p("grad_norm_clip", 4200003, 0, True) == tc.form(
        "reduce", 256, vec16=1, tail=3, second_launch=1)
    assert p("relu_bias_backward", 512, 128) == tc.form("strip", 8, cols=16, xcd_order=1, tail=0)
    assert p("relu_bias_backward", 513, 200) == tc.form("strip", 13, cols=16, xcd_order=0, tail=1)
    assert p("quantizer_input_grad_bias", 4096, 16)["family"] == "qgb_one" and p("quantizer_input_grad_bias", 4097, 16)["family"] == "qg_two"
    assert p("quantizer_input_grad_bias", 100, 48) == tc.form("qg_two", 5, second_launch=1)
    assert p("rq_apply_level", 8200, 64)["grid"] == 513 and p("rq_apply_level", 8200, 64)["grid_sse"] == 256
    assert p("code_stats", 8192, 32, True, 1024)["family"] == "cs_sorted" and p("code_stats", 8193, 32, True, 1024)["family"] == "cs_streaming"
    assert p("code_stats", 8192, 32, True, 1025)["family"] == "cs_streaming"
    assert p("code_stats_levels", 8192, 32, True, 1024)["family"] == "cs_levels" and p("code_stats_levels", 8193, 32, True, 7)["family"] == "cs_per_level"
    for bad in (lambda: p("code_stats", 10, 48, True, 7), lambda: p("recon_loss_grad", 0), lambda: p("code_stats", 10, 16, True, 0)):
        with pytest.raises(Exception):
            bad()


def test_the_table_reaches_every_launch_the_plan_can_report(ops):
    """Over the admitted ranges: every family; both sides of every flag; a capped and an uncapped grid; tail and no tail."""
    rows = {id(r): tc.form_of(r) for r in PLANNED}
    forms = list(rows.values()) + [f for r in tc.STATS for f in tc.stats_forms(r)]
    assert {f["family"] for f in forms} == set(ops.TAIL_FAMILIES)
    for call, per in (("recon", 4), ("norm", 16)):
        red = [tc.form_of(r) for r in (tc.RECON if call == "recon" else tc.NORM)]
        assert {(f["vec16"], f["grid"] == tc.RED_CAP, f["tail"] > 0 if f["vec16"] else True) for f in red} >= {
            (1, False, True), (1, True, True), (0, False, True), (0, True, True)}
        assert any(f["grid"] == 1 for f in red) and any(1 < f["grid"] < tc.RED_CAP for f in red)
    assert any(f["vec16"] and f["tail"] == 0 for f in (tc.form_of(r) for r in tc.RECON))
    strips = [tc.form_of(r) for r in tc.RELU]
    assert {f["xcd_order"] for f in strips} == {0, 1} and {f["tail"] == 0 for f in strips} == {True, False}
    qg = [tc.form_of(r) for r in tc.QG]
    assert {(f["family"], f["tail"] == 0) for f in qg} >= {("qgb_one", True), ("qgb_one", False), ("qg_two", True)}
    ap = [tc.form_of(r) for r in tc.APPLY]
    assert any(f["grid_sse"] < f["grid"] for f in ap) and any(f["grid_sse"] == f["grid"] for f in ap)
    for e in (16, 32, 64):
        assert {f["family"] for r in tc.STATS if r.e == e for f in tc.stats_forms(r)} == {"cs_sorted", "cs_streaming", "cs_levels", "cs_per_level"}
        assert {r.e for r in tc.QG if tc.form_of(r)["family"] == "qgb_one"} == {16, 32, 64}
    every = PLANNED + tc.CBGRAD + tc.LOSSES + tc.STATS + tc.EMA
    assert len({(type(r).__name__, tc.row_id(r)) for r in every}) == len(every)


# ---------------------------------------------------------------- the builders keep their promises

@pytest.mark.parametrize("row", tc.RECON, ids=tc.row_id)
def test_recon_inputs_and_reference(row):
    out, x = tc.recon_inputs(row)
    d = out - x
    n = row.count
    assert (d[0::3] > 0).all() and (d[1::3] < 0).all() and (d[2::3] == 0).all() and n >= 3
    total = n * row.total_factor
    g, exact, model = ref.recon_loss_grad(out, x, total, row.l1)
    assert g.dtype == np.float32 and g.shape == (n,) and np.isfinite(g).all()
    if row.l1:
        assert set(np.unique(g)) == {np.float32(0), np.float32(1) / np.float32(total), -(np.float32(1) / np.float32(total))}
    # the fp64-accumulated model against the exact sum: inside the 1 ulp the GPU test allows
    assert abs(float(model) - exact) <= ref.ulp32(exact)
    long_exact = np.sum(np.abs(d).astype(np.longdouble) if row.l1 else d.astype(np.longdouble) ** 2) / np.longdouble(total)
    assert abs(float(long_exact) - exact) <= 2.0 ** -30 * abs(exact)


@pytest.mark.parametrize("row", tc.NORM, ids=tc.row_id)
def test_norm_inputs_and_reference(row):
    g = tc.norm_inputs(row)
    exact, model = ref.grad_norm(g)
    assert abs(float(model) - exact) <= ref.ulp32(exact)
    below = exact < row.max_norm
    assert below == (row.count == 1)
    coef = ref.clip_coef(np.float32(exact), row.max_norm)
    assert (coef == np.float32(1.0)) == below and 0 < coef <= 1
    assert {r.count == 1 for r in tc.NORM} == {True, False}


@pytest.mark.parametrize("row", [r for r in tc.RELU if r.variant in ("relu", "norelu")], ids=tc.row_id)
def test_relu_inputs_and_reference(row):
    gy, y = tc.relu_inputs(row)
    yb = ref.bits(y)
    if y.size >= 12:
        assert (yb == 0).any() and (yb == 0x80000000).any()
    if y.size >= 64:
        assert (y > 0).any() and (y < 0).any()
    g = ref.relu_bias_backward(gy, y, row.variant == "relu")
    if row.variant == "relu":
        assert (ref.bits(g)[y.reshape(g.shape) == 0] == 0).all()            # +0.0 for both zeros, never -0.0 * gy
    want, bound = ref.colsum_bounds(g)
    assert (np.abs(ref.colsum_model(g).astype(np.float64) - want) <= bound).all()


@pytest.mark.parametrize("row", tc.QG, ids=tc.row_id)
def test_qg_inputs_and_reference(row):
    z, cb0, idx, g_xq = tc.qg_inputs(row)
    assert idx.shape == (row.n, row.idx_cols) and idx[:, 0].min() >= 0 and idx[:, 0].max() < tc.QG_K
    assert row.idx_cols == 1 or (idx[:, 1:] >= tc.QG_K).all()
    out = ref.quantizer_input_grad(z, cb0, idx[:, 0], tc.QG_COEF, tc.QG_WEIGHT, g_xq)
    other = out.astype(np.float64) - g_xq
    ratio = np.abs(g_xq).mean() / np.abs(other).mean()
    assert 0.3 < ratio < 3.0                                               # neither term hides the other
    long = (np.longdouble(tc.QG_COEF) * (z.astype(np.longdouble) - cb0[idx[:, 0]]) * np.longdouble(tc.QG_WEIGHT) + g_xq)
    assert np.abs(out - long).max() <= 4 * 2.0 ** -24 * np.abs(long).max() + 4 * 2.0 ** -24 * np.abs(other).max()
    want, bound = ref.colsum_bounds(out)
    assert (np.abs(ref.colsum_model(out).astype(np.float64) - want) <= bound).all()
    assert {r.idx_cols for r in tc.QG if tc.form_of(r)["family"] == "qgb_one"} == {1, 4, 5}


def test_cbgrad_sizes():
    assert [r.K * r.e for r in tc.CBGRAD] == [255, 256, 257]
    for row in tc.CBGRAD:
        count, total, cb, scale, weight = tc.cbgrad_inputs(row)
        g = ref.codebook_grad(count, total, cb, scale, weight)
        long = (np.longdouble(scale) * (count[:, None].astype(np.longdouble) * cb - total)) * np.longdouble(weight)
        assert np.abs(g - long).max() <= 8 * 2.0 ** -24 * np.abs(long).max()


@pytest.mark.parametrize("row", tc.LOSSES, ids=tc.row_id)
def test_losses_inputs_and_reference(row):
    (sse1, rec1, probe1), (sse2, rec2, probe2) = tc.losses_inputs(row)
    assert np.isnan(rec1) == (row.nan == "recon") and np.isnan(sse1).any() == (row.nan == "sse")
    assert (probe1 < 0) == (row.probe < 0) and probe2 >= 0 and np.isfinite(sse2).all() and np.isfinite(rec2)
    out = ref.step_losses(sse1, tc.LOSS_N, tc.LOSS_E, tc.LOSS_BETA, tc.LOSS_QLW, rec1)
    assert np.isnan(out[0]) == (row.nan != "none")
    out2 = ref.step_losses(sse2, tc.LOSS_N, tc.LOSS_E, tc.LOSS_BETA, tc.LOSS_QLW, rec2)
    mse = sse2 / (tc.LOSS_N * tc.LOSS_E)
    assert abs(float(out2[2]) - float(np.mean(mse * (1 + tc.LOSS_BETA)))) <= 1e-6 * float(out2[2])
    assert {r.L for r in tc.LOSSES} == {1, 4, 8}


@pytest.mark.parametrize("row", tc.APPLY, ids=tc.row_id)
def test_apply_inputs_and_reference(oracle, row):
    resid, cb, idx, xq = tc.apply_inputs(row)
    col = idx[:, -1]
    assert (xq is not None) == row.accumulate and idx.shape[1] == row.idx_cols
    if row.idx_kind == "oor":
        assert list(col[:4]) == [-1, tc.APPLY_K, 2 ** 32 + 1, -2 ** 40] and ((col[4:] >= 0) & (col[4:] < tc.APPLY_K)).all()
        assert list(ref.clamp_codes(col[:4], tc.APPLY_K)) == [0, tc.APPLY_K - 1, tc.APPLY_K - 1, 0]
    elif row.idx_kind == "oor1":
        assert col[0] == -1
    else:
        assert ((col >= 0) & (col < tc.APPLY_K)).all()
    xo, ro, sse = ref.apply_level(resid, cb, col, xq)
    if row.idx_kind == "oracle":
        o = oracle.rq_assign(resid, [cb], want_resid=True)
        assert np.array_equal(ref.bits(xo), ref.bits(o["xq"])) and np.array_equal(ref.bits(ro), ref.bits(o["resid"][1]))
        assert abs(sse - o["sse"][0]) <= (resid.size * 2.0 ** -53 + 2.0 ** -23) * sse
    assert {r.idx_kind for r in tc.APPLY} == {"valid", "oor", "oor1", "oracle"}


@pytest.mark.parametrize("row", tc.STATS, ids=tc.row_id)
def test_stats_inputs_and_reference(oracle, row):
    idx, resid, cbs = tc.stats_inputs(row)
    assert idx.shape == (row.n, tc.STATS_L)
    for l in range(tc.STATS_L):
        col = idx[:, l]
        inside = (col >= 0) & (col < row.K)
        if row.pattern == "oor":
            assert not inside[:min(4, row.n)].any() and inside[4:].all()
            assert col[0] == -1 and (row.n < 2 or col[1] == row.K) and (row.n < 3 or col[2] == 2 ** 32 + 1)
        elif row.pattern == "poison":
            assert (col == -1).all()
        else:
            assert inside.all()
        count, total = ref.code_stats(col, resid[l], row.K)
        if row.pattern in ("one", "poison"):
            assert (count > 0).sum() == 1 and count.max() == row.n and (row.pattern == "one" or count[0] == row.n)
        if row.pattern == "spread" and row.K > 2:
            assert (count == 0).any()
        o_count, o_total = oracle.code_stats(ref.clamp_codes(col, row.K), resid[l], row.K)
        assert np.array_equal(ref.bits(count), ref.bits(o_count)) and np.array_equal(ref.bits(total), ref.bits(o_total))


@pytest.mark.parametrize("row", [r for r in tc.EMA if r.skip is None], ids=tc.row_id)
def test_ema_inputs_and_reference(oracle, row):
    ema_count, ema_sum, cb, count, total = tc.ema_inputs(row)
    en, ew, new_cb, _ = ref.ema_update(ema_count, ema_sum, cb, count, total, tc.EMA_DECAY, tc.EMA_EPS)
    eps = np.float32(tc.EMA_EPS)
    assert en[0] < eps and en[1] == eps and en[2] > eps                     # below, exactly on and just above eps
    assert en[0] == np.nextafter(eps, np.float32(0)) and en[2] == np.nextafter(eps, np.float32(1))
    assert np.array_equal(new_cb[:2], cb[:2]) and not np.array_equal(new_cb[2], cb[2])
    o = oracle.ema_update(ema_count, ema_sum, cb, count, total, tc.EMA_DECAY, tc.EMA_EPS)
    for mine, theirs in zip((en, ew, new_cb), o):
        assert np.array_equal(ref.bits(mine), ref.bits(theirs))


def test_fma32_rounds_once():
    """a * b + c a hair below a float32 midpoint, the hair below float64's resolution at c: float64 addition alone lands on the
    tie and rounds to even (up); one rounding of the exact value rounds down."""
    a, b, c = np.float32(2.0 ** 15 + 2.0 ** -8), np.float32(2.0 ** 14 - 2.0 ** -9), np.float32(2.0 ** 53 + 2.0 ** 30)
    assert float(a) * float(b) == 2.0 ** 29 - 2.0 ** -17 and float(c) == 2.0 ** 53 + 2.0 ** 30
    # exact: 2^53 + 2^30 + 2^29 - 2^-17; float32's spacing at 2^53 is 2^30, so 2^53 + 2^30 + 2^29 is a tie whose even side is up
    assert float(np.float32(float(a) * float(b) + float(c))) == 2.0 ** 53 + 2.0 ** 31
    assert float(ref.fma32(a, b, c)) == 2.0 ** 53 + 2.0 ** 30
    assert float(ref.fma32(np.float32(2.0 ** 29), np.float32(1.0), c)) == 2.0 ** 53 + 2.0 ** 31      # exactly the tie: to even
    assert float(ref.fma32(np.float32(3.0), np.float32(5.0), np.float32(0.25))) == 15.25
    assert math.isnan(float(ref.fma32(np.float32(np.nan), a, a)))
