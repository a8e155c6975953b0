"""GPU: every row of tests/step_tail_cases.py through its call of the C ABI, every operand carved out of a sentinel-filled buffer
at the row's offset.  Per row: the library's plan reports the launch the row is listed for; every element-wise output has the bits
of the float32 model in tests/step_tail_ref.py (and of the C oracle where it has the operation); fp64-accumulated scalars are within
1 float32 ulp of the exact sum; fp32 column sums are within (n - 1) 2^-24 sum |v| of the fp64 column sum of the bit-checked
elements; a second run gives the same bits, the ticket and the two-launch forms give the same bits, the ticket word is zero again
and no sentinel beside any operand has changed."""
import os
import subprocess
import sys

import numpy as np
import pytest

import step_tail_cases as tc
import step_tail_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev():
    import torch
    return torch.device(DEV)


def assert_same_bits(a, b, what):
    """Two results of a run_*: dicts of arrays, lists, tuples and scalars."""
    if isinstance(a, dict):
        assert sorted(a) == sorted(b)
        for k in a:
            assert_same_bits(a[k], b[k], f"{what} {k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            assert_same_bits(x, y, f"{what}[{i}]")
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"{what}: the bits differ between two runs"
    else:
        assert a == b, what


def twice(run, what):
    first = run()
    assert_same_bits(first, run(), what)
    return first


def assert_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.flatnonzero(ref.bits(got).ravel() != ref.bits(want).ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} elements differ, first at {bad[0]}: {got.ravel()[bad[0]]!r} vs {want.ravel()[bad[0]]!r}"


def assert_within_one_ulp(got, exact, what):
    """got: a positive float32 from the GPU; exact: the exact value as float64."""
    want = np.float32(exact)
    dist = abs(int(ref.bits(np.float32(got).reshape(1))[0]) - int(ref.bits(want.reshape(1))[0]))
    print(f"{what}: got {float(got)!r} exact {exact!r} ulps {dist}")
    assert dist <= 1, f"{what}: {float(got)!r} is {dist} float32 ulps from {exact!r}"


def assert_colsums(got, elements, what):
    want, bound = ref.colsum_bounds(elements)
    err = np.abs(got.astype(np.float64) - want)
    print(f"{what}: worst column error / bound {float((err / np.maximum(bound, 1e-300)).max()) if bound.max() > 0 else 0.0:.3g}")
    assert (err <= bound).all(), f"{what}: column {int(np.argmax(err - bound))}: error {err.max()!r} above its bound"


def assert_plan(hip, row):
    call, n, width, aligned, K = tc.plan_args(row)
    assert hip.ops.step_tail_plan(call, n, width, aligned, K) == tc.form_of(row), row.why


@pytest.mark.parametrize("row", tc.RECON, ids=tc.row_id)
def test_recon_loss_grad_row(hip, row):
    assert_plan(hip, row)
    res = twice(lambda: tc.run_recon(hip, row, dev(), tickets=True), "recon_loss_grad")
    assert_same_bits(res, tc.run_recon(hip, row, dev(), tickets=False), "ticket vs two launches")
    out, x = tc.recon_inputs(row)
    g, exact, _ = ref.recon_loss_grad(out, x, row.count * row.total_factor, row.l1)
    assert ("grad" in res) == row.want_grad
    if row.want_grad:
        assert_bits(res["grad"], g, "grad")
    assert_within_one_ulp(res["loss"][0], exact, "loss")


@pytest.mark.parametrize("row", tc.NORM, ids=tc.row_id)
def test_grad_norm_clip_row(hip, row):
    assert_plan(hip, row)
    res = twice(lambda: tc.run_norm(hip, row, dev(), tickets=True), "grad_norm_clip")
    assert_same_bits(res, tc.run_norm(hip, row, dev(), tickets=False), "ticket vs two launches")
    exact, _ = ref.grad_norm(tc.norm_inputs(row))
    norm, coef = res["norm_coef"]
    assert_within_one_ulp(norm, exact, "norm")
    assert_bits(np.float32(coef).reshape(1), np.float32(ref.clip_coef(norm, row.max_norm)).reshape(1), "clip coefficient")
    assert (coef == np.float32(1.0)) == (row.count == 1)


def check_relu_row(hip, row):
    assert_plan(hip, row)
    res = twice(lambda: tc.run_relu(hip, row, dev()), "relu_bias_backward")
    gy, y = tc.relu_inputs(row)
    g = ref.relu_bias_backward(gy, y, row.variant != "norelu")
    if row.variant == "no_g_out":
        assert_bits(res["gy_after"], gy, "gy (g_out == NULL: nothing written)")
    else:
        assert_bits(res["g"], g, "g")
    assert ("dbias" in res) == (row.variant != "no_dbias")
    if "dbias" in res:
        assert_colsums(res["dbias"], g, "dbias")


@pytest.mark.parametrize("row", tc.RELU, ids=tc.row_id)
def test_relu_bias_backward_row(hip, row):
    check_relu_row(hip, row)


def test_relu_rows_under_forced_strip_widths(hip):
    """The 8- and 32-column instantiations: the library reads LCREC_STRIP_COLS once per process, so the rows run again in one
    fresh child process per width, one after the other, the second only if the first passed."""
    for width in ("8", "32"):
        env = dict(os.environ, LCREC_STRIP_COLS=width)
        done = subprocess.run([sys.executable, *subprocess._args_from_interpreter_flags(), os.path.abspath(__file__)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
        assert done.returncode == 0, f"LCREC_STRIP_COLS={width}:\n{done.stdout[-3000:]}"
        assert f"{len(tc.RELU)} relu_bias_backward rows passed at strip width {width}" in done.stdout, done.stdout[-1000:]


@pytest.mark.parametrize("row", tc.QG, ids=tc.row_id)
def test_quantizer_input_grad_row(hip, row):
    assert_plan(hip, row)
    plain = twice(lambda: tc.run_qg(hip, row, dev(), bias=False), "quantizer_input_grad")
    fused = twice(lambda: tc.run_qg(hip, row, dev(), bias=True), "quantizer_input_grad_bias")
    z, cb0, idx, g_xq = tc.qg_inputs(row)
    want = ref.quantizer_input_grad(z, cb0, idx[:, 0], tc.QG_COEF, tc.QG_WEIGHT, g_xq)
    assert_bits(plain["out"], want, "out of quantizer_input_grad")
    assert_bits(fused["out"], want, "out of quantizer_input_grad_bias")
    assert_colsums(fused["dbias"], want, "dbias")


@pytest.mark.parametrize("row", tc.CBGRAD, ids=tc.row_id)
def test_codebook_grad_row(hip, row):
    res = twice(lambda: tc.run_cbgrad(hip, row, dev()), "codebook_grad")
    assert_bits(res["grad"], ref.codebook_grad(*tc.cbgrad_inputs(row)), "grad")


def assert_bits_or_nan(got, want, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert_bits(np.where(nan, 0, got).astype(got.dtype), np.where(nan, 0, want).astype(want.dtype), what)


@pytest.mark.parametrize("row", tc.LOSSES, ids=tc.row_id)
def test_step_losses_row(hip, row):
    res = twice(lambda: tc.run_losses(hip, row, dev()), "step_losses")
    (sse1, rec1, probe1), (sse2, rec2, _) = tc.losses_inputs(row)
    want1 = ref.step_losses(sse1, tc.LOSS_N, tc.LOSS_E, tc.LOSS_BETA, tc.LOSS_QLW, rec1)
    want2 = ref.step_losses(sse2, tc.LOSS_N, tc.LOSS_E, tc.LOSS_BETA, tc.LOSS_QLW, rec2)
    assert_bits_or_nan(res["out3_1"], want1, "losses of the first call")
    assert_bits(res["out3_2"], want2, "losses of the second call")
    flags = (int(row.nan != "none"), int(probe1 < 0))
    assert res["flags_1"] == flags and res["flags_2"] == flags, "the NaN and poison flags are sticky"
    assert ("sums" in res) == row.sums
    if row.sums:
        with np.errstate(invalid="ignore"):
            want = np.array([(0.0 + float(want1[0])) + float(want2[0]), (0.0 + float(want1[1])) + float(want2[1])])
        assert_bits_or_nan(res["sums"], want, "running sums")


@pytest.mark.parametrize("row", tc.APPLY, ids=tc.row_id)
def test_rq_apply_level_row(hip, oracle, row):
    assert_plan(hip, row)
    res = twice(lambda: tc.run_apply(hip, row, dev(), tickets=True), "rq_apply_level")
    assert_same_bits(res, tc.run_apply(hip, row, dev(), tickets=False), "ticket vs two launches")
    resid, cb, idx, xq = tc.apply_inputs(row)
    xo, ro, sse = ref.apply_level(resid, cb, idx[:, -1], xq)
    assert_bits(res["xq"], xo, "xq")
    assert_bits(res["resid"], ro, "resid")
    rtol = resid.size * 2.0 ** -53 + 2.0 ** -23
    print(f"sse: got {res['sse'][0]!r} exact {sse!r} relative error {abs(res['sse'][0] - sse) / sse:.3g} rtol {rtol:.3g}")
    assert abs(res["sse"][0] - sse) <= rtol * sse
    if row.idx_kind == "oracle":
        o = oracle.rq_assign(resid, [cb], want_resid=True)
        assert_bits(res["xq"], o["xq"], "xq vs the oracle")
        assert_bits(res["resid"], o["resid"][1], "resid vs the oracle")
        assert abs(res["sse"][0] - o["sse"][0]) <= rtol * sse


@pytest.mark.parametrize("row", tc.STATS, ids=tc.row_id)
def test_code_stats_row(hip, oracle, row):
    single, levels = tc.stats_forms(row)
    assert hip.ops.step_tail_plan("code_stats", row.n, row.e, True, row.K) == single
    assert hip.ops.step_tail_plan("code_stats_levels", row.n, row.e, True, row.K) == levels
    res = twice(lambda: tc.run_stats(hip, row, dev()), "code_stats")
    idx, resid, cbs = tc.stats_inputs(row)
    for l in range(tc.STATS_L):
        count, total = ref.code_stats(idx[:, l], resid[l], row.K)
        o_count, o_total = oracle.code_stats(ref.clamp_codes(idx[:, l], row.K), resid[l], row.K)
        for name, (c, s) in (("code_stats", res["single"][l]), ("code_stats_levels", res["levels"][l][:2])):
            what = f"{name} ({single['family'] if name == 'code_stats' else levels['family']}) level {l}"
            assert_bits(c, count, what + " count")
            assert_bits(s, total, what + " sum")
            assert_bits(c, o_count, what + " count vs the oracle on the clamped codes")
            assert_bits(s, o_total, what + " sum vs the oracle on the clamped codes")
        assert_bits(res["levels"][l][2], ref.codebook_grad(count, total, cbs[l], tc.STATS_SCALE, tc.STATS_WEIGHT), f"fused codebook gradient level {l}")


@pytest.mark.parametrize("row", tc.EMA, ids=tc.row_id)
def test_ema_update_row(hip, oracle, row):
    res = twice(lambda: tc.run_ema(hip, row, dev()), "ema_update")
    ema_count, ema_sum, cb, count, total = tc.ema_inputs(row)
    if row.skip:
        want = (ema_count, ema_sum, cb)
    else:
        want = ref.ema_update(ema_count, ema_sum, cb, count, total, tc.EMA_DECAY, tc.EMA_EPS)[:3]
        for name, o in zip(("ema_count", "ema_sum", "codebook"), oracle.ema_update(ema_count, ema_sum, cb, count, total, tc.EMA_DECAY, tc.EMA_EPS)):
            assert_bits(res[name], o, name + " vs the oracle")
    for name, w in zip(("ema_count", "ema_sum", "codebook"), want):
        assert_bits(res[name], w, name)


if __name__ == "__main__":          # the child process of test_relu_rows_under_forced_strip_widths
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import lcrec_amd
    lcrec_amd._lib.load()
    for relu_row in tc.RELU:
        check_relu_row(lcrec_amd, relu_row)
    print(f"{len(tc.RELU)} relu_bias_backward rows passed at strip width {tc.strip_cols()}")
