"""The case table of the BatchNorm strip kernels (csrc/train_ops.hip: the dword strips bn_relu_forward_kernel /
bn_relu_backward_kernel and the float4 strips bn_relu_forward_v4_kernel / bn_relu_backward_v4_kernel), shared by
tests/test_bn_plan_host.py (CPU: every row gets the form it is listed for, asked of the library's own plan), by
tests/test_gpu_bn_forms.py (GPU: every row against torch fp64 and against the recorded bits) and by tools/record_bn_forms.py
(which writes tests/golden/f12_bn_forms.json from the same calls).

A row is a shape (n, F) with the form of the kernel each call must take for it -- `whole` for bn_relu_forward / bn_relu_backward,
`stats` / `reduce` / `apply` for the data-parallel halves (the dword strips do not narrow for those) -- and the reason the row is
there.  Shapes are the smallest that reach their form; the dispatch, not this file, decides what a shape reaches."""
import functools
import hashlib
from collections import OrderedDict, namedtuple

import numpy as np

CALLS = ("forward", "backward", "stats", "reduce", "apply")        # `call` of lcrec_debug_bn_plan, in this order from 0
EPS, MOMENTUM = 1e-5, 0.1

# what lcrec_debug_bn_plan reports (ops.bn_plan): float4 or dword strips, strip width, rows per lane (float4 only, else 0), the
# register-cached instantiation (dword forward / backward only), workgroups, and whether workgroup b takes the XCD-neighbour
# strip (b % 8) * (grid / 8) + b / 8
Form = namedtuple("Form", "float4 cols rows_per_lane cached grid xcd_order")


def v4(cols, rows_per_lane, grid, xcd):
    return Form(1, cols, rows_per_lane, 0, grid, int(xcd))


def dw(cols, grid, xcd, cached=False):
    return Form(0, cols, 0, int(cached), grid, int(xcd))


Case = namedtuple("Case", "n F whole stats reduce apply gamma_off relu_false why")


def _case(n, F, whole, why, split=None, gamma_off=False, relu_false=False, **calls):
    split = split or whole
    return Case(n, F, whole, calls.get("stats", split), calls.get("reduce", split), calls.get("apply", split), gamma_off, relu_false, why)


CASES = [
    # float4, width 16, F 512: 32 strips in XCD-neighbour order, 256 row groups
    _case(200, 512, v4(16, 1, 32, True), "float4 width 16, 1 row per lane"),
    _case(300, 512, v4(16, 2, 32, True), "float4 width 16, 2 rows per lane"),
    _case(600, 512, v4(16, 4, 32, True), "float4 width 16, 4 rows per lane", relu_false=True),
    _case(1500, 512, v4(16, 8, 32, True), "float4 width 16, 8 rows per lane"),
    _case(3000, 512, v4(8, 8, 64, True), "float4 narrowed to width 8 by the row count"),
    _case(6000, 512, v4(4, 8, 128, True), "float4 narrowed to width 4 by the row count"),
    _case(257, 516, v4(16, 2, 33, False), "float4 width 16, plain strip order, 4 live columns in the last strip, one row past a row group"),
    # float4, width 8, F 256: 512 row groups
    _case(400, 256, v4(8, 1, 32, True), "float4 width 8, 1 row per lane"),
    _case(700, 256, v4(8, 2, 32, True), "float4 width 8, 2 rows per lane"),
    _case(1500, 256, v4(8, 4, 32, True), "float4 width 8, 4 rows per lane"),
    _case(3000, 256, v4(8, 8, 32, True), "float4 width 8, 8 rows per lane"),
    # float4, width 4: 1024 row groups
    _case(700, 36, v4(4, 1, 9, False), "float4 width 4, 1 row per lane, plain strip order"),
    _case(1500, 36, v4(4, 2, 9, False), "float4 width 4, 2 rows per lane"),
    _case(3000, 36, v4(4, 4, 9, False), "float4 width 4, 4 rows per lane"),
    _case(6000, 36, v4(4, 8, 9, False), "float4 width 4, 8 rows per lane"),
    _case(2, 32, v4(4, 1, 8, True), "float4 width 4, XCD-neighbour order, the smallest batch"),
    # dword, F 66: 5 strips of 16 columns, 2 live columns in the last; 64 row groups (128 at width 8)
    _case(2, 66, dw(16, 5, False), "dword, the smallest batch"),
    _case(70, 66, dw(16, 5, False), "dword, tail loop only"),
    _case(600, 66, dw(16, 5, False), "dword, unrolled loop and tail", relu_false=True),
    _case(1500, 66, dw(16, 5, False, cached=True), "dword, register-cached forward / backward", split=dw(16, 5, False)),
    _case(2049, 66, dw(8, 9, False, cached=True), "dword narrowed to width 8 for forward / backward, register-cached",
          split=dw(16, 5, False)),
    _case(5000, 66, dw(8, 9, False), "dword width 8, two-pass: more rows than the register-cached form takes", split=dw(16, 5, False)),
    # dword, other routes
    _case(300, 126, dw(16, 8, True), "dword in XCD-neighbour order"),
    _case(300, 128, dw(16, 8, True), "dword by alignment: gamma is a view one float into a larger buffer (the calls without gamma stay float4)",
          gamma_off=True, stats=v4(4, 1, 32, True), reduce=v4(4, 1, 32, True)),
    _case(8193, 512, dw(8, 64, True), "dword, one row more than the float4 kernels take", split=dw(16, 32, True)),
]


def case_id(c):
    return f"{c.n}x{c.F}"


def runs():
    """(case, relu) pairs: every case with ReLU, two of them also without."""
    return [(c, True) for c in CASES] + [(c, False) for c in CASES if c.relu_false]


def run_id(run):
    return case_id(run[0]) + ("" if run[1] else "-norelu")


def stats_row_form(c):
    """bn_stats into an exchange row writes at row[1:], 4 bytes off 16-byte alignment: always the dword strips, not narrowed."""
    grid = -(-c.F // 16)
    return dw(16, grid, grid % 8 == 0)


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# What makes a row's inputs judgeable against fp64 to the tolerances of a 1 k-row batch, ensured by inputs() for every row (and
# asserted there under fp64 alone, before any kernel runs):
#  - no column's standard deviation is below MIN_STD.  Two close values in a two-row batch make rstd up to 1 / sqrt(eps) = 316
#    while t - mean cancels: the fp32 inputs themselves do not carry dt to 1e-4 there, whatever computes it;
#  - no pre-activation (t - mean) * rstd * gamma + beta lies within MARGIN of the ReLU kink.  There rounding decides the mask --
#    fp64, the forward's expression and the fused fma(t, scale, shift) each their own way (rounding errors of a few 1e-6 at
#    |t| <= 15) -- and ONE flipped element changes its whole column of dt by gy / n: at 8193 x 512 there is about one such element.
MIN_STD = 1.0
MARGIN = 1e-4


def preactivation(t, gamma, beta):
    """(t - mean) * rstd * gamma + beta in fp64."""
    t = t.astype(np.float64)
    return (t - t.mean(0)) / np.sqrt(t.var(0) + EPS) * gamma + beta


@functools.lru_cache(maxsize=2)
def inputs(c):
    """t [n, F] with column means far from 0, gamma, beta, running_mean, running_var, gy [n, F]: fp32, seeded by the shape.
    Shared by the callers of a row: read only."""
    rs = np.random.RandomState(1000 * c.F + c.n)
    t = rs.standard_normal((c.n, c.F)) * 2.0 + rs.standard_normal(c.F) * 3.0
    gamma, beta = f32(1 + 0.2 * rs.standard_normal(c.F)), f32(0.3 * rs.standard_normal(c.F))
    rm, rv = f32(0.1 * rs.standard_normal(c.F)), f32(0.5 + rs.uniform(size=c.F))
    gy = f32(rs.standard_normal((c.n, c.F)))
    assert np.abs(gamma).min() > 0.1
    std = t.std(0)
    t = t.mean(0) + (t - t.mean(0)) * np.where(std < MIN_STD, MIN_STD / std, 1.0)
    pre = preactivation(f32(t), gamma, beta)
    if c.n == 2:        # xhat is +-1 whatever t is: the kink is left by moving beta
        near = np.abs(pre).min(0) < 2 * MARGIN
        beta = f32(beta + np.where(near, 8 * MARGIN, 0.0))
    else:               # elements nearer than 2 MARGIN go out to 4 MARGIN, on their own side
        near = np.abs(pre) < 2 * MARGIN
        step = np.where(pre >= 0, 1.0, -1.0) * 4 * MARGIN * np.sqrt(t.var(0) + EPS) / gamma
        t = np.where(near, t + step - pre * np.sqrt(t.var(0) + EPS) / gamma, t)
    t = f32(t)
    assert np.abs(preactivation(t, gamma, beta)).min() >= MARGIN and t.astype(np.float64).std(0).min() >= 0.999 * MIN_STD
    return t, gamma, beta, rm, rv, gy


def run_calls(ops, c, relu, device):
    """Every call of the table on the case's inputs.  Returns (outputs, aligned): outputs[name] is an OrderedDict of the call's
    output tensors, aligned[name] whether every pointer the call passed sat on 16 bytes (what lcrec_debug_bn_plan is asked with)."""
    import torch
    t, gamma, beta, rm, rv, gy = inputs(c)
    d = lambda a: torch.from_numpy(a).to(device)
    t_d, beta_d, gy_d = d(t), d(beta), d(gy)
    if c.gamma_off:
        buf = torch.zeros(c.F + 4, dtype=torch.float32, device=device)
        gamma_d = buf[1:c.F + 1]
        gamma_d.copy_(d(gamma))
    else:
        gamma_d = d(gamma)
    on16 = lambda *ts: all(x is None or x.data_ptr() % 16 == 0 for x in ts)
    out, aligned = OrderedDict(), {}

    rm_d, rv_d = d(rm), d(rv)
    y, mean, rstd = ops.bn_relu_forward(t_d, gamma_d, beta_d, EPS, MOMENTUM, rm_d, rv_d, relu=relu)
    out["forward_running"] = OrderedDict(y=y, mean=mean, rstd=rstd, running_mean=rm_d, running_var=rv_d)
    aligned["forward_running"] = on16(t_d, gamma_d, beta_d, rm_d, rv_d, y, mean, rstd)
    y2, mean2, rstd2 = ops.bn_relu_forward(t_d, gamma_d, beta_d, EPS, MOMENTUM, None, None, relu=relu)
    out["forward"] = OrderedDict(y=y2, mean=mean2, rstd=rstd2)
    aligned["forward"] = on16(t_d, gamma_d, beta_d, y2, mean2, rstd2)

    # the folded affine of the same BatchNorm, on the host in fp32
    scale = f32(gamma * rstd.cpu().numpy())
    shift = f32(beta - mean.cpu().numpy() * scale)
    fold = (d(scale), d(shift))
    for name, kw in (("backward_y", dict(y=y)), ("backward_beta", dict(y=None, beta=beta_d)), ("backward_fold", dict(y=None, fold=fold))):
        dt, dg, db, dbias = ops.bn_relu_backward(gy_d, t_d, kw.pop("y"), gamma_d, mean, rstd, relu=relu, **kw)
        out[name] = OrderedDict(dt=dt, dgamma=dg, dbeta=db, dbias=dbias)
        aligned[name] = on16(gy_d, t_d, y, gamma_d, mean, rstd, dt, dg, db, dbias, beta_d, *fold)

    s_mean, s_m2 = ops.bn_stats(t_d)
    out["stats"] = OrderedDict(mean=s_mean, m2=s_m2)
    aligned["stats"] = on16(t_d, s_mean, s_m2)
    row = torch.zeros(2 * c.F + 1, dtype=torch.float32, device=device)
    r_mean, r_m2 = ops.bn_stats(t_d, row_out=row)
    out["stats_row"] = OrderedDict(mean=r_mean, m2=r_m2)
    aligned["stats_row"] = on16(t_d, r_mean, r_m2)

    dbeta, dgamma = torch.zeros(c.F, device=device), torch.zeros(c.F, device=device)
    sums = ops.bn_backward_reduce(gy_d, t_d, y, mean, rstd, relu, dbeta_out=dbeta, dgamma_out=dgamma)
    out["reduce"] = OrderedDict(sum_g=sums[0], sum_gx=sums[1], dbeta=dbeta, dgamma=dgamma)
    aligned["reduce"] = on16(gy_d, t_d, y, mean, rstd, sums[0], sums[1], dbeta, dgamma)
    a_dt, a_dbias = ops.bn_backward_apply(gy_d, t_d, y, gamma_d, mean, rstd, sums, c.n, relu)
    out["apply"] = OrderedDict(dt=a_dt, dbias=a_dbias)
    aligned["apply"] = on16(gy_d, t_d, y, gamma_d, mean, rstd, sums[0], sums[1], a_dt, a_dbias)
    return out, aligned


# the plan call and the listed form behind each entry of run_calls
PLAN_OF = {"forward_running": ("forward", lambda c: c.whole), "forward": ("forward", lambda c: c.whole),
           "backward_y": ("backward", lambda c: c.whole), "backward_beta": ("backward", lambda c: c.whole),
           "backward_fold": ("backward", lambda c: c.whole), "stats": ("stats", lambda c: c.stats),
           "stats_row": ("stats", stats_row_form), "reduce": ("reduce", lambda c: c.reduce), "apply": ("apply", lambda c: c.apply)}


def digest(tensor):
    """sha256 of the raw bytes of a tensor's values, row-major."""
    return hashlib.sha256(tensor.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def digests(outputs):
    return {name: {k: digest(v) for k, v in outs.items()} for name, outs in outputs.items()}
