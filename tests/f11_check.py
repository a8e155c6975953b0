"""Judging an fp32 evaluation of the run.sh-width training step against fixture F11 (oracle/make_golden.py
fixture_run_sh_step): the imported reference's gradients in fp64 are the yardstick, the reference's own fp32 run says how
far from it fp32 arithmetic lands, tensor by tensor.  Shared by the CPU test (the oracle's torch restatement) and the GPU
tests (engine, autograd path).

The codes are judged too (judge below).  A path may assign up to 3 of the 1024 rows differently from the fixture, and every
code it assigns, on every row and level, must be ACCEPTABLE by tests/step_check.py's rule: with C64 and C32 the level's cost
matrix (the distances on an argmin level, -ln Q on the Sinkhorn level) of the oracle's torch restatement in fp64 and in
fp32, both with the path's codes forced, b_i the fp64 minimum of row i and D = |C32 - C64|,

    C64[i, k] - C64[i, b_i]  <=  SLACK * (D[i, k] + D[i, b_i]) + floor(i, k)

with floor = 2^-22 * (||R64_i||^2 + ||c_k||^2) on an argmin level and 1e-9 on the Sinkhorn level.  So the rows that differ
are near-ties of the fp64 evaluation, not wrong assignments."""
import numpy as np

import golden_inputs as gi

SLACK = 4.0          # an fp32 path may sit this many times further from fp64 than the reference's own fp32 run does ...
FLOOR = 2e-6         # ... where that distance is at least a few fp32 ulps of accumulated rounding
NOISE = 16.0         # tensors whose true gradient is zero (a Linear bias in front of BatchNorm): rounding noise, bounded by
                     # this multiple of the reference's own noise


def tensors(g):
    return [f[len("f64__sample__"):] for f in g.files if f.startswith("f64__sample__")]


def report(g, grads, f64=None):
    """grads: parameter name -> full gradient array of the path under test.  Returns rows
    (name, kind, path_err, ref_err, bound) and the list of violations.  `f64`: full fp64 gradients to judge against
    instead of the fixture's (f64_gradients_for below, when the path assigned a near-tied row to another code); the
    reference's fp32-vs-fp64 distance stays the fixture's -- it measures the arithmetic, not the assignment."""
    rows, bad = [], []
    for k in tensors(g):
        s64 = (g["f64__sample__" + k] if f64 is None else gi.strided_sample(np.asarray(f64[k]))).astype(np.float64)
        s32 = g["f32__sample__" + k].astype(np.float64)
        sp = gi.strided_sample(np.asarray(grads[k])).astype(np.float64)
        assert sp.shape == s64.shape, (k, sp.shape, s64.shape)
        n64, n32 = np.linalg.norm(s64), np.linalg.norm(s32)
        if n64 < 1e-6 * n32:                      # the true gradient is zero; the fp32 values are pure rounding noise
            path, ref, bound, kind = np.linalg.norm(sp), n32, NOISE * n32, "noise"
        else:
            path, ref = np.linalg.norm(sp - s64) / n64, np.linalg.norm(s32 - s64) / n64
            bound, kind = SLACK * max(ref, FLOOR), "rel"
        rows.append((k, kind, path, ref, bound))
        if not path <= bound:
            bad.append((k, kind, path, ref, bound))
    return rows, bad


_YARDSTICKS = {}


def problem(g):
    """(torch_ref.Spec, state dict name -> array with the fixture's codebooks, batch) of the run.sh step."""
    from oracle import torch_ref
    sd, x = gi.run_sh_train_case()
    for l in range(4):
        sd[f"rq.vq_layers.{l}.embedding.weight"] = g["codebooks"][l].copy()
    spec = torch_ref.Spec(768, [256] * 4, 32, gi.RUN_SH_LAYERS, bn=True, sk_epsilons=[0.0, 0.0, 0.0, 0.003], sk_iters=50)
    return spec, sd, x


def f64_gradients_for(g, idx, costs=None):
    """The run.sh step in fp64 with the codes FORCED to `idx` [1024, 4] (oracle/torch_ref.py, checked against the fixture's
    fp64 values with the fixture's own codes by tests/test_oracle_golden.py): ([loss, recon, rq_loss, grad norm], name ->
    gradient).  A path whose latents differ in the last bit may send a near-tied row of the Sinkhorn level to another code --
    a different problem for that row, not different arithmetic; this evaluates that problem exactly.  `costs`: see
    step_check.evaluate."""
    import torch
    import step_check
    return step_check.evaluate(*problem(g), idx, torch.float64, costs=costs)


def yardsticks(g, idx):
    """Both forced evaluations of the run.sh step for the codes `idx`, made once per set of codes: (fp64 scalars, fp64
    gradients, fp32 scalars, fp32 gradients, step_check.CodeRule of the two)."""
    import torch
    import step_check
    key = np.asarray(idx).astype(np.int64).tobytes()
    if key not in _YARDSTICKS:
        while len(_YARDSTICKS) >= 4:                             # (full gradients of 4.3 M parameters each: keep a few)
            _YARDSTICKS.pop(next(iter(_YARDSTICKS)))
        spec, sd, x = problem(g)
        c64, c32 = [], []
        s64, g64 = f64_gradients_for(g, idx, c64)
        s32, g32 = step_check.evaluate(spec, sd, x, idx, torch.float32, costs=c32)
        _YARDSTICKS[key] = (s64, g64, s32, g32, step_check.CodeRule(spec, c64, c32))
    return _YARDSTICKS[key]


def judge(g, grads, scalars, idx, what):
    """One evaluation of the run.sh step -- its full gradients, [loss, recon, rq_loss, gradient norm before clipping] and
    codes [1024, 4] -- against the fixture.  At most 3 rows may carry other codes than the fixture's, and EVERY code has to
    be acceptable by its fp64 regret (step_check.CodeRule: the cost matrices of the oracle's torch restatement in fp64 and
    in fp32 with the codes forced to `idx`), so a row that differs is a near-tie of the fp64 evaluation and not a wrong
    assignment.  With other codes the yardstick is the fp64 evaluation of THAT problem (f64_gradients_for) -- same bounds."""
    idx = np.asarray(idx).astype(np.int64)
    flipped = int((idx != g["idx"].astype(np.int64)).any(1).sum())
    assert flipped <= 3, (what, flipped)
    s64, g64, _, _, rule = yardsticks(g, idx)
    rule.check(idx, what)
    target, f64 = (s64, g64) if flipped else (g["f64__scalars"], None)
    np.testing.assert_allclose(scalars[:3], target[:3], rtol=1e-5, err_msg=what)      # loss, recon, rq_loss
    np.testing.assert_allclose(scalars[3], target[3], rtol=1e-4, err_msg=what)        # gradient norm before clipping
    rows, bad = report(g, grads, f64)
    print(f"\n[{what}] rows assigned differently: {flipped}\n" + table(rows))
    assert not bad, what + "\n" + table(bad)
    return rows


def table(rows):
    return "\n".join(f"{k:40s} {kind:5s} path {p:.3e}  reference-fp32 {r:.3e}  bound {b:.3e}" for k, kind, p, r, b in rows)
