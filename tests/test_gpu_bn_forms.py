"""GPU: every row of tests/bn_cases.py through every BatchNorm call of lcrec_amd.ops.  Per row: the library's plan gives each call
the form the row is listed for (so a later change of the dispatch rules cannot silently leave a form untested); every output
agrees with torch in fp64 on the CPU, to the tolerances of tests/test_gpu_train.py (so the fixture cannot pin wrong values); the
three sources of the backward's ReLU mask give the same bits; and every output has the bytes recorded in
tests/golden/f12_bn_forms.json by tools/record_bn_forms.py, before the dword kernels were folded into two."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_cases as bn

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLD, "f12_bn_forms.json")) as fh:
        return json.load(fh)


def check_fp64(c, relu, out):
    """The outputs of bn_cases.run_calls against nn.BatchNorm1d (+ ReLU) and autograd in fp64 on the CPU."""
    t, gamma, beta, rm, rv, gy = bn.inputs(c)
    n = c.n
    td = torch.from_numpy(t).double().requires_grad_(True)
    gd, bd = torch.from_numpy(gamma).double().requires_grad_(True), torch.from_numpy(beta).double().requires_grad_(True)
    rmd, rvd = torch.from_numpy(rm).double(), torch.from_numpy(rv).double()
    yd = F.batch_norm(td, rmd, rvd, gd, bd, training=True, momentum=bn.MOMENTUM, eps=bn.EPS)
    if relu:
        yd = F.relu(yd)
    yd.backward(torch.from_numpy(gy).double())
    mean64, var64 = t.astype(np.float64).mean(0), t.astype(np.float64).var(0)
    scale = float(np.abs(td.grad.numpy()).max())
    h = lambda x: x.cpu().numpy()
    for name in ("forward_running", "forward"):
        o = out[name]
        np.testing.assert_allclose(h(o["y"]), yd.detach().numpy(), rtol=1e-5, atol=1e-5, err_msg=name)
        np.testing.assert_allclose(h(o["mean"]), mean64, rtol=1e-6, atol=3e-6, err_msg=name)
        np.testing.assert_allclose(h(o["rstd"]), 1 / np.sqrt(var64 + bn.EPS), rtol=1e-5, err_msg=name)
    np.testing.assert_allclose(h(out["forward_running"]["running_mean"]), rmd.numpy(), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(h(out["forward_running"]["running_var"]), rvd.numpy(), rtol=1e-5, atol=1e-6)
    for name in ("backward_y", "backward_beta", "backward_fold"):
        o = out[name]
        np.testing.assert_allclose(h(o["dt"]), td.grad.numpy(), rtol=1e-4, atol=2e-6 * max(scale, 1.0), err_msg=name)
        np.testing.assert_allclose(h(o["dgamma"]), gd.grad.numpy(), rtol=1e-5, atol=1e-4, err_msg=name)
        np.testing.assert_allclose(h(o["dbeta"]), bd.grad.numpy(), rtol=1e-5, atol=1e-4, err_msg=name)
        # the Linear bias in front of a BatchNorm has gradient sum(dt) = 0 up to rounding
        assert float(o["dbias"].abs().max()) <= 1e-5 * n * max(scale, 1.0), name
    for name in ("stats", "stats_row"):
        o = out[name]
        np.testing.assert_allclose(h(o["mean"]), mean64, rtol=1e-6, atol=3e-6, err_msg=name)
        np.testing.assert_allclose(1 / np.sqrt(h(o["m2"]).astype(np.float64) / n + bn.EPS), 1 / np.sqrt(var64 + bn.EPS), rtol=1e-5, err_msg=name)
    o = out["reduce"]
    np.testing.assert_allclose(h(o["sum_gx"]), gd.grad.numpy(), rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(h(o["sum_g"]), bd.grad.numpy(), rtol=1e-5, atol=1e-4)
    assert torch.equal(o["sum_g"], o["dbeta"]) and torch.equal(o["sum_gx"], o["dgamma"])
    o = out["apply"]
    np.testing.assert_allclose(h(o["dt"]), td.grad.numpy(), rtol=1e-4, atol=2e-6 * max(scale, 1.0))
    np.testing.assert_allclose(h(o["dbias"]), h(o["dt"].double().sum(0)), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("run", bn.runs(), ids=bn.run_id)
def test_bn_form(hip, recorded, run):
    c, relu = run
    out, aligned = bn.run_calls(hip.ops, c, relu, torch.device(DEV))
    for name, (call, listed) in bn.PLAN_OF.items():
        plan = hip.ops.bn_plan(call, c.n, c.F, aligned[name])
        assert bn.Form(**plan) == listed(c), f"{bn.run_id(run)} {name}: listed for {c.why!r}"
    check_fp64(c, relu, out)
    for other in ("backward_beta", "backward_fold"):
        for key, value in out["backward_y"].items():
            assert torch.equal(out[other][key], value), f"{other} {key}: the mask sources differ"
    got, want = bn.digests(out), recorded["cases"][bn.run_id(run)]
    assert sorted(got) == sorted(want)
    for name in got:
        assert got[name] == want[name], f"{bn.run_id(run)} {name}: not the recorded bits ({recorded['commit'][:12]}, {recorded['device']})"
