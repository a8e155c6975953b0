"""GPU: every row of tests/sinkhorn_cases.py through lcrec_debug_sinkhorn_batch -- production's kernels, the solver the row's plan
names -- against the longdouble yardstick: the form that ran, every row's winner, every row's runner-up, and second / best within
the measured tolerance (sinkhorn_cases.tolerance).  Then lcrec_sinkhorn_assign on the same inputs: the same winners, and for the
rows that stand for production's choice the batch-sized solver's trace label.  No row of any problem is excluded: the host test
(tests/test_sinkhorn_plan_host.py) holds every row's inputs to margins under the reference alone."""
import numpy as np
import pytest
import torch

import sinkhorn_cases as sk

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", sk.CASES, ids=sk.case_id)
def test_solver_form_against_the_yardstick(hip, case):
    ops = hip.ops
    p = sk.plan(case)
    z, cb = sk.inputs(case)
    dev = torch.device("cuda:0")
    zt, cbt = torch.from_numpy(z).to(dev), torch.from_numpy(cb).to(dev)
    guard = torch.full((case.B, case.stride), -1, dtype=torch.int64, device=dev)
    runner = torch.full((case.B,), -1, dtype=torch.int64, device=dev)
    ratio = torch.full((case.B,), float("nan"), dtype=torch.float64, device=dev)
    # (a launch the runtime refuses raises here: a failure, not a skip)
    _, _, _, ran = ops.sinkhorn_debug(zt, cbt, case.eps, case.iters, form=case.form, out=guard[:, 0], runner_out=runner, ratio_out=ratio)
    torch.cuda.synchronize()
    assert ran == p["form"], f"{sk.case_id(case)}: {sk.FORM_NAMES.get(ran, ran)} ran, the plan says {sk.FORM_NAMES[p['form']]}"
    got = guard.cpu().numpy()
    assert (got[:, 1:] == -1).all(), "the solver wrote between the strided outputs"
    winner, runner, ratio = got[:, 0].copy(), runner.cpu().numpy(), ratio.cpu().numpy()
    y = sk.reference(case).yardstick
    with np.errstate(invalid="ignore"):
        print(f"{sk.case_id(case)}: form {ran}; winners differing {int((winner != y.winner).sum())}, runner-ups differing "
              f"{int((runner != y.runner).sum())}, second / best off by {np.nanmax(np.abs(ratio - y.ratio) / y.ratio):.3e} "
              f"({int(np.isnan(ratio).sum())} not written), tolerance {sk.tolerance(case):.3e}")
    verdict = sk.judge(case, p, winner, runner, ratio)
    assert verdict is None, verdict

    # the debug entry is production's path: lcrec_sinkhorn_assign gives the same winners, by the batch-sized solver
    ops.trace_enable(True)
    try:
        assigned = ops.sinkhorn_assign(zt, cbt, case.eps, case.iters).cpu().numpy()
        trace = ops.trace_collect()
    finally:
        ops.trace_enable(False)
    assert np.array_equal(assigned, winner), f"{int((assigned != winner).sum())} rows of lcrec_sinkhorn_assign differ from the debug entry"
    if case.form == sk.AUTO:
        assert sk.TRACE_LABEL in trace and not ({"sinkhorn_small", "sinkhorn_slab", "sinkhorn_tiny"} & set(trace)), trace
