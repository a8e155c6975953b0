"""GPU: every row of tests/sinkhorn_group_cases.py through lcrec_debug_sinkhorn_groups -- lcrec_sinkhorn_assign's launch code and
kernels, plus runner-up and second / best -- and then through lcrec_sinkhorn_assign itself: every row of every group has the fp64
reference's winner and runner-up, second / best within the group's measured tolerance (exactly 1.0 where the reference's is), the
guard columns and the rows of no group are untouched, both entries give the same winners, and the launches carry the trace labels
the plan names.  No row is excluded or tolerated: tests/test_sinkhorn_groups_plan_host.py holds every row's inputs to the stability
condition under the reference alone."""
import ctypes

import numpy as np
import pytest
import torch

import sinkhorn_group_cases as gc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _upload(case):
    z, cb = gc.inputs(case)
    return torch.from_numpy(z).to(DEV), torch.from_numpy(cb).to(DEV)


def _outputs(case):
    n = gc.rows(case)
    return (torch.full((n, case.stride), -1, dtype=torch.int64, device=DEV), torch.full((n,), -1, dtype=torch.int64, device=DEV),
            torch.full((n,), float("nan"), dtype=torch.float64, device=DEV))


def _debug(ops, case, zt, cbt):
    """The row through lcrec_debug_sinkhorn_groups; nothing is waited for.  -> (guard [n, stride], runner [n], ratio [n])"""
    guard, runner, ratio = _outputs(case)
    ops.sinkhorn_groups_debug(zt, cbt, case.eps, case.iters, gc.offsets(case), out=guard[:, 0], runner_out=runner, ratio_out=ratio,
                              context=case.context)
    return guard, runner, ratio


def _assign(ops, case, zt, cbt):
    """The row through lcrec_sinkhorn_assign by the C ABI, with the row's context or NULL.  -> guard [n, stride]"""
    lib = ops._lib.load()
    guard = torch.full((gc.rows(case), case.stride), -1, dtype=torch.int64, device=DEV)
    offs = gc.offsets(case)
    oarr = offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    n, G = gc.rows(case), len(case.sizes)
    dev = zt.device
    with ops._on(dev):
        ws = ops._workspace(lib.lcrec_sinkhorn_assign_workspace(n, case.K, oarr, G), dev)
        rc = lib.lcrec_sinkhorn_assign(ops._ptr(zt), n, case.e, ops._ptr(cbt), case.K, oarr, G, float(case.eps), int(case.iters),
                                       ops._ptr(guard), case.stride, ops._ptr(ws), ws.numel(), ops._context(dev) if case.context else None,
                                       ops._ptr(ops._ticket(dev)), ops._stream_ptr())
    ops._lib.check(rc, "lcrec_sinkhorn_assign")
    return guard


def _verdict(case, guard, runner, ratio):
    got = guard.cpu().numpy()
    assert (got[:, 1:] == -1).all(), f"{gc.case_id(case)}: the solver wrote between the strided outputs"
    winner, runner, ratio = got[:, 0].copy(), runner.cpu().numpy(), ratio.cpu().numpy()
    ref = gc.reference(case)
    m = ref.grouped
    with np.errstate(invalid="ignore"):
        print(f"{gc.case_id(case)}: winners differing {int((winner != ref.winner)[m].sum())}, runner-ups differing "
              f"{int((runner != ref.runner)[m].sum())}, second / best off by {np.nanmax((np.abs(ratio - ref.ratio) / ref.ratio)[m]):.3e} "
              f"({int(np.isnan(ratio[m]).sum())} not written), tolerances {np.nanmin(ref.tol):.3e} .. {np.nanmax(ref.tol):.3e}, "
              f"exactly 1.0 on {int((ratio[m] == 1.0).sum())} rows, asked on {int(ref.exact_one.sum())}")
    return winner, gc.judge(case, winner, runner, ratio)


def _labels(p):
    want = {}
    for c in p["cls"]:
        if c["groups"]:
            want[c["label"]] = want.get(c["label"], 0) + 1
    if p["batch_groups"]:
        want["sinkhorn"] = p["batch_groups"]
    return want


@pytest.mark.parametrize("case", gc.CASES, ids=gc.case_id)
def test_grouped_solve_against_the_reference(hip, case):
    ops = hip.ops
    p = gc.plan(case)
    zt, cbt = _upload(case)
    ops.trace_enable(True)
    try:
        guard, runner, ratio = _debug(ops, case, zt, cbt)
        torch.cuda.synchronize()
        trace = ops.trace_collect()
    finally:
        ops.trace_enable(False)
    winner, verdict = _verdict(case, guard, runner, ratio)
    assert verdict is None, verdict
    names = ("sinkhorn", "sinkhorn_tiny", "sinkhorn_small", "sinkhorn_slab")
    assert {k: v[0] for k, v in trace.items() if k in names} == _labels(p), (trace, p)

    # the debug entry is production's path: lcrec_sinkhorn_assign gives the same winners by the same launches
    ops.trace_enable(True)
    try:
        assigned = _assign(ops, case, zt, cbt)
        torch.cuda.synchronize()
        trace = ops.trace_collect()
    finally:
        ops.trace_enable(False)
    got = assigned.cpu().numpy()
    assert (got[:, 1:] == -1).all(), "lcrec_sinkhorn_assign wrote between the strided outputs"
    assert np.array_equal(got[:, 0], winner), f"{int((got[:, 0] != winner).sum())} rows of lcrec_sinkhorn_assign differ from the debug entry"
    assert {k: v[0] for k, v in trace.items() if k in names} == _labels(p), (trace, p)


def test_the_same_sizes_with_and_without_a_context_give_identical_winners(hip):
    ops = hip.ops
    key = lambda c: c._replace(context=True, expect={}, covers=())
    pairs = [(a, b) for a in gc.CASES for b in gc.CASES if a.context and not b.context and key(a) == key(b)]
    assert len(pairs) >= 2
    for a, b in pairs:
        zt, cbt = _upload(a)
        one, two = _assign(ops, a, zt, cbt), _assign(ops, b, zt, cbt)
        assert torch.equal(one, two), gc.case_id(a)


def test_six_calls_back_to_back_reuse_the_ring(hip):
    """Six calls with different group tables and no synchronisation between them: the context's pinned ring has four slots, so
    the fifth and sixth upload reuse the first and second slot while the device may still be behind.  Every call is judged."""
    ops = hip.ops
    cases = [gc.CASES[i] for i in gc.BACK_TO_BACK]
    data = [_upload(c) for c in cases]
    for c in cases:
        gc.reference(c)                                              # (the references first: nothing on the host between the calls)
    torch.cuda.synchronize()
    results = [_debug(ops, c, zt, cbt) for c, (zt, cbt) in zip(cases, data)]
    torch.cuda.synchronize()
    for c, (guard, runner, ratio) in zip(cases, results):
        _winner, verdict = _verdict(c, guard, runner, ratio)
        assert verdict is None, verdict
