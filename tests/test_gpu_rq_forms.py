"""GPU: every row of tests/rq_cases.py once through lcrec_debug_rq_assign -- production's kernels through production's launcher, in
the form the row's plan names -- into guarded buffers, then through the judge: idx, xq, every residual, margin and near-tie word
bit for bit against the oracle, the sums of squares within rtol 1e-6, no guard row or column written.  The trace must show as many
rq_assign launches as the plan says, and rq_sse_finalize exactly when no ticket was given (whose sums must then be the ticket
form's, bit for bit).  Rows whose forced form is production's choice also go through lcrec_rq_assign: the same bits.  The host test
(tests/test_rq_plan_host.py) holds every row to its plan and every row's inputs to what the row is for."""
import numpy as np
import pytest
import torch

import rq_cases as rq

pytestmark = pytest.mark.gpu


def _run(ops, case, force, ticket):
    """The row through the library into fresh guarded buffers: (buffers as numpy, trace)."""
    dev = torch.device("cuda:0")
    z, cbs, _ = rq.inputs(case)
    flat, ks = ops.flatten_codebooks([torch.from_numpy(c).to(dev) for c in cbs])
    buf = {k: (None if v is None else torch.from_numpy(v).to(dev)) for k, v in rq.blank(case).items()}
    L = len(ks)
    ops.trace_enable(True)
    try:
        ops.rq_assign_into(torch.from_numpy(z).to(dev), flat, ks, buf["idx"], L + rq.PAD_COLS, xq=buf["xq"], xq_accumulate=case.accumulate,
                           sse=buf["sse"], resid=buf["resid"], margin=buf["margin"], neartie=buf["neartie"], tie_tau=case.tau,
                           ticket=ticket, force=force)
        torch.cuda.synchronize()
        trace = ops.trace_collect()
    finally:
        ops.trace_enable(False)
    return {k: (None if v is None else v.cpu().numpy()) for k, v in buf.items()}, trace


@pytest.mark.parametrize("case", rq.CASES, ids=rq.case_id)
def test_kernel_form_against_the_oracle(hip, case):
    ops = hip.ops
    p = rq.plan(case)
    out, trace = _run(ops, case, rq.force_of(case), case.ticket)
    want = rq.expected(case)
    L = len(case.Ks)
    with np.errstate(invalid="ignore"):
        print(f"{rq.case_id(case)}: split {p['split']}, {p['threads']} threads, grid {p['grid']}, {p['launches']} launches; trace {trace}; "
              f"idx differing {int((out['idx'] != want['idx']).sum())}, sse relative error "
              f"{np.max(np.abs(out['sse'][:L] - want['sse'][:L]) / want['sse'][:L]):.3e}")
    verdict = rq.judge(case, p, out)
    assert verdict is None, verdict
    assert trace.get(rq.TRACE_LABEL, (0,))[0] == p["launches"], trace
    assert trace.get(rq.TRACE_FINALIZE, (0,))[0] == (0 if case.ticket else p["launches"]), trace
    if not case.ticket:
        # rq_sse_finalize_kernel's sums are the ticket tail's, bit for bit
        ticketed, trace = _run(ops, case, rq.force_of(case), True)
        assert rq.TRACE_FINALIZE not in trace and trace[rq.TRACE_LABEL][0] == p["launches"], trace
        assert np.array_equal(ticketed["sse"][:L], out["sse"][:L]), (ticketed["sse"][:L], out["sse"][:L])
        assert rq.judge(case, p, ticketed) is None
    if p == rq.plan(case, (-1, 0, 0)):
        # the debug entry is production's path: lcrec_rq_assign itself leaves the same bits
        prod, trace = _run(ops, case, None, case.ticket)
        assert trace.get(rq.TRACE_LABEL, (0,))[0] == p["launches"], trace
        for name, got in out.items():
            if got is not None:
                assert np.array_equal(prod[name], got, equal_nan=got.dtype.kind == "f"), f"lcrec_rq_assign's {name} differs from the debug entry's"
