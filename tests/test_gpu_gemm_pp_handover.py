"""The tile hand-over of linear_fwd_pp3_kernel at the rows of tests/gemm_pp_handover_cases.py: every output element against
the CPU oracle bit for bit, with guard rows around the output and two launches back to back (as tests/test_gpu_gemm_pp.py),
and one row of special values -- NaN, +-inf and zero rows in the first and the last row panel, -0.0 in front of the ReLU."""
import numpy as np
import pytest
import torch

import gemm_pp_cases as pp
import gemm_pp_handover_cases as ho

pytestmark = pytest.mark.gpu

GUARD = 16                           # guard rows on either side of the output
SENTINEL = 0x7FC5A5A5                # a quiet NaN no kernel produces


@pytest.fixture(scope="module")
def cus(hip):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _run_twice_and_compare(hip, cus, case, arrays, want):
    """Two guarded launches of `case` on `arrays` back to back; each against `want` bit for bit; returns the first result."""
    launches = pp.plan(case.n, case.k, case.out, cus)
    bad = ho.check_claims(case, launches)
    assert not bad, (f"on this device ({cus} CUs) the row {pp.case_id(case)} does not test what it says:\n  "
                     + "\n  ".join(bad) + f"\n  plan: {launches}")
    dev = torch.device("cuda:0")
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    dx, dW, db, dsc, dsh = (t(a) for a in arrays)
    bufs = []
    for _ in range(2):
        buf = torch.full((case.n + 2 * GUARD, case.out), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
        bufs.append((buf, buf[GUARD:GUARD + case.n]))
    torch.cuda.synchronize()
    hip.ops.trace_enable(True)
    for _, view in bufs:                 # back to back on one stream, no synchronisation in between
        y = hip.ops.linear_forward(dx, dW, db, dsc, dsh, relu=case.relu, out=view)
        assert y.data_ptr() == view.data_ptr()
    trace = {name: count for name, (count, _) in hip.ops.trace_collect().items()}
    hip.ops.trace_enable(False)
    assert trace == pp.plan_labels(launches, repeat=2), (trace, launches)
    results = []
    for i, (buf, _) in enumerate(bufs):
        full = buf.cpu().numpy()
        got = full[GUARD:GUARD + case.n]
        results.append(got)
        where = pp.localise(got, want, launches)
        assert where is None and np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
            f"launch {i + 1} of 2, {pp.case_id(case)}:\n  {where}"
        guards = np.concatenate([full[:GUARD], full[GUARD + case.n:]]).view(np.uint32)
        assert (guards == SENTINEL).all(), \
            f"launch {i + 1} of 2 wrote outside its output: {int((guards != SENTINEL).sum())} guard elements changed"
    assert np.array_equal(results[0].view(np.uint32), results[1].view(np.uint32))
    return results[0]


@pytest.mark.parametrize("case", ho.CASES, ids=pp.case_id)
def test_handover_bit_exact(hip, oracle, cus, case):
    arrays = pp.inputs(case)
    want = oracle.linear(*arrays, relu=case.relu, threads=8)
    _run_twice_and_compare(hip, cus, case, arrays, want)


def test_special_values_bit_exact(hip, oracle, cus):
    """NaN, +inf, -inf, single-infinity and all-zero rows in the first row panel (handed over) and the last (stored by
    finish()); columns whose negative bn_scale and bn_shift = -0.0 put -0.0 in front of the ReLU.  Expected: the oracle's
    bits, (t > 0) ? t : 0 -- NaN and -0.0 become +0.0."""
    x, W, b, sc, sh, rows = ho.special_inputs()
    want = oracle.linear(x, W, b, sc, sh, relu=True, threads=8)
    got = _run_twice_and_compare(hip, cus, ho.SPECIAL, (x, W, b, sc, sh), want)
    # what the special rows must look like whatever the oracle says: no NaN and no negative zero survives the ReLU
    special = got[sorted(rows)]
    assert not np.isnan(special).any() and not (special.view(np.uint32) == 0x80000000).any()
    zero_rows = [r for r, kind in rows.items() if kind == "zero"]
    assert (got[zero_rows][:, ho.NEG_SCALE_ZERO_COLUMNS].view(np.uint32) == 0).all()
    assert np.isinf(got[[r for r, kind in rows.items() if kind.startswith("one")]]).any()
