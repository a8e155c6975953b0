"""The two ping-pong GEMM kernels at the smallest shapes that reach each of their paths (tests/gemm_pp_cases.py), every
output element against the CPU oracle bit for bit, with guard rows around the output and two launches back to back."""
import time

import numpy as np
import pytest
import torch

import gemm_pp_cases as pp

pytestmark = pytest.mark.gpu

GUARD = 16                           # guard rows on either side of the output
SENTINEL = 0x7FC5A5A5                # a quiet NaN no kernel produces


@pytest.fixture(scope="module")
def cus(hip):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _guarded(n, out, dev):
    buf = torch.full((n + 2 * GUARD, out), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    return buf, buf[GUARD:GUARD + n]


def _launches(trace):
    return {name: launches for name, (launches, _) in trace.items()}


@pytest.mark.parametrize("case", pp.CASES, ids=pp.case_id)
def test_pp_bit_exact(hip, oracle, cus, case):
    launches = pp.plan(case.n, case.k, case.out, cus)
    bad = pp.check_claims(case, launches)
    assert not bad, (f"on this device ({cus} CUs) the row {pp.case_id(case)} does not test what it says:\n  "
                     + "\n  ".join(bad) + f"\n  plan: {launches}")
    x, W, b, sc, sh = pp.inputs(case)
    t0 = time.perf_counter()
    want = oracle.linear(x, W, b, sc, sh, relu=case.relu, threads=8)
    t_oracle = time.perf_counter() - t0
    dev = torch.device("cuda:0")
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    dx, dW, db, dsc, dsh = t(x), t(W), t(b), t(sc), t(sh)
    bufs = [_guarded(case.n, case.out, dev) for _ in range(2)]
    torch.cuda.synchronize()
    hip.ops.trace_enable(True)
    for _, view in bufs:                 # back to back on one stream, no synchronisation in between
        y = hip.ops.linear_forward(dx, dW, db, dsc, dsh, relu=case.relu, out=view)
        assert y.data_ptr() == view.data_ptr()
    trace = hip.ops.trace_collect()
    hip.ops.trace_enable(False)
    print(f"{pp.case_id(case)}: oracle {t_oracle:.2f} s, plan on {cus} CUs {launches}, trace {trace}")
    assert _launches(trace) == pp.plan_labels(launches, repeat=2), (trace, launches)
    results = []
    for i, (buf, _) in enumerate(bufs):
        full = buf.cpu().numpy()
        got = full[GUARD:GUARD + case.n]
        results.append(got)
        where = pp.localise(got, want, launches)
        assert np.array_equal(got, want) and where is None, f"launch {i + 1} of 2, {pp.case_id(case)}:\n  {where}"
        guards = np.concatenate([full[:GUARD], full[GUARD + case.n:]]).view(np.uint32)
        assert (guards == SENTINEL).all(), \
            f"launch {i + 1} of 2 wrote outside its output: {int((guards != SENTINEL).sum())} guard elements changed, " \
            f"first at guard row {int(np.argwhere(guards != SENTINEL)[0][0])} (rows >= {GUARD} lie after the output)"
    assert np.array_equal(results[0].view(np.uint32), results[1].view(np.uint32))


def test_encode_assign_reaches_persistent_bn_kernel(hip, oracle, cus):
    """RQVAE.get_indices on a BatchNorm model: the widest encoder layer (384 -> 4096 at 2048 items) goes through
    linear_fwd_pp3_kernel<true>; latent, indices and xq against the oracle, bit for bit."""
    n, dims = 2048, [384, 4096, 256, 32]
    plans = [pp.plan(n, dims[l], dims[l + 1], cus) for l in range(3)]
    assert [(l["label"], l["form"], l["rows"]) for l in plans[0]] == [(pp.PP_LABEL, pp.PERSISTENT, n)], plans[0]
    assert all(l["label"] != pp.PP_LABEL for p in plans[1:] for l in p), plans
    rs = np.random.RandomState(2048 + 384)
    x = rs.standard_normal((n, dims[0])).astype(np.float32)
    Ws = [(rs.standard_normal((dims[l + 1], dims[l])) * np.sqrt(2.0 / (dims[l] + dims[l + 1]))).astype(np.float32) for l in range(3)]
    bs = [(0.01 * rs.standard_normal(dims[l + 1])).astype(np.float32) for l in range(3)]
    scs = [(1 + 0.1 * rs.standard_normal(dims[l + 1])).astype(np.float32) if l < 2 else None for l in range(3)]
    shs = [(0.1 * rs.standard_normal(dims[l + 1])).astype(np.float32) if l < 2 else None for l in range(3)]
    cbs = [(rs.standard_normal((64, 32)) * 0.5 ** l).astype(np.float32) for l in range(3)]
    want = oracle.encode_assign(x, Ws, bs, cbs, bn_scale=scs, bn_shift=shs, threads=8)
    dev = torch.device("cuda:0")
    t = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    flat, ks = hip.ops.flatten_codebooks([t(c) for c in cbs])
    hip.ops.trace_enable(True)
    idx, latent, xq, _ = hip.ops.encode_assign(t(x), [t(w) for w in Ws], [t(b) for b in bs], flat, ks,
                                               bn_scales=[t(s) for s in scs], bn_shifts=[t(s) for s in shs],
                                               want_latent=True, want_xq=True)
    trace = _launches(hip.ops.trace_collect())
    hip.ops.trace_enable(False)
    assert trace.get(pp.PP_LABEL) == 1, trace
    for p in plans:
        for l in p:
            assert trace.get(l["label"], 0) >= 1, (l["label"], trace)
    assert np.array_equal(latent.cpu().numpy(), want["latent"]), f"latent: max abs diff {np.abs(latent.cpu().numpy() - want['latent']).max()}"
    assert np.array_equal(idx.cpu().numpy(), want["idx"])
    assert np.array_equal(xq.cpu().numpy(), want["xq"])
