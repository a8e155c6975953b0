"""Every form of the generic GEMM kernels, the 32 x 64 kernel, the grouped weight-gradient kernel and the split-K reducers at the
smallest shapes that reach it (tests/gemm_cases.py): every output element against the CPU oracle bit for bit, outputs and split-K
workspaces between sentinel guard rows, operands exactly sized, two calls back to back into two buffers, trace labels against the
plan, tickets back at zero; the training forward's statistics against float64 within the bound derived in the case file."""
import ctypes
import time

import numpy as np
import pytest
import torch

import gemm_cases as gc

pytestmark = pytest.mark.gpu

GUARD = 16                           # guard rows on either side of an output
SENTINEL = 0x7FC5A5A5                # a quiet NaN no kernel produces
DEV = "cuda:0"


@pytest.fixture(scope="module")
def cus(hip):
    return torch.cuda.get_device_properties(0).multi_processor_count


class Guarded:
    """A float32 [rows][cols] device buffer between GUARD sentinel rows on either side; the view is 16-byte aligned (cols % 4
    == 0, or the guard rows hold a multiple of four floats)."""
    def __init__(self, rows, cols):
        self.rows = rows
        self.buf = torch.full((rows + 2 * GUARD, cols), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
        self.view = self.buf[GUARD:GUARD + rows]
        assert self.view.data_ptr() % 16 == 0

    def read(self, what):
        full = self.buf.cpu().numpy()
        guards = np.concatenate([full[:GUARD], full[GUARD + self.rows:]]).view(np.uint32)
        assert (guards == SENTINEL).all(), (f"{what}: written outside the buffer: {int((guards != SENTINEL).sum())} guard elements changed, "
                                            f"first at guard row {int(np.argwhere(guards != SENTINEL)[0][0])} (rows >= {GUARD} lie after it)")
        return full[GUARD:GUARD + self.rows]


def _d(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _labels(launches, repeat=2):
    """{trace label: count}: a reducer runs inside its product's bracket, a grouped launch is one bracket"""
    out = {}
    seen_group = False
    for l in launches:
        if l["family"] == "reducer" or (l["grouped"] and seen_group):
            continue
        seen_group = seen_group or l["grouped"]
        out[l["label"]] = out.get(l["label"], 0) + repeat
    return out


def _trace(hip):
    return {name: launches for name, (launches, _) in hip.ops.trace_collect().items()}


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _check(got, want, l, what, run=None, nan_ok=False):
    if nan_ok:                                            # same NaN mask, same bits elsewhere
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN masks differ at {np.argwhere(np.isnan(got) != np.isnan(want))[:4].tolist()}"
        got, want = np.where(np.isnan(want), np.float32(0), got), np.where(np.isnan(want), np.float32(0), want)
    where = gc.localise(got, want, l, run)
    assert where is None, f"{what}:\n  {where}"


def _stream(hip):
    return hip.ops._stream_ptr()


@pytest.fixture
def planned(hip, cus, request):
    def plan(row):
        launches = gc.launches_of(row, hip.ops, cus)
        bad = gc.check_claims(row, launches)
        assert not bad, f"on this device ({cus} CUs) the row {gc.row_id(row)} does not test what it says:\n  " + "\n  ".join(bad) + f"\n  plan: {launches}"
        return launches
    return plan


ROWS = {k: [r for r in gc.ROWS if r.kind == k] for k in ("fwd", "bwd", "grp", "train")}


@pytest.mark.parametrize("row", ROWS["fwd"], ids=gc.row_id)
def test_forward_forms_bit_exact(hip, oracle, planned, row):
    launches = planned(row)
    n, k, out = row.dims
    x, W, b, sc, sh = gc.fwd_inputs(row)
    t0 = time.perf_counter()
    want = oracle.linear(x, W, b, sc, sh, relu=row.opt["relu"], threads=8)
    t_oracle = time.perf_counter() - t0
    dx, dW, db, dsc, dsh = _d(x), _d(W), _d(b), _d(sc), _d(sh)
    bufs = [Guarded(n, out) for _ in range(2)]             # (odd widths too: sixteen guard rows are a multiple of 16 bytes)
    torch.cuda.synchronize()
    hip.ops.trace_enable(True)
    for g in bufs:                                         # back to back on one stream, no synchronisation in between
        hip.ops.linear_forward(dx, dW, db, dsc, dsh, relu=row.opt["relu"], out=g.view)
    trace = _trace(hip)
    hip.ops.trace_enable(False)
    print(f"{gc.row_id(row)}: oracle {t_oracle:.2f} s, forms {[gc.form_of(l) for l in launches]}, trace {trace}")
    assert trace == _labels(launches), (trace, launches)
    got = [g.read(f"call {i + 1} of 2") for i, g in enumerate(bufs)]
    for i, y in enumerate(got):
        _check(y, want, launches[-1], f"call {i + 1} of 2, {gc.row_id(row)}", nan_ok=row.opt["inf"])
    assert _same(got[0], got[1])
    if row.opt["inf"]:
        assert np.isinf(want[n - 1]).any() or np.isnan(want[n - 1]).any()
        assert np.isfinite(want[:n - 1]).all()            # the inf stays in its own row: padding below it read zeros, not inf * 0


def _backward_call(lib, hip, gy, x, W, n, i, o, gx, gw, ws):
    rc = lib.lcrec_linear_backward(_p(gy), _p(x), _p(W), n, i, o, _p(gx), _p(gw), _p(ws), 0 if ws is None else ws.numel() * 4, _stream(hip))
    hip._lib.check(rc, "lcrec_linear_backward")


@pytest.mark.parametrize("row", ROWS["bwd"], ids=gc.row_id)
def test_backward_forms_bit_exact(hip, oracle, planned, row):
    launches = planned(row)
    lib = hip._lib.load()
    n, i, o = row.dims
    gy, x, W = gc.bwd_inputs(row)
    dw = next((l for l in launches if l["role"] == "dw"), None)
    S = dw["runs"] if dw else 1
    t0 = time.perf_counter()
    want_gx = oracle.linear(gy, np.ascontiguousarray(W.T), threads=8) if row.opt["gx"] else None
    per = (dw["k_tiles_per_run"] * 32) if dw else n
    parts = []
    if row.opt["gw"]:
        for lo in range(0, n, per):
            parts.append(oracle.linear(np.ascontiguousarray(gy[lo:lo + per].T), np.ascontiguousarray(x[lo:lo + per].T), threads=8))
        want_gw = parts[0]
        for part in parts[1:]:
            want_gw = (want_gw + part).astype(np.float32)
        assert len(parts) == S
        if not row.opt["inf"] and n * i * o < 2 ** 24:
            assert _same(want_gw, oracle.linear_backward(gy, x, W, splits=S)[1])       # the same reference as the older tests'
    t_oracle = time.perf_counter() - t0
    dgy, dx, dW = _d(gy), _d(x), _d(W)
    calls = []
    for _ in range(2):
        calls.append((Guarded(n, i) if row.opt["gx"] else None, Guarded(o, i) if row.opt["gw"] else None,
                      Guarded(S * o, i) if S > 1 else None))
    torch.cuda.synchronize()
    hip.ops.trace_enable(True)
    for gx, gw, ws in calls:
        _backward_call(lib, hip, dgy, dx, dW, n, i, o, gx and gx.view, gw and gw.view, ws and ws.view)
    trace = _trace(hip)
    hip.ops.trace_enable(False)
    print(f"{gc.row_id(row)}: oracle {t_oracle:.2f} s, forms {[gc.form_of(l) for l in launches]}, S {S}, trace {trace}")
    assert trace == _labels(launches), (trace, launches)
    results = []
    for c, (gx, gw, ws) in enumerate(calls):
        what = f"call {c + 1} of 2, {gc.row_id(row)}"
        res = []
        if gx is not None:
            res.append(gx.read(what + " gx"))
            _check(res[-1], want_gx, launches[0], what + " gx")
        if ws is not None:                                # the K-runs' partial products, each against its own chain
            partial = ws.read(what + " workspace")
            res.append(partial)
            for s in range(S):
                _check(partial[s * o:(s + 1) * o], parts[s], dw, what + f" partial product {s}", run=s, nan_ok=row.opt["inf"])
        if gw is not None:
            res.append(gw.read(what + " gw"))
            _check(res[-1], want_gw, launches[-1] if S > 1 else dw, what + " gw", nan_ok=row.opt["inf"])
        results.append(res)
    assert all(_same(a, b) for a, b in zip(*results))
    if row.opt["inf"]:
        assert np.isinf(want_gw[:, i // 2]).all() and np.isfinite(np.delete(want_gw, i // 2, axis=1)).all()


@pytest.mark.parametrize("row", ROWS["grp"], ids=gc.row_id)
def test_grouped_weight_gradients_bit_exact(hip, oracle, planned, row):
    """Against the oracle directly (not against per-layer calls): every problem's gradient is the ordered sum of its planned
    K-runs' chains over the folded input; the shared workspace sits between guards too."""
    launches = planned(row)
    lib = hip._lib.load()
    count = len(row.dims)
    products = launches[:count]
    data = gc.grp_inputs(row)
    t0 = time.perf_counter()
    wants = []
    for (n, i, o, fold, _), (gy, x, f), l in zip(row.dims, data, products):
        u = x if f is None else oracle.affine_relu(x, f[0], f[1], relu=fold == "relu")
        wants.append(oracle.linear_backward(gy, u, np.zeros((o, i), np.float32), splits=l["runs"], threads=4)[1])
        assert l["k_tiles_per_run"] == -(-(-(-n // 32)) // l["runs"])
    t_oracle = time.perf_counter() - t0
    dev = [(_d(gy), _d(x), None if f is None else (_d(f[0]), _d(f[1]))) for gy, x, f in data]
    arr = (hip._lib.DwProblem * count)()
    nbytes = None
    calls = []
    for _ in range(2):
        outs = [Guarded(o, i) for _, i, o, _, _ in row.dims]
        for p, ((n, i, o, fold, s), (gy, x, f), g) in enumerate(zip(row.dims, dev, outs)):
            arr[p] = hip._lib.DwProblem(gy.data_ptr(), x.data_ptr(), g.view.data_ptr(), n, i, o, f and f[0].data_ptr(), f and f[1].data_ptr(),
                                        int(fold == "relu"), s)
        if nbytes is None:
            nbytes = lib.lcrec_linear_backward_weights_workspace(ctypes.cast(arr, ctypes.c_void_p), count)
            assert nbytes % 256 == 0 and nbytes > 0
        ws = Guarded(nbytes // 256, 64)
        calls.append((outs, ws, bytes(arr)))
    torch.cuda.synchronize()
    hip.ops.trace_enable(True)
    for outs, ws, raw in calls:
        ctypes.memmove(arr, raw, len(raw))
        rc = lib.lcrec_linear_backward_weights(ctypes.cast(arr, ctypes.c_void_p), count, _p(ws.view), nbytes, _stream(hip))
        hip._lib.check(rc, "lcrec_linear_backward_weights")
    trace = _trace(hip)
    hip.ops.trace_enable(False)
    print(f"{gc.row_id(row)}: oracle {t_oracle:.2f} s, grids {launches[0]['grids']}, S {[l['runs'] for l in products]}, trace {trace}")
    assert trace == _labels(launches), (trace, launches)
    got = []
    for c, (outs, ws, _) in enumerate(calls):
        ws.read(f"call {c + 1} of 2 workspace")
        got.append([g.read(f"call {c + 1} of 2 problem {p}") for p, g in enumerate(outs)])
        for p, (y, want, l) in enumerate(zip(got[-1], wants, products)):
            _check(y, want, l, f"call {c + 1} of 2, problem {p} {row.dims[p]}", nan_ok=row.dims[p][3] == "inf")
            if row.dims[p][3] == "inf":
                i0 = row.dims[p][1] // 2
                assert (want[:, i0] == np.inf).all() and np.isfinite(np.delete(want, i0, axis=1)).all()
    assert all(_same(a, b) for a, b in zip(*got))


@pytest.mark.parametrize("row", ROWS["train"], ids=gc.row_id)
def test_training_forward_forms(hip, oracle, planned, row):
    launches = planned(row)
    l = launches[0]
    lib = hip._lib.load()
    n, k, out = row.dims
    o = row.opt
    x, sc, sh, W, b, gamma, beta, rm0, rv0 = gc.train_inputs(row)
    if not o["affine"]:
        gamma = beta = None
    if not o["running"]:
        rm0 = rv0 = None
    t0 = time.perf_counter()
    u = oracle.affine_relu(x, sc, sh, relu=o["in_relu"]) if o["pro"] else x
    want = oracle.linear(u, W, b, threads=8)
    ref = gc.stats_reference(want, l["tile_rows"]) if o["stats"] else None
    t_oracle = time.perf_counter() - t0
    dx, dW, db = _d(x), _d(W), _d(b)
    dsc, dsh = (_d(sc), _d(sh)) if o["pro"] else (None, None)
    dg, dbe = _d(gamma), _d(beta)
    nws = lib.lcrec_linear_bn_forward_workspace(n, out)
    assert nws == -(-n // l["tile_rows"]) * 3 * out * 4
    tickets = torch.zeros(64 + 16, dtype=torch.int32, device=DEV)
    calls = []
    for _ in range(2):
        calls.append(dict(t=Guarded(n, out), st=Guarded(4, out) if o["stats"] else None, ws=Guarded(nws // (4 * out), out) if o["stats"] else None,
                          rm=_d(rm0), rv=_d(rv0)))
    torch.cuda.synchronize()
    hip.ops.trace_enable(True)
    for c in calls:
        st = c["st"]
        row_ptr = lambda r: None if st is None else ctypes.c_void_p(st.view[r].data_ptr())
        rc = lib.lcrec_linear_bn_forward(_p(dx), n, k, _p(dsc), _p(dsh), int(o["in_relu"]), _p(dW), _p(db), out, _p(c["t"].view), int(o["stats"]),
                                         _p(dg), _p(dbe), gc.TRAIN_EPS, gc.TRAIN_MOMENTUM, _p(c["rm"]), _p(c["rv"]), row_ptr(0), row_ptr(1),
                                         row_ptr(2), row_ptr(3), None if c["ws"] is None else _p(c["ws"].view), nws if o["stats"] else 0,
                                         ctypes.c_void_p(tickets.data_ptr() + 64), _stream(hip))
        hip._lib.check(rc, "lcrec_linear_bn_forward")
    trace = _trace(hip)
    hip.ops.trace_enable(False)
    print(f"{gc.row_id(row)}: oracle {t_oracle:.2f} s, form {gc.form_of(l)}, chunks {l['chunks']} of {l['chunk_row_tiles']} row tiles, trace {trace}")
    assert trace == _labels(launches), (trace, launches)
    assert int(tickets.abs().sum()) == 0                   # every strip's ticket is back at zero
    got = []
    for i, c in enumerate(calls):
        what = f"call {i + 1} of 2, {gc.row_id(row)}"
        t = c["t"].read(what + " t")
        _check(t, want, l, what)
        res = [t]
        if o["stats"]:
            c["ws"].read(what + " workspace")
            st = c["st"].read(what + " statistics")
            mean, rstd, scale, shift = st
            print(f"  {what}: |mean - float64| / bound max {np.max(np.abs(mean - ref['mean']) / np.maximum(ref['mean_tol'], 1e-300)):.3f}; "
                  f"adversarial columns: mean {mean[:4]}, rstd {rstd[:4]} in {ref['rstd_lo'][:4]} .. {ref['rstd_hi'][:4]}")
            assert (np.abs(mean - ref["mean"]) <= ref["mean_tol"]).all(), np.argwhere(np.abs(mean - ref["mean"]) > ref["mean_tol"])[:4]
            assert ((rstd >= ref["rstd_lo"]) & (rstd <= ref["rstd_hi"])).all(), np.argwhere((rstd < ref["rstd_lo"]) | (rstd > ref["rstd_hi"]))[:4]
            exact_rstd = np.float32(1) / np.sqrt(np.float32(gc.TRAIN_EPS))
            assert mean[1] == gc.CONST_SHORT and rstd[1] == exact_rstd          # a constant column: the constant, 1 / sqrtf(eps)
            assert rstd[3] == exact_rstd
            # scale, shift and the running statistics follow from mean and rstd by the kernel's expressions, in float32
            w_scale, w_shift, w_rm, w_rv = gc.derived_stats(mean, rstd, n, gamma, beta, rm0, rv0)
            assert _same(scale, w_scale) and _same(shift, w_shift)
            if o["running"]:
                rm, rv = c["rm"].cpu().numpy(), c["rv"].cpu().numpy()
                assert _same(rm, w_rm)
                var_tol = gc.running_var_tol(rstd, n, rv0, w_rv)
                assert (np.abs(rv - w_rv) <= var_tol).all(), np.argwhere(np.abs(rv - w_rv) > var_tol)[:4]
                res += [rm, rv]
            res.append(st)
        got.append(res)
    assert all(_same(a, b) for a, b in zip(*got))
