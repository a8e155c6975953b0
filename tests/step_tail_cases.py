"""The case table of the reduction and gradient tail of a training step -- csrc/train_ops.hip: relu_bias_backward, recon_loss_grad,
sumsq / grad_norm_finish, step_losses, quantizer_input_grad(_bias), codebook_grad; csrc/vq_train.hip: apply_level, the three
code_stats forms, ema_update -- shared by tests/test_step_tail_host.py (CPU: every row gets the launch it is listed for, asked of
the library's own plan; the input builders keep their promises; the references satisfy their own bounds) and
tests/test_gpu_step_tail.py (GPU: every row against tests/step_tail_ref.py).

A row names a shape, the element offset of each operand inside a larger sentinel-filled buffer (offset 0: on 16 bytes; 1, 2, 3: not),
and what makes it different from its neighbours.  The shapes are the smallest that reach each launch; form_of() restates the
dispatch rules in a few lines, and the host test asks the library whether it agrees."""
import functools
import os
from collections import namedtuple

import numpy as np

import step_tail_ref as ref

F32 = np.float32
GUARD = 64                         # sentinel elements on both sides of every operand (a multiple of 16 bytes for every type)
SENT32, SENT64, SENT8 = 0x7FC5A5A5, 0x7FF5A5A5A5A5A5A5, 0xA5       # NaN patterns no arithmetic produces
RED_CAP = 256                      # workgroups of a flat reduction, of apply_level's sse
OOR = (-1, None, 2 ** 32 + 1, -2 ** 40)        # out-of-range codes planted among valid ones; None stands for K


def strip_cols():
    """The strip width of the dword strips: 16, or what LCREC_STRIP_COLS forces for the process (read once by the library)."""
    forced = int(os.environ.get("LCREC_STRIP_COLS", "0") or 0)
    return forced if forced in (8, 16, 32) else 16


def form(family, grid, **kw):
    d = dict(K=0, family=family, grid=grid, grid_sse=0, cols=0, xcd_order=0, vec16=0, second_launch=0, tail=0)
    d.update(kw)
    return d


# ---------------------------------------------------------------- rows

Recon = namedtuple("Recon", "count l1 off_out off_x off_g want_grad total_factor why")
RECON = []
for _l1 in (0, 1):
    for _count, _why in ((3, "tail only"), (4, "one quad, no tail"), (4099, "one quad-loop trip plus a tail"),
                         (1100003, "the 256-workgroup cap plus a tail")):
        RECON.append(Recon(_count, _l1, 0, 0, 0, True, 1, "16-byte path: " + _why))
        RECON.append(Recon(_count, _l1, 1, 0, 0, True, 1, "scalar path, out off 16 bytes: " + _why))
        RECON.append(Recon(_count, _l1, 0, 1, 0, True, 1, "scalar path, x off 16 bytes: " + _why))
        RECON.append(Recon(_count, _l1, 0, 0, 1, True, 1, "scalar path, grad alone off 16 bytes: " + _why))
    RECON.append(Recon(4099, _l1, 0, 0, 0, False, 1, "no gradient asked (g == NULL), 16-byte path"))
    RECON.append(Recon(4099, _l1, 2, 2, 0, False, 1, "no gradient asked, scalar path"))
    RECON.append(Recon(4099, _l1, 0, 0, 0, True, 3, "a shard of a global batch three times its size"))

Norm = namedtuple("Norm", "count off max_norm why")
NORM = [Norm(c, off, 1.0, why) for c, why in ((1, "one element, norm below max_norm: coefficient exactly 1"), (5, "one quad and a tail"),
                                              (16387, "two workgroups and a tail"), (4200003, "the 256-workgroup cap and a tail"))
        for off in (0, 3)]

Relu = namedtuple("Relu", "n F variant off why")
RELU_SHAPES = ((1, 16, "one row"), (63, 17, "below one row group, two strips"), (64, 1, "one column, exactly one row group"),
               (449, 15, "row group 0 takes one unrolled trip, the others the tail"), (512, 128, "grid 8: XCD-neighbour strips, no tail"),
               (513, 200, "grid 13, one row past the unrolled block"), (777, 2048, "a wide layer"))
RELU_VARIANTS = ("relu", "norelu", "no_g_out", "no_dbias", "inplace")
RELU = [Relu(n, F, v, (n + F + i) % 4, why) for n, F, why in RELU_SHAPES for i, v in enumerate(RELU_VARIANTS)]

Qg = namedtuple("Qg", "n e idx_cols off why")
QG = []
for _e in (16, 32, 64):
    _rg = 1024 // _e
    QG += [Qg(5, _e, 1, 1, "below one row group"), Qg(_rg, _e, 4, 0, "exactly one row group"),
           Qg(4 * _rg + 1, _e, 1, 0, "one row past the 4-row unroll"), Qg(4 * _rg + 1, _e, 4, 2, "the same, index column of [n, 4]"),
           Qg(4 * _rg + 1, _e, 5, 0, "the same, index column of [n, 5]"), Qg(65536 // _e, _e, 5, 0, "the one-workgroup limit"),
           Qg(65536 // _e + 1, _e, 4, 3, "the hand-over to the two-launch form")]
QG.append(Qg(100, 48, 5, 1, "an e the one-workgroup kernel does not take"))

CbGrad = namedtuple("CbGrad", "K e off why")
CBGRAD = [CbGrad(17, 15, 1, "255 elements"), CbGrad(16, 16, 0, "256 elements"), CbGrad(257, 1, 3, "257 elements")]

Losses = namedtuple("Losses", "L sums nan probe why")
LOSSES = [Losses(L, sums, nan, probe, f"L={L} sums={int(sums)} nan={nan} probe={probe}")
          for L in (1, 4, 8) for nan in ("none", "recon", "sse") for sums, probe in ((True, -1), (False, 5))]

Apply = namedtuple("Apply", "n e accumulate idx_cols alias idx_kind why")
APPLY = []
for _e in (16, 64):
    APPLY += [Apply(1, _e, False, 1, False, "valid", "one item"), Apply(1, _e, True, 1, False, "oor1", "one item, code -1"),
              Apply(77, _e, False, 1, False, "oracle", "the oracle's own argmin"), Apply(77, _e, True, 3, True, "oor", "strided column, aliased, accumulate, codes out of range"),
              Apply(8200, _e, False, 3, False, "oor", "the sse grid (cap at e = 64), strided column, codes out of range"),
              Apply(8200, _e, True, 1, True, "valid", "accumulate, aliased")]
APPLY_K = 9

Stats = namedtuple("Stats", "n e K pattern why")
STATS = []
for _e in (16, 32, 64):
    for _n, _K, _why in ((1, 1, "one item, one code"), (255, 7, "below one sort pass"), (257, 7, "one past a staged chunk"),
                         (8192, 1024, "the sorted form's limits"), (257, 1025, "K past the sort: streaming, levels fall back"),
                         (8193, 7, "n past the sort: streaming, levels fall back")):
        for _pat in ("spread", "one", "oor", "poison"):
            STATS.append(Stats(_n, _e, _K, _pat, _why))
STATS_L = 3

Ema = namedtuple("Ema", "K e skip why")
EMA = [Ema(K, e, skip, f"skip flag {skip}") for K, e in ((5, 16), (8, 32), (3, 64), (256, 32)) for skip in (None, 0, 1)]
EMA_DECAY, EMA_EPS = 0.99, 1e-5


def row_id(r):
    return "-".join(str(v) for v in r[:-1]).replace(" ", "_")


# ---------------------------------------------------------------- the launch each row is listed for

def red_form(count, per_thread, aligned):
    return form("reduce", min(RED_CAP, -(-count // (1024 * per_thread))), vec16=int(aligned), tail=count % 4 if aligned else count,
                second_launch=1)


def recon_aligned(r):
    return r.off_out == 0 and r.off_x == 0 and (r.off_g == 0 or not r.want_grad)


def form_of(r):
    """What lcrec_debug_step_tail_plan must report for the row's main call."""
    if isinstance(r, Recon):
        return red_form(r.count, 4, recon_aligned(r))
    if isinstance(r, Norm):
        return red_form(r.count, 16, r.off == 0)
    if isinstance(r, Relu):
        cols = strip_cols()
        grid = -(-r.F // cols)
        return form("strip", grid, cols=cols, xcd_order=int(cols < 32 and grid % 8 == 0), tail=r.n % (8 * (1024 // cols)))
    if isinstance(r, Qg):
        if r.e in (16, 32, 64) and r.n * r.e <= 65536:
            return form("qgb_one", 1, tail=r.n % (4 * (1024 // r.e)))
        return form("qg_two", min(2048, -(-r.n * r.e // 1024)), second_launch=1)
    if isinstance(r, Apply):
        grid = min(1024, -(-r.n * (r.e // 4) // 256))
        return form("apply_level", grid, grid_sse=min(RED_CAP, grid), vec16=1, second_launch=1)
    raise TypeError(r)


def stats_forms(r):
    """(code_stats, code_stats_levels) for a Stats row."""
    if r.n <= 8192 and r.K <= 1024:
        grid = -(-r.K * r.e // 256)
        return form("cs_sorted", grid, K=r.K, vec16=1), form("cs_levels", grid, K=r.K, vec16=1)
    return form("cs_streaming", -(-r.K // (256 // r.e)), K=r.K, vec16=1), form("cs_per_level", 0, K=r.K, vec16=1, second_launch=1)


def plan_args(r):
    """(call, n_or_count, width, aligned, K) of ops.step_tail_plan for the row's main call."""
    if isinstance(r, Recon):
        return ("recon_loss_grad", r.count, 0, recon_aligned(r), 0)
    if isinstance(r, Norm):
        return ("grad_norm_clip", r.count, 0, r.off == 0, 0)
    if isinstance(r, Relu):
        return ("relu_bias_backward", r.n, r.F, True, 0)
    if isinstance(r, Qg):
        return ("quantizer_input_grad_bias", r.n, r.e, True, 0)
    if isinstance(r, Apply):
        return ("rq_apply_level", r.n, r.e, True, 0)
    raise TypeError(r)


# ---------------------------------------------------------------- input builders (host, deterministic; shared: read only)

def _rs(*key):
    return np.random.RandomState(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


@functools.lru_cache(maxsize=4)
def recon_inputs(r):
    """(out, x): element i has out - x above 0 (i % 3 == 0), below 0 (i % 3 == 1), exactly 0 (i % 3 == 2) -- so the first element
    of the array, and the first of a ragged tail after 4096 elements, each move the loss."""
    rs = _rs(1, r.count, r.l1)
    x = ref.f32(rs.standard_normal(r.count))
    step = ref.f32(0.125 + np.abs(rs.standard_normal(r.count)))
    sign = np.array([1.0, -1.0, 0.0], dtype=np.float32)[np.arange(r.count) % 3]
    return ref.f32(x + sign * step), x


@functools.lru_cache(maxsize=2)
def norm_inputs(r):
    rs = _rs(2, r.count)
    return ref.f32(0.25 * np.ones(1)) if r.count == 1 else ref.f32(rs.standard_normal(r.count))


@functools.lru_cache(maxsize=4)
def relu_inputs(r):
    """(gy, y): y holds exact +0.0 (every 7th element) and -0.0 (every 11th from 3) among both signs."""
    rs = _rs(3, r.n, r.F)
    gy, y = ref.f32(rs.standard_normal((r.n, r.F))), ref.f32(rs.standard_normal((r.n, r.F)))
    flat = y.reshape(-1)
    flat[::7] = 0.0
    flat[3::11] = -0.0
    return gy, y


QG_K, QG_COEF, QG_WEIGHT = 37, 0.37, 1.3


@functools.lru_cache(maxsize=4)
def qg_inputs(r):
    """(z, cb0, idx matrix [n, idx_cols] whose column 0 is the level-0 index, g_xq of the size of the other term)."""
    rs = _rs(4, r.n, r.e, r.idx_cols)
    z, cb0 = ref.f32(rs.standard_normal((r.n, r.e))), ref.f32(rs.standard_normal((QG_K, r.e)))
    idx = rs.randint(0, QG_K, size=(r.n, r.idx_cols)).astype(np.int64)
    idx[:, 1:] = 10 ** 12                       # the other columns: what a wrong stride would read (and fault on: never launched wrong here)
    g_xq = ref.f32(QG_COEF * QG_WEIGHT * 1.4 * rs.standard_normal((r.n, r.e)))
    return z, cb0, idx, g_xq


def cbgrad_inputs(r):
    rs = _rs(5, r.K, r.e)
    return (ref.f32(rs.randint(0, 9, size=r.K)), ref.f32(rs.standard_normal((r.K, r.e))), ref.f32(rs.standard_normal((r.K, r.e))),
            0.031, 0.25)                         # count, sum, codebook, scale, weight


LOSS_N, LOSS_E, LOSS_BETA, LOSS_QLW = 1024, 32, 0.25, 1.0


def losses_inputs(r):
    """Two calls' worth: ((sse, recon, probe) of the first call, per the row; of the second: clean)."""
    rs = _rs(6, r.L)
    sse1, sse2 = rs.uniform(100.0, 900.0, size=r.L), rs.uniform(100.0, 900.0, size=r.L)
    rec1, rec2 = F32(0.37), F32(0.29)
    if r.nan == "recon":
        rec1 = F32(np.nan)
    if r.nan == "sse":
        sse1[r.L // 2] = np.nan
    return (sse1, rec1, r.probe), (sse2, rec2, 7)


def plant_oor(col, K):
    """The four out-of-range codes at the front of an index column, valid ones after them."""
    for i, v in enumerate(OOR[:len(col)]):
        col[i] = K if v is None else v
    return col


@functools.lru_cache(maxsize=4)
def apply_inputs(r):
    """(resid, codebook, idx matrix [n, idx_cols] -- the level's column is the last one --, xq_in or None)."""
    rs = _rs(7, r.n, r.e, r.idx_cols)
    resid, cb = ref.f32(rs.standard_normal((r.n, r.e))), ref.f32(rs.standard_normal((APPLY_K, r.e)))
    idx = rs.randint(0, APPLY_K, size=(r.n, r.idx_cols)).astype(np.int64)
    if r.idx_kind == "oracle":
        from oracle import cpu_oracle
        idx[:, -1] = cpu_oracle.rq_assign(resid, [cb])["idx"][:, 0]
    elif r.idx_kind == "oor":
        plant_oor(idx[:, -1], APPLY_K)
    elif r.idx_kind == "oor1":
        idx[0, -1] = -1
    xq = ref.f32(rs.standard_normal((r.n, r.e))) if r.accumulate else None
    return resid, cb, idx, xq


@functools.lru_cache(maxsize=4)
def stats_inputs(r):
    """(idx [n, STATS_L], [resid_l], [codebook_l]): `spread`: random codes (K > n leaves codes empty; code K - 1 is kept empty when
    K > 2), `one`: a single code owns every row, `oor`: spread with the out-of-range codes planted in every column, `poison`:
    every code -1, the column a batch-sized Sinkhorn solve leaves when it gives up."""
    rs = _rs(8, r.n, r.e, r.K)
    hi = r.K - 1 if r.K > 2 else r.K
    idx = rs.randint(0, hi, size=(r.n, STATS_L)).astype(np.int64)
    if r.pattern == "one":
        idx[:] = np.array([r.K // 2, 0, r.K - 1], dtype=np.int64)[:STATS_L]
    if r.pattern == "oor":
        for l in range(STATS_L):
            plant_oor(idx[:, l], r.K)
    if r.pattern == "poison":
        idx[:] = -1
    resid = [ref.f32(rs.standard_normal((r.n, r.e))) for _ in range(STATS_L)]
    cbs = [ref.f32(rs.standard_normal((r.K, r.e))) for _ in range(STATS_L)]
    return idx, resid, cbs


def _count_landing_on(eps32, dec):
    """An ema_count whose product with the float32 decay rounds exactly to eps, and its neighbours' landing sides."""
    c = F32(eps32 / dec)
    for _ in range(16):
        p = c * dec
        if p == eps32:
            return c
        c = np.nextafter(c, F32(np.inf) if p < eps32 else F32(-np.inf))
    raise AssertionError("no float32 lands on eps")


def ema_inputs(r):
    """(ema_count, ema_sum, codebook, count, sum).  Codes 0, 1, 2 get no items this step and an ema_count that the decay brings
    just below, exactly onto and just above eps; the others are ordinary."""
    rs = _rs(9, r.K, r.e)
    dec, _, _ = ref.ema_rates(EMA_DECAY)
    eps32 = F32(EMA_EPS)
    on = _count_landing_on(eps32, dec)
    below = on
    while below * dec >= eps32:
        below = np.nextafter(below, F32(-np.inf))
    above = on
    while above * dec <= eps32:
        above = np.nextafter(above, F32(np.inf))
    ema_count = ref.f32(rs.uniform(0.5, 20.0, size=r.K))
    count = ref.f32(rs.randint(0, 6, size=r.K))
    ema_count[:3] = (below, on, above)
    count[:3] = 0.0
    total = ref.f32(rs.standard_normal((r.K, r.e)) * count[:, None])
    return ema_count, ref.f32(rs.standard_normal((r.K, r.e))), ref.f32(rs.standard_normal((r.K, r.e))), count, total


# ---------------------------------------------------------------- device side: operands inside sentinel-filled buffers

class Arena:
    """Device operands carved out of larger buffers filled with a sentinel: GUARD elements, the row's offset, the operand, GUARD
    elements.  check() finds every sentinel outside the operands in place."""

    def __init__(self, device):
        import torch
        self.torch, self.device, self.items = torch, device, []

    def put(self, data, off=0, dtype=None, shape=None):
        """data: a numpy array to upload, or None with dtype and shape for an output (left full of sentinels)."""
        torch = self.torch
        if data is not None:
            data = np.ascontiguousarray(data)
            dtype, shape = data.dtype, data.shape
        dtype = np.dtype(dtype)
        numel = int(np.prod(shape, dtype=np.int64))
        carrier, sent = {1: (torch.uint8, SENT8), 4: (torch.int32, SENT32), 8: (torch.int64, SENT64)}[dtype.itemsize]
        buf = torch.full((GUARD + off + numel + GUARD,), sent, dtype=carrier, device=self.device)
        view = buf[GUARD + off:GUARD + off + numel]
        assert (view.data_ptr() % 16 == 0) == (off * dtype.itemsize % 16 == 0)
        if data is not None:
            view.copy_(torch.from_numpy(data.reshape(-1).view({1: np.uint8, 4: np.int32, 8: np.int64}[dtype.itemsize])))
        self.items.append((buf, GUARD + off, numel, sent))
        return Operand(view, dtype, shape)

    def check(self):
        for buf, lo, numel, sent in self.items:
            assert bool((buf[:lo] == sent).all()) and bool((buf[lo + numel:] == sent).all()), "a sentinel beside an operand was overwritten"


class Operand:
    def __init__(self, view, dtype, shape):
        self.view, self.dtype, self.shape = view, dtype, tuple(shape)

    @property
    def ptr(self):
        return self.view.data_ptr()

    def numpy(self):
        return self.view.cpu().numpy().view(self.dtype).reshape(self.shape)


def _ptr(op):
    return None if op is None else op.ptr


def _rc(hip, rc, what):
    hip._lib.check(rc, what)


def _ticket(hip, dev, tickets):
    """(pointer or None, the ticket tensor or None) under ops.USE_TICKETS = tickets."""
    ops = hip.ops
    saved = ops.USE_TICKETS
    ops.USE_TICKETS = tickets
    try:
        t = ops._ticket(dev)
    finally:
        ops.USE_TICKETS = saved
    return (None if t is None else t.data_ptr()), t


def _workspace(hip, dev, nbytes=None):
    lib = hip._lib.load()
    return hip.ops._workspace(nbytes or lib.lcrec_train_reduce_workspace(), dev)


def _ticket_is_zero(t):
    return t is None or int(t[0]) == 0


def run_recon(hip, r, dev, tickets=True):
    import torch
    lib, a = hip._lib.load(), Arena(dev)
    out, x = recon_inputs(r)
    o_d, x_d = a.put(out, r.off_out), a.put(x, r.off_x)
    g_d = a.put(None, r.off_g, np.float32, (r.count,)) if r.want_grad else None
    loss = a.put(None, 0, np.float32, (1,))
    tp, t = _ticket(hip, dev, tickets)
    with torch.cuda.device(dev):
        ws = _workspace(hip, dev)
        _rc(hip, lib.lcrec_recon_loss_grad(o_d.ptr, x_d.ptr, r.count, r.count * r.total_factor if r.total_factor > 1 else 0, r.l1, _ptr(g_d),
                                           loss.ptr, ws.data_ptr(), ws.numel(), tp, hip.ops._stream_ptr()), "lcrec_recon_loss_grad")
    res = {"loss": loss.numpy().copy()}
    if g_d is not None:
        res["grad"] = g_d.numpy().copy()
    a.check()
    assert _ticket_is_zero(t), "the ticket word is not zero after the call"
    return res


def run_norm(hip, r, dev, tickets=True):
    import torch
    lib, a = hip._lib.load(), Arena(dev)
    g_d = a.put(norm_inputs(r), r.off)
    res = a.put(None, 0, np.float32, (2,))
    tp, t = _ticket(hip, dev, tickets)
    with torch.cuda.device(dev):
        ws = _workspace(hip, dev)
        _rc(hip, lib.lcrec_grad_norm_clip(g_d.ptr, r.count, r.max_norm, res.ptr, ws.data_ptr(), ws.numel(), tp, hip.ops._stream_ptr()),
            "lcrec_grad_norm_clip")
    out = {"norm_coef": res.numpy().copy()}
    a.check()
    assert _ticket_is_zero(t), "the ticket word is not zero after the call"
    return out


def run_relu(hip, r, dev):
    import torch
    lib, a = hip._lib.load(), Arena(dev)
    gy, y = relu_inputs(r)
    relu = r.variant != "norelu"
    gy_d = a.put(gy, r.off)
    y_d = a.put(y, (r.off + 1) % 4) if relu else None
    g_d = None if r.variant == "no_g_out" else (gy_d if r.variant == "inplace" else a.put(None, (r.off + 2) % 4, np.float32, gy.shape))
    db_d = None if r.variant == "no_dbias" else a.put(None, (r.off + 3) % 4, np.float32, (r.F,))
    with torch.cuda.device(dev):
        _rc(hip, lib.lcrec_relu_bias_backward(gy_d.ptr, _ptr(y_d), r.n, r.F, int(relu), _ptr(g_d), _ptr(db_d), hip.ops._stream_ptr()),
            "lcrec_relu_bias_backward")
    out = {}
    if g_d is not None:
        out["g"] = g_d.numpy().copy()
    else:
        out["gy_after"] = gy_d.numpy().copy()
    if db_d is not None:
        out["dbias"] = db_d.numpy().copy()
    a.check()
    return out


def run_qg(hip, r, dev, bias):
    import torch
    lib, a = hip._lib.load(), Arena(dev)
    z, cb0, idx, g_xq = qg_inputs(r)
    z_d, cb_d, idx_d, gx_d = a.put(z, r.off), a.put(cb0, (r.off + 1) % 4), a.put(idx, r.off % 2), a.put(g_xq, (r.off + 2) % 4)
    out_d = a.put(None, (r.off + 3) % 4, np.float32, z.shape)
    db_d = a.put(None, r.off, np.float32, (r.e,)) if bias else None
    with torch.cuda.device(dev):
        if bias:
            rc = lib.lcrec_quantizer_input_grad_bias(z_d.ptr, cb_d.ptr, idx_d.ptr, r.idx_cols, r.n, r.e, QG_COEF, QG_WEIGHT, gx_d.ptr, out_d.ptr,
                                                     db_d.ptr, hip.ops._stream_ptr())
        else:
            rc = lib.lcrec_quantizer_input_grad(z_d.ptr, cb_d.ptr, idx_d.ptr, r.idx_cols, r.n, r.e, QG_COEF, QG_WEIGHT, gx_d.ptr, out_d.ptr,
                                                hip.ops._stream_ptr())
    _rc(hip, rc, "lcrec_quantizer_input_grad")
    res = {"out": out_d.numpy().copy()}
    if bias:
        res["dbias"] = db_d.numpy().copy()
    a.check()
    return res


def run_cbgrad(hip, r, dev):
    import torch
    lib, a = hip._lib.load(), Arena(dev)
    count, total, cb, scale, weight = cbgrad_inputs(r)
    c_d, t_d, cb_d = a.put(count, r.off), a.put(total, (r.off + 1) % 4), a.put(cb, (r.off + 2) % 4)
    g_d = a.put(None, (r.off + 3) % 4, np.float32, cb.shape)
    with torch.cuda.device(dev):
        _rc(hip, lib.lcrec_codebook_grad(c_d.ptr, t_d.ptr, cb_d.ptr, r.K, r.e, scale, weight, g_d.ptr, hip.ops._stream_ptr()), "lcrec_codebook_grad")
    res = {"grad": g_d.numpy().copy()}
    a.check()
    return res


def run_losses(hip, r, dev):
    """Two calls on the same outputs: (out3 of call 1, out3 of call 2, sums, nan flag, probe flag after each)."""
    import torch
    lib, a = hip._lib.load(), Arena(dev)
    first, second = losses_inputs(r)
    out3 = a.put(None, 1, np.float32, (3,))
    sums = a.put(np.zeros(2), 1) if r.sums else None
    nan_flag, probe_flag = a.put(np.zeros(1, dtype=np.uint8), 3), a.put(np.zeros(1, dtype=np.uint8), 5)
    res = {}
    for tag, (sse, rec, probe) in (("1", first), ("2", second)):
        sse_d, rec_d, probe_d = a.put(sse, 1), a.put(np.array([rec], dtype=np.float32), 2), a.put(np.array([probe], dtype=np.int64), 1)
        with torch.cuda.device(dev):
            _rc(hip, lib.lcrec_step_losses(sse_d.ptr, r.L, LOSS_N, LOSS_E, LOSS_BETA, LOSS_QLW, rec_d.ptr, out3.ptr, _ptr(sums), nan_flag.ptr,
                                           probe_d.ptr, probe_flag.ptr, hip.ops._stream_ptr()), "lcrec_step_losses")
        res["out3_" + tag] = out3.numpy().copy()
        res["flags_" + tag] = (int(nan_flag.numpy()[0]), int(probe_flag.numpy()[0]))
    if sums is not None:
        res["sums"] = sums.numpy().copy()
    a.check()
    return res


def run_apply(hip, r, dev, tickets=True):
    import torch
    lib, a = hip._lib.load(), Arena(dev)
    resid, cb, idx, xq = apply_inputs(r)
    r_d, cb_d, idx_d = a.put(resid), a.put(cb), a.put(idx)
    xq_d = a.put(xq) if r.accumulate else a.put(None, 0, np.float32, resid.shape)
    ro_d = r_d if r.alias else a.put(None, 0, np.float32, resid.shape)
    sse_d = a.put(None, 1, np.float64, (1,))
    tp, t = _ticket(hip, dev, tickets)
    with torch.cuda.device(dev):
        ws = _workspace(hip, dev, 8192)
        col = idx_d.ptr + 8 * (r.idx_cols - 1)
        _rc(hip, lib.lcrec_rq_apply_level(r_d.ptr, r.n, r.e, cb_d.ptr, APPLY_K, col, r.idx_cols, xq_d.ptr, int(r.accumulate), ro_d.ptr, sse_d.ptr,
                                          ws.data_ptr(), ws.numel(), tp, hip.ops._stream_ptr()), "lcrec_rq_apply_level")
    res = {"xq": xq_d.numpy().copy(), "resid": ro_d.numpy().copy(), "sse": sse_d.numpy().copy()}
    a.check()
    assert _ticket_is_zero(t), "the ticket word is not zero after the call"
    return res


def run_stats(hip, r, dev):
    """code_stats on every column of the row's index matrix, and code_stats_levels (with the fused gradients) on the matrix."""
    import ctypes
    import torch
    lib, a = hip._lib.load(), Arena(dev)
    idx, resid, cbs = stats_inputs(r)
    idx_d = a.put(idx)
    r_d, cb_d = [a.put(x) for x in resid], [a.put(c) for c in cbs]
    single = [(a.put(None, 1, np.float32, (r.K,)), a.put(None, 0, np.float32, (r.K, r.e))) for _ in range(STATS_L)]
    fused = [(a.put(None, 3, np.float32, (r.K,)), a.put(None, 0, np.float32, (r.K, r.e)), a.put(None, 0, np.float32, (r.K, r.e)))
             for _ in range(STATS_L)]
    PA = ctypes.c_void_p * STATS_L
    with torch.cuda.device(dev):
        for l in range(STATS_L):
            _rc(hip, lib.lcrec_code_stats(idx_d.ptr + 8 * l, STATS_L, r_d[l].ptr, r.n, r.e, r.K, single[l][0].ptr, single[l][1].ptr,
                                          hip.ops._stream_ptr()), "lcrec_code_stats")
        _rc(hip, lib.lcrec_code_stats_levels(idx_d.ptr, PA(*[x.ptr for x in r_d]), r.n, r.e, hip.ops._ints([r.K] * STATS_L), STATS_L,
                                             PA(*[f[0].ptr for f in fused]), PA(*[f[1].ptr for f in fused]), PA(*[c.ptr for c in cb_d]),
                                             PA(*[f[2].ptr for f in fused]), STATS_SCALE, STATS_WEIGHT, hip.ops._stream_ptr()),
            "lcrec_code_stats_levels")
    res = {"single": [(c.numpy().copy(), s.numpy().copy()) for c, s in single],
           "levels": [(c.numpy().copy(), s.numpy().copy(), g.numpy().copy()) for c, s, g in fused]}
    a.check()
    return res


STATS_SCALE, STATS_WEIGHT = 0.0625 / 3, 0.7


def run_ema(hip, r, dev):
    import torch
    lib, a = hip._lib.load(), Arena(dev)
    ema_count, ema_sum, cb, count, total = ema_inputs(r)
    ec_d, es_d, cb_d, c_d, t_d = a.put(ema_count, 1), a.put(ema_sum), a.put(cb, 2), a.put(count, 3), a.put(total, 1)
    skip_d = None if r.skip is None else a.put(np.array([r.skip], dtype=np.uint8), 7)
    dec, alpha, keep = ref.ema_rates(EMA_DECAY)
    with torch.cuda.device(dev):
        _rc(hip, lib.lcrec_ema_update(ec_d.ptr, es_d.ptr, cb_d.ptr, c_d.ptr, t_d.ptr, r.K, r.e, float(dec), float(alpha), float(keep), EMA_EPS,
                                      _ptr(skip_d), hip.ops._stream_ptr()), "lcrec_ema_update")
    res = {"ema_count": ec_d.numpy().copy(), "ema_sum": es_d.numpy().copy(), "codebook": cb_d.numpy().copy()}
    a.check()
    return res
