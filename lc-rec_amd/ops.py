"""Tensor-level entry points over the C-ABI (include/lcrec.h).

torch is plumbing here: it owns device memory and the stream; every function
hands raw device pointers to liblcrec_hip.so and enqueues on torch's current
stream.  Inputs must already live on a HIP device; nothing here computes on
the CPU.
"""
import ctypes
import functools
import threading

import torch

from . import _lib

_c_int_p = ctypes.POINTER(ctypes.c_int)
_workspaces = {}

# Default threshold of the near-tie audit (lcrec_rq_assign's tie_tau): a level is flagged when its top-2 distance gap is
# <= NEARTIE_TAU * (xx + cc[idx]).  Measured, not derived (oracle/neartie_audit.py, tests/golden/f9_neartie_*.npz): on
# 1 M x 768-d items 33 tuples differ between the reference's CPU ops (batch 64 or 4096; the two batch sizes differ from
# EACH OTHER on 9) and this library's canonical order, the worst of them at a relative gap of 2.5e-6; 2^-17 covers that
# with a power of two of slack and flags 995 of the 1 M items (0.1 %).  On the Games shape (16 859 x 4096-d) 0 differ.
NEARTIE_TAU = 2.0 ** -17


# Host cost matters: a training step makes ~50 calls into the library, and torch.cuda.current_stream() /
# torch.cuda.device() cost 5-10 us each (Stream objects, index normalisation) -- as much as the launch itself.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream_int(index=None):
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device() if index is None else index)
    return torch.cuda.current_stream(index).cuda_stream


def _stream_ptr():
    return ctypes.c_void_p(_stream_int())


class _on:
    """`with _on(device)`: torch.cuda.device(device), skipped when that device is already current."""
    __slots__ = ("guard",)

    def __init__(self, device):
        same = _cur_device is not None and device.index is not None and device.index == _cur_device()
        self.guard = None if same else torch.cuda.device(device)

    def __enter__(self):
        if self.guard is not None:
            self.guard.__enter__()

    def __exit__(self, *exc):
        if self.guard is not None:
            return self.guard.__exit__(*exc)
        return False


def _dev(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.LcrecError(f"{name} must be a tensor on a HIP device (lcrec_amd has no CPU path)")
    if t.dtype != torch.float32:
        raise _lib.LcrecError(f"{name} must be float32, got {t.dtype}")
    return t.contiguous()


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _ints(values):
    return (ctypes.c_int * len(values))(*[int(v) for v in values])


def _workspace(nbytes, device):
    """Grow-only scratch buffer per (device, stream); reuse is safe because calls are stream-ordered."""
    key = (device.index, _stream_int(device.index))
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _workspaces[key] = buf
    return buf


def release_workspaces():
    _workspaces.clear()
    _tickets.clear()


# `ticket` arguments of include/lcrec.h: one zeroed 4-byte word per (device, stream) -- every call leaves it zero, and calls on
# one stream are ordered, so they can all share it.  LCREC_TICKETS=0 (diagnostic): the two-launch forms.
_tickets = {}
USE_TICKETS = __import__("os").environ.get("LCREC_TICKETS", "1") != "0"


def _ticket(device, force=False):
    """int32 [96] zeros: word 0 is the ticket of the reduction tails; words 16 .. 79 are the 64 column-strip tickets of
    lcrec_linear_bn_forward (force=True: that call has no ticket-less form)."""
    if not USE_TICKETS and not force:
        return None
    key = (device.index, _stream_int(device.index))
    t = _tickets.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            raise _lib.LcrecError("the stream's ticket word must exist before a graph capture (run the step once eagerly first)")
        t = _tickets[key] = torch.zeros(96, dtype=torch.int32, device=device)
    return t


# One lcrec_context per device (include/lcrec.h): the library's helper streams, their events and the pinned upload ring.
# Created on first use by the two calls that can overlap launches, destroyed at interpreter exit / release_contexts().
_contexts = {}
_pipelines = 1


def _context(device):
    ctx = _contexts.get(device.index)
    if ctx is None:
        lib = _lib.load()
        h = ctypes.c_void_p()
        with _on(device):
            _lib.check(lib.lcrec_context_create(ctypes.byref(h)), "lcrec_context_create")
        _lib.check(lib.lcrec_context_set_pipelines(h, _pipelines), "lcrec_context_set_pipelines")
        ctx = _contexts[device.index] = h
    return ctx


def set_pipelines(n):
    """Chunk pipelines of encode_assign (lcrec_context_set_pipelines): 1 (default) = everything on the current stream,
    2 = odd chunks on a helper stream (+1.5-1.9 % on C3, but see include/lcrec.h: intermittently much slower)."""
    global _pipelines
    n = int(n)
    if n not in (1, 2):
        raise _lib.LcrecError("pipelines must be 1 or 2")
    _pipelines = n
    for h in _contexts.values():
        _lib.check(_lib.load().lcrec_context_set_pipelines(h, n), "lcrec_context_set_pipelines")


def release_contexts():
    """Drain and destroy the library's helper streams (lcrec_context_destroy)."""
    while _contexts:
        _, h = _contexts.popitem()
        try:
            _lib.load().lcrec_context_destroy(h)
        except Exception:          # interpreter shutdown: the runtime may already be gone
            pass


def _forget_contexts_at_exit():
    """Interpreter exit: drop the handles WITHOUT calling into the library.  lcrec_context_destroy synchronises and destroys
    streams; at exit the HIP runtime (and a profiler's preloaded tool library) is tearing down underneath it, and a profiled run
    was seen not to return from its exit handlers (tools/prof_train.sh).  Process teardown reclaims streams, events and pinned
    memory anyway; release_contexts() remains the explicit, orderly way while the process lives."""
    _contexts.clear()


import atexit  # noqa: E402
atexit.register(_forget_contexts_at_exit)


def _audit_buffers(audit, tie_tau, n, L, dev):
    """(margin tensor | None, neartie tensor | None, tau) for the near-tie audit outputs of lcrec_rq_assign."""
    if audit is None:
        return None, None, 0.0
    margin = torch.empty((n, L), dtype=torch.float32, device=dev)
    neartie = torch.zeros(n, dtype=torch.int32, device=dev) if tie_tau is not None else None
    audit["margin"] = margin
    if neartie is not None:
        audit["neartie"] = neartie           # bit l: level l's top-2 gap <= tie_tau * (xx + cc[idx])
        audit["tie_tau"] = float(tie_tau)
    return margin, neartie, float(tie_tau or 0.0)


def linear_forward(x, weight, bias=None, bn_scale=None, bn_shift=None, relu=False, out=None):
    """y = [relu]([bn](x @ weight.T + bias)) -- one group of MLPLayers.forward (layers.py:18-30,42).
    out: optional contiguous float32 [n, out_dim] device tensor the result is written into (a row range of a larger
    buffer, say); it is returned."""
    lib = _lib.load()
    x = _dev(x, "x")
    weight = _dev(weight, "weight")
    bias = None if bias is None else _dev(bias, "bias")
    bn_scale = None if bn_scale is None else _dev(bn_scale, "bn_scale")
    bn_shift = None if bn_shift is None else _dev(bn_shift, "bn_shift")
    n, k = x.shape
    out_dim = weight.shape[0]
    if weight.shape[1] != k:
        raise _lib.LcrecError(f"weight is {tuple(weight.shape)}, x is {tuple(x.shape)}")
    y = out if out is not None else torch.empty((n, out_dim), dtype=torch.float32, device=x.device)
    if y.shape != (n, out_dim) or y.dtype != torch.float32 or y.device != x.device or not y.is_contiguous():
        raise _lib.LcrecError("out must be a contiguous float32 [n, out_dim] tensor on x's device")
    with _on(x.device):
        rc = lib.lcrec_linear_forward(_ptr(x), n, k, _ptr(weight), _ptr(bias), _ptr(bn_scale), _ptr(bn_shift),
                                      int(bool(relu)), out_dim, _ptr(y), _stream_ptr())
    _lib.check(rc, "lcrec_linear_forward")
    return y


def linear_bn_supported(n, in_dim, out_dim):
    """Whether lcrec_linear_bn_forward takes this shape (a batch-sized launch; include/lcrec.h), input fold and batch
    statistics both asked for.  The library is asked (lcrec_debug_linear_bn_forward_plan, the function the entry point
    launches by), not a copy of its rule: a host-only call, nothing is launched and no device is needed.  A refusal writes the
    last-error text of the thread that asked, and a question is no error of the caller's: each shape is asked once, on a
    thread of its own, and remembered (the training engine asks for every layer of every eager step)."""
    return _linear_bn_supported(int(n), int(in_dim), int(out_dim))


@functools.lru_cache(maxsize=None)
def _linear_bn_supported(n, in_dim, out_dim):
    plan, answer = _lib.load().lcrec_debug_linear_bn_forward_plan, []
    asker = threading.Thread(target=lambda: answer.append(plan(n, in_dim, out_dim, 1, 1, ctypes.byref(_lib.GemmLaunch())) == 1))
    asker.start()
    asker.join()
    return answer[0]


def linear_bn_forward(x, weight, bias, in_fold=None, in_relu=True, bn=None):
    """One Linear of a training step with the BatchNorms around it folded in (lcrec_linear_bn_forward):
    t = max(x * in_fold[0] + in_fold[1], 0 if in_relu) @ weight.T + bias, and -- with bn = (gamma, beta, eps, momentum,
    running_mean, running_var) -- the batch statistics of t.  Returns (t, None) or (t, (mean, rstd, scale, shift)):
    scale / shift are this BatchNorm's folded affine, the next layer's in_fold."""
    lib = _lib.load()
    x, weight, bias = _dev(x, "x"), _dev(weight, "weight"), _dev(bias, "bias")
    n, k = x.shape
    out_dim = weight.shape[0]
    dev = x.device
    t = torch.empty((n, out_dim), dtype=torch.float32, device=dev)
    sc, sh = (None, None) if in_fold is None else (_vec(in_fold[0], "in_scale", k), _vec(in_fold[1], "in_shift", k))
    stats = None
    gamma = beta = rm = rv = None
    eps = momentum = 0.0
    if bn is not None:
        gamma, beta, eps, momentum, rm, rv = bn
        stats = torch.empty((4, out_dim), dtype=torch.float32, device=dev)     # mean, rstd, scale, shift
        gamma, beta = _vec(gamma, "gamma", out_dim), _vec(beta, "beta", out_dim)
    with _on(dev):
        ws = _workspace(lib.lcrec_linear_bn_forward_workspace(n, out_dim), dev) if bn is not None else None
        tk = _ticket(dev, force=True) if bn is not None else None
        rc = lib.lcrec_linear_bn_forward(_ptr(x), n, k, _ptr(sc), _ptr(sh), int(bool(in_relu)), _ptr(weight), _ptr(bias), out_dim,
                                         _ptr(t), int(bn is not None), _ptr(gamma), _ptr(beta), float(eps), float(momentum or 0.0),
                                         _ptr(rm), _ptr(rv), _ptr(None if stats is None else stats[0]),
                                         _ptr(None if stats is None else stats[1]), _ptr(None if stats is None else stats[2]),
                                         _ptr(None if stats is None else stats[3]), _ptr(ws), 0 if ws is None else ws.numel(),
                                         ctypes.c_void_p(tk.data_ptr() + 64) if tk is not None else None, _stream_ptr())
    _lib.check(rc, "lcrec_linear_bn_forward")
    return t, (None if stats is None else (stats[0], stats[1], stats[2], stats[3]))


def linear_backward(gy, x, weight, need_gx=True, need_gw=True, gw_out=None):
    """(gx, gw) of y = x W^T for a given gy = dL/dy (autograd's LinearBackward; include/lcrec.h,
    lcrec_linear_backward): gx = gy W, gw = gy^T x, every operand read as stored.  Raises
    LcrecError(LCREC_EUNSUPPORTED) for shapes the k-major kernels do not cover.
    gw_out: optional contiguous [out_dim, in_dim] tensor the weight gradient is written into (a view of a flat
    gradient buffer).
    The dX kernel slices K = out_dim in steps of 32: for a layer whose width is not a multiple of that (e_dim 16, say),
    gy gets zero columns and weight zero rows up to the next multiple first -- fma(0, w, acc) adds nothing, the copies are
    a few KB -- and gw is the first out_dim rows of the padded product (the same bits: dW contracts over the batch)."""
    lib = _lib.load()
    gy, x, weight = _dev(gy, "gy"), _dev(x, "x"), _dev(weight, "weight")
    n, out_dim = gy.shape
    in_dim = x.shape[1]
    if x.shape[0] != n or tuple(weight.shape) != (out_dim, in_dim):
        raise _lib.LcrecError(f"linear_backward: shapes gy {tuple(gy.shape)}, x {tuple(x.shape)}, W {tuple(weight.shape)}")
    pad = (-out_dim) % 32 if need_gx else 0
    if pad:
        gx, gw = linear_backward(torch.nn.functional.pad(gy, (0, pad)), x, torch.nn.functional.pad(weight, (0, 0, 0, pad)), True, need_gw)
        if gw is not None and gw_out is not None:
            gw_out.copy_(gw[:out_dim])
            return gx, gw_out
        return gx, None if gw is None else gw[:out_dim]
    gx = torch.empty((n, in_dim), dtype=torch.float32, device=gy.device) if need_gx else None
    gw = None
    if need_gw:
        gw = gw_out if gw_out is not None else torch.empty((out_dim, in_dim), dtype=torch.float32, device=gy.device)
        if tuple(gw.shape) != (out_dim, in_dim) or not gw.is_contiguous() or gw.dtype != torch.float32:
            raise _lib.LcrecError("gw_out must be a contiguous float32 [out_dim, in_dim] tensor")
    with _on(gy.device):
        nbytes = lib.lcrec_linear_backward_workspace(n, in_dim, out_dim) if need_gw else 0
        ws = _workspace(nbytes, gy.device)
        rc = lib.lcrec_linear_backward(_ptr(gy), _ptr(x), _ptr(weight), n, in_dim, out_dim, _ptr(gx), _ptr(gw), _ptr(ws),
                                       ws.numel(), _stream_ptr())
    _lib.check(rc, "lcrec_linear_backward")
    return gx, gw


def linear_backward_weights(problems, splits=0):
    """Weight gradients of several Linear layers in ONE launch (lcrec_linear_backward_weights): `problems` is a list of
    (gy [n, out], x [n, in], gw_out [out, in]) device tensors; every gw_out is written in place, bit-identical to what
    linear_backward(gy, x, W, need_gx=False) computes for that layer.  A fourth entry (scale, shift, relu) makes the layer
    input max(x * scale + shift, 0 if relu) -- x being a pre-BatchNorm tensor of lcrec_linear_bn_forward -- formed on the fly.
    splits > 0: that many K-runs over the batch for every problem instead of lcrec_linear_backward_splits' (1 = one chain)."""
    lib = _lib.load()
    count = len(problems)
    if count == 0:
        return
    arr = (_lib.DwProblem * count)()
    keep = []
    for i, prob in enumerate(problems):
        gy, x, gw = prob[:3]
        fold = prob[3] if len(prob) > 3 else None
        gy, x = _dev(gy, "gy"), _dev(x, "x")
        n, out_dim = gy.shape
        in_dim = x.shape[1]
        if x.shape[0] != n or tuple(gw.shape) != (out_dim, in_dim) or not gw.is_contiguous() or gw.dtype != torch.float32:
            raise _lib.LcrecError(f"linear_backward_weights: problem {i}: gy {tuple(gy.shape)}, x {tuple(x.shape)}, gw {tuple(gw.shape)}")
        if fold is None:
            arr[i] = _lib.DwProblem(gy.data_ptr(), x.data_ptr(), gw.data_ptr(), n, in_dim, out_dim, None, None, 0, int(splits))
        else:
            fs, fh = _vec(fold[0], "x_scale", in_dim), _vec(fold[1], "x_shift", in_dim)
            arr[i] = _lib.DwProblem(gy.data_ptr(), x.data_ptr(), gw.data_ptr(), n, in_dim, out_dim, fs.data_ptr(), fh.data_ptr(),
                                    int(bool(fold[2])), int(splits))
            keep += [fs, fh]
        keep += [gy, x]
    dev = problems[0][0].device
    with _on(dev):
        nbytes = lib.lcrec_linear_backward_weights_workspace(ctypes.cast(arr, ctypes.c_void_p), count)
        ws = _workspace(nbytes, dev)
        rc = lib.lcrec_linear_backward_weights(ctypes.cast(arr, ctypes.c_void_p), count, _ptr(ws), ws.numel(), _stream_ptr())
    _lib.check(rc, "lcrec_linear_backward_weights")


def linear_backward_splits(n, in_dim, out_dim):
    """Number of batch runs whose partial products make up gw (part of the arithmetic contract, include/lcrec.h)."""
    return int(_lib.load().lcrec_linear_backward_splits(n, in_dim, out_dim))


GEMM_ROLES = ("dx", "dw", "reduce", "forward")                 # LCREC_GEMMR_* of include/lcrec.h, in order
GEMM_FAMILIES = ("tile_body", "32x64", "reducer", "pp")        # LCREC_GEMMK_*


def _gemm_launches(buf, count):
    out = []
    for i in range(count):
        d = {name: getattr(buf[i], name) for name, _ in _lib.GemmLaunch._fields_}
        d["label"] = d["label"].decode()
        d["role"] = GEMM_ROLES[d["role"]]
        d["family"] = GEMM_FAMILIES[d["family"]]
        out.append(d)
    return out


def linear_forward_plan(n, in_dim, out_dim, cus=256):
    """The launches of linear_forward for [n][in_dim] -> [n][out_dim] on a device of `cus` compute units, in order (include/lcrec.h,
    lcrec_debug_linear_forward_plan): a list of dicts as linear_backward_plan gives them.  Host only: no GPU is needed.  Raises
    LcrecError for a shape the entry point refuses (this export leaves the library's last-error text alone)."""
    buf = (_lib.GemmLaunch * 4)()
    count = _lib.load().lcrec_debug_linear_forward_plan(int(n), int(in_dim), int(out_dim), int(cus), ctypes.addressof(buf), 4)
    if count < 0:
        err = _lib.LcrecError(f"lcrec_debug_linear_forward_plan({n}, {in_dim}, {out_dim}, {cus}) failed ({count}): "
                              "a shape lcrec_linear_forward refuses")
        err.code = count
        raise err
    return _gemm_launches(buf, count)


def linear_backward_plan(n, in_dim, out_dim, need_gx=True, need_gw=True):
    """The launches of linear_backward for these sizes, in order (include/lcrec.h, lcrec_debug_linear_backward_plan): a list of
    dicts of the fields of lcrec_gemm_launch, `role` and `family` as their names in GEMM_ROLES / GEMM_FAMILIES.  Host only: no
    GPU is needed.  Raises LcrecError for a shape the entry point refuses."""
    buf = (_lib.GemmLaunch * 3)()
    count = _lib.load().lcrec_debug_linear_backward_plan(int(n), int(in_dim), int(out_dim), int(bool(need_gx)), int(bool(need_gw)),
                                                         ctypes.addressof(buf), 3)
    if count < 0:
        _lib.check(count, "lcrec_debug_linear_backward_plan")
    return _gemm_launches(buf, count)


def linear_backward_weights_plan(problems):
    """What linear_backward_weights launches for `problems`, a list of (n, in_dim, out_dim, folded, splits): (products, reducers,
    (grid of the grouped launch, grid of the grouped reducer)) -- products[p] is problem p's share of the one launch, reducers the
    shares of the problems with more than one K-run, in problem order.  Host only (lcrec_debug_linear_backward_weights_plan)."""
    count = len(problems)
    arr = (_lib.DwProblem * max(count, 1))()
    for i, (n, in_dim, out_dim, folded, splits) in enumerate(problems):
        flag = 16 if folded else None                          # only whether a fold is given is read
        arr[i] = _lib.DwProblem(None, None, None, int(n), int(in_dim), int(out_dim), flag, flag, int(bool(folded)), int(splits))
    buf = (_lib.GemmLaunch * max(2 * count, 1))()
    grids = (ctypes.c_int * 2)()
    got = _lib.load().lcrec_debug_linear_backward_weights_plan(ctypes.cast(arr, ctypes.c_void_p), count, ctypes.addressof(buf), 2 * count,
                                                               grids)
    if got < 0:
        _lib.check(got, "lcrec_debug_linear_backward_weights_plan")
    launches = _gemm_launches(buf, got)
    return launches[:count], launches[count:], (int(grids[0]), int(grids[1]))


def linear_bn_forward_plan(n, in_dim, out_dim, pro, stats):
    """The launch of linear_bn_forward with an input fold (pro) and / or batch statistics (stats), as a dict of the fields of
    lcrec_gemm_launch; None when neither is asked for (the call is linear_forward's).  Host only
    (lcrec_debug_linear_bn_forward_plan)."""
    buf = (_lib.GemmLaunch * 1)()
    got = _lib.load().lcrec_debug_linear_bn_forward_plan(int(n), int(in_dim), int(out_dim), int(bool(pro)), int(bool(stats)),
                                                         ctypes.addressof(buf))
    if got < 0:
        _lib.check(got, "lcrec_debug_linear_bn_forward_plan")
    return _gemm_launches(buf, got)[0] if got else None


def flatten_codebooks(codebooks):
    """List of [K_l, e] tensors -> (flat fp32 tensor, [K_l]) in the layout lcrec_rq_assign expects."""
    ks = [int(c.shape[0]) for c in codebooks]
    cbs = [_dev(c, "codebook") for c in codebooks]
    # codebooks that already lie back to back in ONE storage (the training engine's flat parameter buffer) are passed as a
    # view of it: no concatenation launch per step.  Every tensor must belong to that storage and the view must fit in it --
    # separately allocated parameters can be neighbours in memory too, and a view past the end of a storage resizes it.
    base = cbs[0].untyped_storage()
    total = sum(c.numel() for c in cbs)
    if (len(cbs) > 1 and all(c.untyped_storage().data_ptr() == base.data_ptr() for c in cbs)
            and all(a.data_ptr() + a.numel() * 4 == b.data_ptr() for a, b in zip(cbs, cbs[1:]))
            and (cbs[0].storage_offset() + total) * 4 <= base.nbytes()):
        flat = cbs[0].new_empty(0).set_(base, cbs[0].storage_offset(), (total,), (1,))
        return flat, ks
    flat = cbs[0].reshape(-1) if len(cbs) == 1 else torch.cat([c.reshape(-1) for c in cbs])
    return flat, ks


def rq_assign(z, codebooks_flat, ks, want_xq=False, want_sse=False, want_resid=False, xq_init=None, audit=None,
              tie_tau=None, sse_out=None, idx_into=None):
    """ResidualVectorQuantizer.forward values with use_sk=False (rq.py:39-55).

    xq_init: optional [n, e] tensor that the x_q sum starts from (it is updated in place and returned).
    audit: optional dict that receives the near-tie audit outputs (include/lcrec.h): "margin" float32 [n, L] (top-2
    distance gap per level) and, with tie_tau, "neartie" int32 [n] (bit l set = level l is a near tie under tie_tau).
    idx_into: (matrix, col0) -- write the L index columns straight into columns col0 .. col0+L-1 of a wider contiguous int64
    [n, L_total] matrix (no copy afterwards); the returned idx is then that column block as a view.
    Returns (idx int64 [n, L], xq [n, e] | None, sse float64 [L] | None, resid [L+1, n, e] | None);
    resid[l] is the residual entering level l, resid[L] the residual left after the last level."""
    lib = _lib.load()
    z = _dev(z, "z")
    cb = _dev(codebooks_flat, "codebooks")
    n, e = z.shape
    L = len(ks)
    dev = z.device
    if idx_into is not None:
        matrix, col0 = idx_into
        if not (matrix.is_cuda and matrix.dtype == torch.int64 and matrix.dim() == 2 and matrix.is_contiguous()
                and matrix.shape[0] == n and 0 <= col0 and col0 + L <= matrix.shape[1]):
            raise _lib.LcrecError("idx_into must be (contiguous int64 [n, L_total] device matrix, first column)")
        idx, idx_ptr, idx_stride = matrix[:, col0:col0 + L], ctypes.c_void_p(matrix.data_ptr() + 8 * col0), int(matrix.shape[1])
    else:
        idx = torch.empty((n, L), dtype=torch.int64, device=dev)
        idx_ptr, idx_stride = _ptr(idx), L
    if xq_init is not None:
        xq = _dev(xq_init, "xq_init")
        if xq.data_ptr() != xq_init.data_ptr() or tuple(xq.shape) != (n, e):
            raise _lib.LcrecError("xq_init must be a contiguous [n, e] float32 device tensor")
    else:
        xq = torch.empty((n, e), dtype=torch.float32, device=dev) if want_xq else None
    sse = _sse_buffer(sse_out, L, dev, n) if want_sse else None
    resid = torch.empty((L + 1, n, e), dtype=torch.float32, device=dev) if want_resid else None
    margin, neartie, tau = _audit_buffers(audit, tie_tau, n, L, dev)
    karr = _ints(ks)
    with _on(dev):
        nbytes = lib.lcrec_rq_assign_workspace(n, e, karr, L)
        ws = _workspace(nbytes, dev)
        rc = lib.lcrec_rq_assign(_ptr(z), n, e, _ptr(cb), karr, L, idx_ptr, idx_stride, _ptr(xq), int(xq_init is not None),
                                 _ptr(sse), _ptr(resid), _ptr(margin), _ptr(neartie), tau, _ptr(ws), ws.numel(),
                                 _ptr(_ticket(dev)) if want_sse else None, _stream_ptr())
    _lib.check(rc, "lcrec_rq_assign")
    return idx, xq, sse, resid


def rq_assign_plan(n, e, ks, force_split=-1, force_threads=0, force_grid=0):
    """The form lcrec_rq_assign takes for [n, e] items and codebooks of `ks` codes, or the forced one (include/lcrec.h,
    lcrec_debug_rq_assign_plan), as a dict of the fields of lcrec_rq_plan: the per-launch fields as lists of `launches` entries,
    the per-level fields as lists of len(ks).  Host only: no GPU is needed.  LcrecError when the form cannot take the shape."""
    plan = _lib.RqPlan()
    L = len(ks)
    rc = _lib.load().lcrec_debug_rq_assign_plan(int(n), int(e), _ints(ks), L, int(force_split), int(force_threads), int(force_grid),
                                                ctypes.addressof(plan))
    _lib.check(rc, "lcrec_debug_rq_assign_plan")
    out = {}
    for name, ctype in _lib.RqPlan._fields_:
        value = getattr(plan, name)
        if name in ("l0", "l1", "rows", "lds_bytes"):
            out[name] = [int(v) for v in value[:plan.launches]]
        elif name in ("row_off", "blocks_per_wave", "idle_waves"):
            out[name] = [int(v) for v in value[:L]]
        else:
            out[name] = int(value)
    return out


def rq_assign_into(z, codebooks_flat, ks, idx, idx_stride, xq=None, xq_accumulate=False, sse=None, resid=None, margin=None,
                   neartie=None, tie_tau=0.0, ticket=True, force=None):
    """lcrec_rq_assign (force=None) or lcrec_debug_rq_assign (force = (split, threads, grid), include/lcrec.h) into buffers the
    caller owns -- each may be LARGER than the call needs, so that a test can look at what lies past the end: idx int64 with at
    least n * idx_stride elements, xq [>= n, e], sse float64 [>= L], resid float32 with at least (L + 1) * n * e elements
    (entry l at element l * n * e), margin float32 [>= n, L], neartie int32 [>= n].  ticket=False: the sums of squares are
    finished by a launch of their own.  Nothing is returned."""
    lib = _lib.load()
    z = _dev(z, "z")
    cb = _dev(codebooks_flat, "codebooks")
    n, e = z.shape
    L = len(ks)
    dev = z.device
    idx_stride = int(idx_stride)
    if cb.numel() != sum(int(k) for k in ks) * e:
        raise _lib.LcrecError(f"codebooks hold {cb.numel()} floats, {ks} x {e} need {sum(ks) * e}")
    for name, t, dtype, need in (("idx", idx, torch.int64, n * idx_stride), ("xq", xq, torch.float32, n * e), ("sse", sse, torch.float64, L),
                                 ("resid", resid, torch.float32, (L + 1) * n * e), ("margin", margin, torch.float32, n * L),
                                 ("neartie", neartie, torch.int32, n)):
        if t is None and name != "idx":
            continue
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev and t.dtype == dtype and t.is_contiguous()
                and t.numel() >= need):
            raise _lib.LcrecError(f"{name} must be a contiguous {dtype} tensor on z's device with at least {need} elements")
    if idx_stride < L:
        raise _lib.LcrecError(f"idx_stride {idx_stride} < L = {L}")
    karr = _ints(ks)
    with _on(dev):
        ws = _workspace(lib.lcrec_rq_assign_workspace(n, e, karr, L), dev)
        args = (_ptr(z), n, e, _ptr(cb), karr, L, _ptr(idx), idx_stride, _ptr(xq), int(bool(xq_accumulate)), _ptr(sse), _ptr(resid),
                _ptr(margin), _ptr(neartie), float(tie_tau), _ptr(ws), ws.numel(), _ptr(_ticket(dev, force=True)) if ticket else None,
                _stream_ptr())
        if force is None:
            rc, what = lib.lcrec_rq_assign(*args), "lcrec_rq_assign"
        else:
            rc, what = lib.lcrec_debug_rq_assign(*args, *[int(v) for v in force]), "lcrec_debug_rq_assign"
    _lib.check(rc, what)


def encode_plan(n, dims, ks, chunk_rows=0, pipelines=None):
    """How encode_assign walks n rows of an encoder of widths `dims` (in_dim, hidden sizes ..., e_dim) and where everything lies in
    its workspace (include/lcrec.h, lcrec_debug_encode_assign_plan): (dict of the fields of lcrec_encode_plan, list of one dict per
    chunk of the fields of lcrec_encode_chunk).  chunk_rows: 0 = the built-in chunk; pipelines: None = the current set_pipelines
    setting.  Host only: no GPU is needed.  LcrecError for arguments lcrec_encode_assign refuses."""
    lib = _lib.load()
    plan = _lib.EncodePlan()
    nl, L = len(dims) - 1, len(ks)
    P = _pipelines if pipelines is None else int(pipelines)
    darr, karr = _ints(dims), _ints(ks)
    rc = lib.lcrec_debug_encode_assign_plan(int(n), darr, nl, karr, L, int(chunk_rows), P, ctypes.addressof(plan), None, 0)
    _lib.check(rc, "lcrec_debug_encode_assign_plan")
    count = int(plan.n_chunks)
    buf = (_lib.EncodeChunk * max(count, 1))()
    rc = lib.lcrec_debug_encode_assign_plan(int(n), darr, nl, karr, L, int(chunk_rows), P, ctypes.addressof(plan), ctypes.addressof(buf), count)
    _lib.check(rc, "lcrec_debug_encode_assign_plan")
    out = {}
    for name, _ in _lib.EncodePlan._fields_:
        value = getattr(plan, name)
        out[name] = [int(v) for v in value] if name == "act_offset" else int(value)
    return out, [{name: int(getattr(buf[c], name)) for name, _ in _lib.EncodeChunk._fields_} for c in range(count)]


def encode_assign(x, weights, biases, codebooks_flat, ks, bn_scales=None, bn_shifts=None, want_latent=False,
                  want_xq=False, want_sse=False, audit=None, tie_tau=None, chunk_rows=None, into=None, workspace=None):
    """RQVAE.get_indices(xs, use_sk=False) (rqvae.py:68-72): encoder MLP + L-level argmin assignment.
    audit / tie_tau: as rq_assign (near-tie audit of the quantiser).

    weights[l] is nn.Linear.weight of encoder layer l ([out_l, in_l]); bn_scales/bn_shifts are
    per-layer folded eval-mode BatchNorm affines or None (the whole list, or single entries).
    chunk_rows: None = lcrec_encode_assign; a number = lcrec_debug_encode_assign with that chunk size (0: the built-in one) -- the
    same launch code, for the tests (encode_plan reports the walk).
    into: a dict of buffers the caller owns, written instead of fresh ones -- "idx" int64 (required), "latent", "xq", "margin"
    float32, "sse" float64, "neartie" int32, each contiguous on x's device with at least the elements the call writes (it may
    be LARGER, so that a test can look at what lies past the end); an output that is not in the dict is passed as NULL, and
    want_* / audit are not read.  workspace: a uint8 device tensor passed as the workspace as it is, its size included.
    Returns (idx, latent | None, xq | None, sse | None)."""
    lib = _lib.load()
    x = _dev(x, "x")
    nl = len(weights)
    ws_ = [_dev(w, "weight") for w in weights]
    bs_ = [_dev(b, "bias") for b in biases]
    scs = [None] * nl if bn_scales is None else [None if s is None else _dev(s, "bn_scale") for s in bn_scales]
    shs = [None] * nl if bn_shifts is None else [None if s is None else _dev(s, "bn_shift") for s in bn_shifts]
    cb = _dev(codebooks_flat, "codebooks")
    dims = [int(ws_[0].shape[1])] + [int(w.shape[0]) for w in ws_]
    if x.shape[1] != dims[0]:
        raise _lib.LcrecError(f"x has {x.shape[1]} features, encoder expects {dims[0]}")
    for l in range(nl):
        if ws_[l].shape[1] != dims[l]:
            raise _lib.LcrecError(f"encoder layer {l}: weight {tuple(ws_[l].shape)} does not chain")
    n, e, L, dev = x.shape[0], dims[-1], len(ks), x.device
    if into is None:
        idx = torch.empty((n, L), dtype=torch.int64, device=dev)
        latent = torch.empty((n, e), dtype=torch.float32, device=dev) if want_latent else None
        xq = torch.empty((n, e), dtype=torch.float32, device=dev) if want_xq else None
        sse = torch.zeros(L, dtype=torch.float64, device=dev) if want_sse else None
        margin, neartie, tau = _audit_buffers(audit, tie_tau, n, L, dev)
    else:
        sizes = {"idx": (torch.int64, n * L), "latent": (torch.float32, n * e), "xq": (torch.float32, n * e),
                 "sse": (torch.float64, L), "margin": (torch.float32, n * L), "neartie": (torch.int32, n)}
        if "idx" not in into or set(into) - set(sizes):
            raise _lib.LcrecError(f"into must hold idx and may hold {sorted(sizes)}, got {sorted(into)}")
        for name, t in into.items():
            dtype, need = sizes[name]
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev and t.dtype == dtype and t.is_contiguous()
                    and t.numel() >= need):
                raise _lib.LcrecError(f"into[{name!r}] must be a contiguous {dtype} tensor on x's device with at least {need} elements")
        idx, latent, xq, sse, margin, neartie = (into.get(k) for k in ("idx", "latent", "xq", "sse", "margin", "neartie"))
        tau = float(tie_tau or 0.0)
    if workspace is not None and not (isinstance(workspace, torch.Tensor) and workspace.is_cuda and workspace.device == dev
                                      and workspace.dtype == torch.uint8 and workspace.is_contiguous()):
        raise _lib.LcrecError("workspace must be a contiguous uint8 tensor on x's device")
    PA = ctypes.c_void_p * nl
    wp = PA(*[t.data_ptr() for t in ws_])
    bp = PA(*[t.data_ptr() for t in bs_])
    scp = None if bn_scales is None else PA(*[0 if t is None else t.data_ptr() for t in scs])    # (no list: the NULL array)
    shp = None if bn_shifts is None else PA(*[0 if t is None else t.data_ptr() for t in shs])
    darr, karr = _ints(dims), _ints(ks)
    with _on(dev):
        if workspace is not None:
            ws = workspace
        elif chunk_rows is None:
            ws = _workspace(lib.lcrec_encode_assign_workspace(n, darr, nl, karr, L), dev)
        else:
            ws = _workspace(lib.lcrec_debug_encode_assign_workspace(n, darr, nl, karr, L, int(chunk_rows)), dev)
        args = (_ptr(x), n, darr, nl, wp, bp, scp, shp, _ptr(cb), karr, L, _ptr(idx), _ptr(latent), _ptr(xq), _ptr(sse),
                _ptr(margin), _ptr(neartie), tau, _ptr(ws), ws.numel(), _context(dev), _stream_ptr())
        if chunk_rows is None:
            rc, what = lib.lcrec_encode_assign(*args), "lcrec_encode_assign"
        else:
            rc, what = lib.lcrec_debug_encode_assign(*args, int(chunk_rows)), "lcrec_debug_encode_assign"
    _lib.check(rc, what)
    return idx, latent, xq, sse


def _idx_col(idx, n):
    """(tensor, element stride) for an int64 index column: a [n] vector or a column view of [n, L]."""
    if not idx.is_cuda or idx.dtype != torch.int64 or idx.dim() != 1 or idx.shape[0] != n:
        raise _lib.LcrecError("idx must be an int64 device vector of length n (a column view is fine)")
    return idx, int(idx.stride(0)) if n > 1 else 1


def sinkhorn_assign(resid, codebook, epsilon, iters, group_offsets=None, out=None):
    """use_sk branch of VectorQuantizer.forward (vq.py:76-83): int64 [n] Sinkhorn assignments.

    group_offsets: host sequence of ascending row offsets delimiting independent problems
    (default: one group = all rows, the training case).  `out` may be a column view of [n, L]."""
    lib = _lib.load()
    resid = _dev(resid, "resid")
    codebook = _dev(codebook, "codebook")
    n, e = resid.shape
    K = codebook.shape[0]
    import numpy as np
    offs = np.ascontiguousarray([0, n] if group_offsets is None else group_offsets, dtype=np.int64)
    G = len(offs) - 1
    if out is None:
        out = torch.zeros(n, dtype=torch.int64, device=resid.device)
    out, stride = _idx_col(out, n)
    oarr = offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    with _on(resid.device):
        nbytes = lib.lcrec_sinkhorn_assign_workspace(n, K, oarr, G)
        ws = _workspace(nbytes, resid.device)
        rc = lib.lcrec_sinkhorn_assign(_ptr(resid), n, e, _ptr(codebook), K, oarr, G, float(epsilon), int(iters),
                                       _ptr(out), stride, _ptr(ws), ws.numel(), _context(resid.device),
                                       _ptr(_ticket(resid.device)), _stream_ptr())
    _lib.check(rc, "lcrec_sinkhorn_assign")
    if G > 0 and int(np.diff(offs).max()) * K > 16384:
        # the one-launch solver for batch-sized problems poisons its output with -1 if its (bounded)
        # grid barrier ever times out; turn that into an error rather than training on garbage --
        # here and now, or (inside deferred_checks(), the trainer's epoch loop) when the block ends,
        # so that a training step has no host synchronisation of its own
        # (a single problem: the kernel poisons EVERY row -- whoever timed out set the flag all workgroups read before they
        # write -- so the first row tells; several groups: only the rows of the group that took that path)
        if _deferred is not None and _deferred_raw and G == 1:
            # the caller folds the test into a kernel of its own (lcrec_step_losses' poison_probe): hand it the element to look at
            _deferred.append((_POISON_MSG, out[0:1]))
            return out
        bad = (out[0] < 0) if G == 1 else (out < 0).any()
        if _deferred is not None:
            _deferred.append(("lcrec_sinkhorn_assign: grid barrier timed out (device oversubscribed?); "
                              "set LCREC_SINKHORN_PERSISTENT=0 to use the multi-launch solver", bad))
        elif bool(bad):
            raise _lib.LcrecError("lcrec_sinkhorn_assign: grid barrier timed out (device oversubscribed?); "
                                  "set LCREC_SINKHORN_PERSISTENT=0 to use the multi-launch solver")
    return out


SK_FORMS = {0: "production's choice", 1: "scaling, XCD-local sets", 2: "scaling, agent scope", 3: "persistent", 4: "multi-launch"}


def sinkhorn_plan(B, K, iters, form=0):
    """The solver lcrec_sinkhorn_assign's batch-sized path takes for a lone [B, K] problem, or the forced `form` (SK_FORMS),
    as a dict of the fields of lcrec_sinkhorn_plan (include/lcrec.h).  Host only: no GPU is needed.  LcrecError when the
    form cannot take the shape."""
    plan = _lib.SinkhornPlan()
    rc = _lib.load().lcrec_debug_sinkhorn_plan(int(B), int(K), int(iters), int(form), ctypes.addressof(plan))
    _lib.check(rc, "lcrec_debug_sinkhorn_plan")
    return {name: int(getattr(plan, name)) for name, _ in _lib.SinkhornPlan._fields_}


def sinkhorn_debug(resid, codebook, epsilon, iters, form=0, out=None, runner_out=None, ratio_out=None):
    """lcrec_debug_sinkhorn_batch: all rows as one problem through the batch-sized solver `form` (SK_FORMS), with
    production's kernels.  Returns (idx int64 [n], runner-up column int64 [n], second / best double [n], form that ran).
    `out` may be a column view of [n, L]; outputs that are passed in keep whatever the solver does not write."""
    lib = _lib.load()
    resid = _dev(resid, "resid")
    codebook = _dev(codebook, "codebook")
    n, e = resid.shape
    K = codebook.shape[0]
    dev = resid.device
    if out is None:
        out = torch.zeros(n, dtype=torch.int64, device=dev)
    out, stride = _idx_col(out, n)
    if runner_out is None:
        runner_out = torch.full((n,), -1, dtype=torch.int64, device=dev)
    if ratio_out is None:
        ratio_out = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    for t, dt in ((runner_out, torch.int64), (ratio_out, torch.float64)):
        if not t.is_cuda or t.dtype != dt or t.shape != (n,) or not t.is_contiguous():
            raise _lib.LcrecError("runner_out / ratio_out must be contiguous device vectors of length n (int64 / float64)")
    nbytes = sinkhorn_plan(n, K, iters, form)["workspace_bytes"]
    ran = ctypes.c_int(0)
    with _on(dev):
        ws = _workspace(nbytes, dev)
        rc = lib.lcrec_debug_sinkhorn_batch(_ptr(resid), n, e, _ptr(codebook), K, float(epsilon), int(iters), _ptr(out), stride,
                                            _ptr(ws), ws.numel(), _ptr(_ticket(dev)), _stream_ptr(), int(form),
                                            _ptr(runner_out), _ptr(ratio_out), ctypes.byref(ran))
    _lib.check(rc, "lcrec_debug_sinkhorn_batch")
    return out, runner_out, ratio_out, ran.value


SK_TABLE_TRANSPORTS = {0: "none", 1: "argument", 2: "ring", 3: "synchronous"}


def sinkhorn_groups_plan(K, group_offsets, has_context=True, routes=False):
    """The launches lcrec_sinkhorn_assign makes for a group table (lcrec_debug_sinkhorn_groups_plan, the function it launches by),
    as a dict of the fields of lcrec_sinkhorn_groups_plan (include/lcrec.h); "cls" is a list of five dicts.  routes=True adds
    "routes": per group (class, position in the reordered table, slab offset).  Host only: no GPU is needed."""
    import numpy as np
    offs = np.ascontiguousarray(group_offsets, dtype=np.int64)
    G = len(offs) - 1
    plan = _lib.SinkhornGroupsPlan()
    route = (_lib.SinkhornGroupRoute * max(G, 1))() if routes else None
    rc = _lib.load().lcrec_debug_sinkhorn_groups_plan(int(K), offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), G, int(bool(has_context)),
                                                      ctypes.addressof(plan), ctypes.addressof(route) if routes else None)
    _lib.check(rc, "lcrec_debug_sinkhorn_groups_plan")
    out = {name: int(getattr(plan, name)) for name, _ in _lib.SinkhornGroupsPlan._fields_ if name != "cls"}
    out["cls"] = [{name: (getattr(c, name).decode() if getattr(c, name) else None) if name == "label" else int(getattr(c, name))
                   for name, _ in _lib.SinkhornClassPlan._fields_} for c in plan.cls]
    if routes:
        out["routes"] = [(int(route[g].cls), int(route[g].position), int(route[g].slab_offset)) for g in range(G)]
    return out


def sinkhorn_groups_debug(resid, codebook, epsilon, iters, group_offsets, out=None, runner_out=None, ratio_out=None, context=True):
    """lcrec_debug_sinkhorn_groups: lcrec_sinkhorn_assign's launch code with the runner-up column and second / best of every
    grouped row.  Returns (idx int64 [n], runner int64 [n], ratio double [n]); rows of no group keep what the outputs held (-1 /
    NaN when they are made here).  context=False: the call is made with a NULL context."""
    import numpy as np
    lib = _lib.load()
    resid = _dev(resid, "resid")
    codebook = _dev(codebook, "codebook")
    n, e = resid.shape
    K = codebook.shape[0]
    dev = resid.device
    offs = np.ascontiguousarray(group_offsets, dtype=np.int64)
    G = len(offs) - 1
    if out is None:
        out = torch.full((n,), -1, dtype=torch.int64, device=dev)
    out, stride = _idx_col(out, n)
    if runner_out is None:
        runner_out = torch.full((n,), -1, dtype=torch.int64, device=dev)
    if ratio_out is None:
        ratio_out = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    for t, dt in ((runner_out, torch.int64), (ratio_out, torch.float64)):
        if not t.is_cuda or t.dtype != dt or t.shape != (n,) or not t.is_contiguous():
            raise _lib.LcrecError("runner_out / ratio_out must be contiguous device vectors of length n (int64 / float64)")
    oarr = offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    with _on(dev):
        nbytes = lib.lcrec_sinkhorn_assign_workspace(n, K, oarr, G)
        ws = _workspace(nbytes, dev)
        rc = lib.lcrec_debug_sinkhorn_groups(_ptr(resid), n, e, _ptr(codebook), K, oarr, G, float(epsilon), int(iters), _ptr(out), stride,
                                             _ptr(ws), ws.numel(), _context(dev) if context else None, _ptr(_ticket(dev)), _stream_ptr(),
                                             _ptr(runner_out), _ptr(ratio_out))
    _lib.check(rc, "lcrec_debug_sinkhorn_groups")
    return out, runner_out, ratio_out


_deferred = None
_deferred_raw = False
_POISON_MSG = ("lcrec_sinkhorn_assign: grid barrier timed out (device oversubscribed?); "
               "set LCREC_SINKHORN_PERSISTENT=0 to use the multi-launch solver")


class deferred_checks:
    """Context in which result checks that need a device->host read (the Sinkhorn poison flag) are
    collected as device booleans and evaluated together at exit, or every `every` collected checks."""

    def __init__(self, every=256, raw=False):
        """raw: single-problem Sinkhorn calls append (message, int64 [1] view of their first assignment) instead of a device
        boolean -- no compare launch; the caller (engine.py) drains them and tests the element itself (< 0 = poisoned)."""
        self.every = every
        self.raw = raw

    def __enter__(self):
        global _deferred, _deferred_raw
        self._outer = (_deferred, _deferred_raw)
        _deferred, _deferred_raw = [], self.raw
        return self

    def flush(self):
        global _deferred
        pending, _deferred = _deferred, []
        if pending and bool(torch.stack([b for _, b in pending]).any()):
            for msg, b in pending:
                if bool(b):
                    raise _lib.LcrecError(msg)

    def poll(self):
        if _deferred is not None and len(_deferred) >= self.every:
            self.flush()

    @staticmethod
    def drain():
        """Hand the collected (message, device bool) pairs to the caller without evaluating them (a graph capture folds
        them into a device-side flag instead of reading them back)."""
        global _deferred
        pending, _deferred = (_deferred or []), []
        return pending

    def __exit__(self, exc_type, exc, tb):
        global _deferred, _deferred_raw
        try:
            if exc_type is None and not self.raw:
                self.flush()
        finally:
            _deferred, _deferred_raw = self._outer
        return False


def _sse_buffer(sse_out, L, dev, n=1):
    """float64 [L] for a kernel's per-level sums of squares: the caller's view (a slice of its own buffer) or a new one.
    The kernels write every slot, so there is no zero fill -- except for an empty batch, which launches nothing."""
    if sse_out is None:
        return (torch.zeros if n == 0 else torch.empty)(L, dtype=torch.float64, device=dev)
    if not (sse_out.is_cuda and sse_out.dtype == torch.float64 and sse_out.is_contiguous() and sse_out.numel() == L):
        raise _lib.LcrecError(f"sse_out must be a contiguous float64 [{L}] device tensor")
    if n == 0:
        sse_out.zero_()
    return sse_out


def rq_apply_level(resid, codebook, idx, xq=None, want_sse=False, sse_out=None):
    """Gather + STE + residual update of one level for given indices (vq.py:87-95, rq.py:47-48).

    xq: None (start a new x_q sum) or the running [n, e] sum, updated in place.
    Returns (xq, resid_next, sse float64 [1] | None)."""
    lib = _lib.load()
    resid = _dev(resid, "resid")
    codebook = _dev(codebook, "codebook")
    n, e = resid.shape
    K = codebook.shape[0]
    idx, stride = _idx_col(idx, n)
    accumulate = xq is not None
    if xq is None:
        xq = torch.empty((n, e), dtype=torch.float32, device=resid.device)
    elif not (xq.is_cuda and xq.is_contiguous() and xq.dtype == torch.float32 and tuple(xq.shape) == (n, e)):
        raise _lib.LcrecError("xq must be a contiguous [n, e] float32 device tensor")
    nxt = torch.empty_like(resid)
    sse = _sse_buffer(sse_out, 1, resid.device, n) if want_sse else None
    with _on(resid.device):
        ws = _workspace(8192, resid.device)
        rc = lib.lcrec_rq_apply_level(_ptr(resid), n, e, _ptr(codebook), K, _ptr(idx), stride, _ptr(xq),
                                      int(accumulate), _ptr(nxt), _ptr(sse), _ptr(ws), ws.numel(),
                                      _ptr(_ticket(resid.device)) if want_sse else None, _stream_ptr())
    _lib.check(rc, "lcrec_rq_apply_level")
    return xq, nxt, sse


def code_stats(idx, resid, K):
    """count [K] and per-code residual sums [K, e] in item order (index_improve vq.py:151-167)."""
    lib = _lib.load()
    resid = _dev(resid, "resid")
    n, e = resid.shape
    idx, stride = _idx_col(idx, n)
    count = torch.empty(K, dtype=torch.float32, device=resid.device)
    total = torch.empty((K, e), dtype=torch.float32, device=resid.device)
    with _on(resid.device):
        rc = lib.lcrec_code_stats(_ptr(idx), stride, _ptr(resid), n, e, K, _ptr(count), _ptr(total), _stream_ptr())
    _lib.check(rc, "lcrec_code_stats")
    return count, total


def code_stats_levels(idx, resid_in, ks, codebooks=None, grads_out=None, scale=0.0, weight=0.0):
    """[(count, sum)] for every level of an [n, L] index matrix in one launch (lcrec_code_stats_levels); with codebooks and
    grads_out (lists of [K_l, e] tensors) the codebook gradients (scale * (count*C - sum)) * weight are written too."""
    lib = _lib.load()
    if not (idx.is_cuda and idx.dtype == torch.int64 and idx.dim() == 2 and idx.is_contiguous()):
        raise _lib.LcrecError("idx must be a contiguous int64 [n, L] device tensor")
    n, L = idx.shape
    resid = [_dev(r, "resid") for r in resid_in]
    e = resid[0].shape[1]
    dev = idx.device
    counts = [torch.empty(int(k), dtype=torch.float32, device=dev) for k in ks]
    sums = [torch.empty((int(k), e), dtype=torch.float32, device=dev) for k in ks]
    PA = ctypes.c_void_p * L
    fused = codebooks is not None
    cbs = [_dev(c, "codebook") for c in codebooks] if fused else None
    with _on(dev):
        rc = lib.lcrec_code_stats_levels(_ptr(idx), PA(*[r.data_ptr() for r in resid]), n, e, _ints(ks), L,
                                         PA(*[c.data_ptr() for c in counts]), PA(*[t.data_ptr() for t in sums]),
                                         PA(*[c.data_ptr() for c in cbs]) if fused else None,
                                         PA(*[g.data_ptr() for g in grads_out]) if fused else None, float(scale), float(weight),
                                         _stream_ptr())
    _lib.check(rc, "lcrec_code_stats_levels")
    return list(zip(counts, sums))


def ema_update(ema_count, ema_sum, codebook, count, total, decay, eps, skip_flag=None):
    """In-place EMA step of index_improve vq.py:155-184 on three contiguous fp32 device tensors.  skip_flag: a device
    bool/uint8 scalar; when set the call changes nothing (lcrec_ema_update)."""
    lib = _lib.load()
    for name, t in (("ema_count", ema_count), ("ema_sum", ema_sum), ("codebook", codebook)):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32):
            raise _lib.LcrecError(f"{name} must be a contiguous float32 device tensor (it is updated in place)")
    count, total = _dev(count, "count"), _dev(total, "sum")
    K, e = codebook.shape
    alpha = 1 - decay                  # the reference's python doubles, rounded to fp32 at the ABI
    keep = 1 - (1 - decay)
    with _on(codebook.device):
        rc = lib.lcrec_ema_update(_ptr(ema_count), _ptr(ema_sum), _ptr(codebook), _ptr(count), _ptr(total), K, e,
                                  decay, alpha, keep, eps, _ptr(skip_flag), _stream_ptr())
    _lib.check(rc, "lcrec_ema_update")


def collision_groups(idx, ks, want_groups=True):
    """Tuple collisions of an int64 [n, L] index matrix (trainer.py:139-150, generate_indices.py:18-42).

    Returns dict(unique, max_count, collision_rate, n_groups) and, with want_groups, the groups in
    get_collision_item's order (first occurrence of the tuple; ids ascending inside a group):
      want_groups=True      `groups`: a list of item-id lists (small inputs, tests, the reference's helper API);
      want_groups="device"  `members` int64 [items in groups] and `offsets` int64 [n_groups + 1] device
                            tensors -- group g = members[offsets[g]:offsets[g+1]] -- no Python lists."""
    lib = _lib.load()
    if not (idx.is_cuda and idx.dtype == torch.int64 and idx.dim() == 2):
        raise _lib.LcrecError("idx must be an int64 [n, L] device tensor")
    idx = idx.contiguous()
    n, L = idx.shape
    dev = idx.device
    counters = torch.zeros(4, dtype=torch.int64, device=dev)
    members = torch.empty(max(n, 1), dtype=torch.int64, device=dev) if want_groups else None
    offsets = torch.empty(n // 2 + 2, dtype=torch.int64, device=dev) if want_groups else None
    karr = _ints(ks)
    with _on(dev):
        nbytes = lib.lcrec_collision_groups_workspace(n, L)
        ws = _workspace(nbytes, dev)
        rc = lib.lcrec_collision_groups(_ptr(idx), n, L, karr, _ptr(members), _ptr(offsets), _ptr(counters), _ptr(ws),
                                        ws.numel(), _stream_ptr())
    _lib.check(rc, "lcrec_collision_groups")
    c = counters.tolist()
    out = {"unique": c[0], "max_count": c[3], "collision_rate": (n - c[0]) / n if n else 0.0}
    if want_groups:
        out["n_groups"] = c[1]
        if want_groups == "device":
            out["members"] = members[: c[2]]
            out["offsets"] = offsets[: c[1] + 1]
        else:
            offs = offsets[: c[1] + 1].tolist()
            mem = members[: c[2]].tolist()
            out["groups"] = [mem[offs[g]:offs[g + 1]] for g in range(c[1])]
    return out


def collision_plan(n, ks):
    """What collision_groups decides on the host for n items of len(ks) levels (include/lcrec.h, lcrec_debug_collision_plan), as a
    dict of the fields of lcrec_collision_plan, `bits` a list of one entry per level.  Host only: no GPU is needed."""
    plan = _lib.CollisionPlan()
    rc = _lib.load().lcrec_debug_collision_plan(int(n), len(ks), _ints(ks), ctypes.addressof(plan))
    _lib.check(rc, "lcrec_debug_collision_plan")
    out = {name: int(getattr(plan, name)) for name, _ in _lib.CollisionPlan._fields_ if name != "bits"}
    out["bits"] = list(plan.bits)[:len(ks)]
    return out


def _inplace_idx(idx):
    """(n, L) of an idx that a pass updates in place."""
    if not (isinstance(idx, torch.Tensor) and idx.is_cuda and idx.dtype == torch.int64 and idx.dim() == 2 and idx.is_contiguous()):
        raise _lib.LcrecError("idx must be a contiguous int64 [n, L] device tensor (it is updated in place)")
    return idx.shape


def _frozen_count(n_frozen, n, L):
    n_frozen = int(n_frozen)
    if not 0 <= n_frozen <= n:
        raise _lib.LcrecError(f"n_frozen={n_frozen} does not go with idx {(n, L)} (0 .. {n})")
    return n_frozen


def _group_table(members, offsets, what=""):
    """A (members, offsets) table in collision_groups' "device" layout, both contiguous; `what` names the table in the message."""
    for name, t in (("members", members), ("offsets", offsets)):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64 and t.dim() == 1):
            raise _lib.LcrecError(f"{what}{name} must be an int64 [*] device tensor")
    return members.contiguous(), offsets.contiguous()


def _counters_out(counters_out, device, count=2):
    """The counters of a pass -- the (moved, unresolved) pair of a nearest-free pass, or the `count` = 4 of a beam finishing pass --
    as the caller's own int64 [count] tensor on `device`, or (None) a fresh one."""
    if counters_out is None:
        return torch.empty(count, dtype=torch.int64, device=device)
    if not (isinstance(counters_out, torch.Tensor) and counters_out.device == device and counters_out.dtype == torch.int64
            and tuple(counters_out.shape) == (count,) and counters_out.is_contiguous()):
        raise _lib.LcrecError(f"counters_out must be a contiguous int64 [{count}] tensor on idx's device ({device})")
    return counters_out


def _is_workspace(workspace, device):
    """whether `workspace` can go to the library as it is: a contiguous uint8 tensor on `device`"""
    return (isinstance(workspace, torch.Tensor) and workspace.device == device and workspace.dtype == torch.uint8
            and workspace.is_contiguous())


def _own_workspace(workspace, device, need, query):
    """A workspace the caller owns, passed to the library as it is: a contiguous uint8 tensor on `device` of at least the `need`
    bytes that `query` (the entry's workspace function) states for this call."""
    if not _is_workspace(workspace, device):
        raise _lib.LcrecError(f"workspace must be a contiguous uint8 tensor on the call's device ({device})")
    if workspace.numel() < need:
        raise _lib.LcrecError(f"workspace of {workspace.numel()} bytes, {int(need)} needed ({query})")
    return workspace


def finish_nearest_free(idx, resid_last, cb_last, ks, members, offsets, counters_out=None):
    """The nearest-free-code finishing pass (lcrec_finish_nearest_free of include/lcrec.h, which states the rule): every item of
    a bucket -- `members[offsets[b]:offsets[b+1]]`, the items sharing idx[:, :L-1], ids ascending -- that still shares its last
    code with another gets the nearest free last-level code; the holder nearest to a shared code keeps it.  Beyond the reference,
    which stops after its conflict rounds (generate_indices.py:107-136).

    idx int64 [n, L] is updated IN PLACE (last column, movers only); resid_last float32 [n, e] is the residual entering the last
    level, cb_last float32 [K_last, e]; members / offsets are int64 device tensors in collision_groups' "device" layout.
    Returns (moved, unresolved); afterwards exactly `unresolved` items of the listed buckets still collide.
    counters_out: an int64 [2] tensor on idx's device that receives (moved, unresolved) instead; the binding then reads nothing
    back and returns None -- the form of the call that a graph capture can record (it allocates nothing and never waits)."""
    return _nearest_free(None, idx, resid_last, cb_last, ks, members, offsets, counters_out)


def extend_nearest_free(idx, n_frozen, resid_new, cb_last, ks, members, offsets, counters_out=None):
    """The frozen-aware nearest-free-code pass (lcrec_extend_nearest_free of include/lcrec.h, which states the rule): items
    0 .. n_frozen-1 of idx never change; a new item that shares its tuple with a frozen one moves to the nearest free last-level
    code of its bucket, and among new items only the holder nearest to a shared code keeps it.

    idx int64 [n, L] is updated IN PLACE (last column, new movers only); resid_new float32 [n - n_frozen, e] holds the residual
    entering the last level of the NEW items only (row i - n_frozen for item i); cb_last float32 [K_last, e]; members / offsets
    are int64 device tensors in collision_groups' "device" layout over all n items.  Returns (moved, unresolved).
    counters_out: as finish_nearest_free -- an int64 [2] device tensor that receives the pair; nothing is read back, None is returned."""
    return _nearest_free(n_frozen, idx, resid_new, cb_last, ks, members, offsets, counters_out)


def _nearest_free(n_frozen, idx, resid, cb_last, ks, members, offsets, counters_out):
    """finish_nearest_free (n_frozen None) and extend_nearest_free: one set of checks; the entry differs, and the name and the
    number of the residual rows it takes"""
    lib = _lib.load()
    n, L = _inplace_idx(idx)
    entry, name, rows, per_new = "lcrec_finish_nearest_free", "resid_last", n, ""
    if n_frozen is not None:
        n_frozen = _frozen_count(n_frozen, n, L)
        entry, name, rows = "lcrec_extend_nearest_free", "resid_new", n - n_frozen
        per_new = f" and n_frozen={n_frozen}: one row per new item"
    resid, cb_last = _dev(resid, name), _dev(cb_last, "cb_last")
    members, offsets = _group_table(members, offsets)
    if resid.dim() != 2 or cb_last.dim() != 2 or resid.shape[0] != rows or resid.shape[1] != cb_last.shape[1]:
        raise _lib.LcrecError(f"{name} {tuple(resid.shape)} and cb_last {tuple(cb_last.shape)} do not go with idx {(n, L)}{per_new}")
    if len(ks) != L or int(ks[-1]) != cb_last.shape[0]:
        raise _lib.LcrecError(f"ks {list(ks)} does not go with idx [*, {L}] and cb_last [{cb_last.shape[0]}, *]")
    n_buckets = max(offsets.numel() - 1, 0)
    dev = idx.device
    counters = _counters_out(counters_out, dev)
    with _on(dev):
        head = (_ptr(idx), n) + (() if n_frozen is None else (n_frozen,))
        rc = getattr(lib, entry)(*head, L, _ints(ks), _ptr(resid), resid.shape[1], _ptr(cb_last), _ptr(members), _ptr(offsets),
                                 n_buckets, _ptr(counters), _stream_ptr())
    _lib.check(rc, entry)
    if counters_out is not None:
        return None
    moved, unresolved = counters.tolist()
    return moved, unresolved


def spill_nearest_free(idx, n_frozen, resid_prev, resid_last, cb_prev, cb_last, ks, tuple_groups, super_groups, counters_out=None,
                       workspace=None):
    """Spill to a sibling bucket (lcrec_spill_nearest_free of include/lcrec.h, which states the rule): every item that still
    shares its tuple after finish_nearest_free / extend_nearest_free -- its bucket has more items than the last level has codes --
    takes the nearest code of level L-2 whose row has a free cell in its super-bucket (the items sharing idx[:, :L-2]) and the
    nearest free last-level code there.  Items 0 .. n_frozen-1 never change.

    idx int64 [n, L], L >= 2, is updated IN PLACE (columns L-2 and L-1 of the items that move); resid_prev / resid_last float32
    [n - n_frozen, e] are the residuals entering levels L-2 / L-1 of the NEW items (row i - n_frozen for item i); cb_prev
    [ks[L-2], e], cb_last [ks[L-1], e]; tuple_groups / super_groups are (members, offsets) pairs of int64 device tensors in
    collision_groups' "device" layout: the groups of the full idx, and of idx[:, :L-2].  Returns (moved, unresolved).
    counters_out: as finish_nearest_free -- an int64 [2] device tensor that receives the pair; nothing is read back, None is returned.
    workspace: a uint8 device tensor of at least lcrec_spill_nearest_free_workspace(n) bytes, passed as the workspace as it is, its
    size included; None: the binding's own grow-only buffer of the stream, which a captured graph must not point into."""
    lib = _lib.load()
    n, L = _inplace_idx(idx)
    n_frozen = _frozen_count(n_frozen, n, L)
    resid_prev, resid_last = _dev(resid_prev, "resid_prev"), _dev(resid_last, "resid_last")
    cb_prev, cb_last = _dev(cb_prev, "cb_prev"), _dev(cb_last, "cb_last")
    tables = []
    for what, pair in (("tuple_groups", tuple_groups), ("super_groups", super_groups)):
        if not (isinstance(pair, (tuple, list)) and len(pair) == 2):
            raise _lib.LcrecError(f"{what} must be a (members, offsets) pair")
        tables.append(_group_table(*pair, what=f"{what}: "))
    e = cb_last.shape[1] if cb_last.dim() == 2 else -1
    for name, t in (("resid_prev", resid_prev), ("resid_last", resid_last)):
        if t.dim() != 2 or t.shape[0] != n - n_frozen or t.shape[1] != e:
            raise _lib.LcrecError(f"{name} {tuple(t.shape)} does not go with idx {(n, L)}, n_frozen={n_frozen} and cb_last "
                                  f"{tuple(cb_last.shape)}: one row per new item")
    if L < 2:
        raise _lib.LcrecError(f"spill_nearest_free: L={L}: the pass moves an item one level above the last, it needs two levels")
    if len(ks) != L or cb_prev.dim() != 2 or tuple(cb_prev.shape) != (int(ks[-2]), e) or int(ks[-1]) != cb_last.shape[0]:
        raise _lib.LcrecError(f"ks {list(ks)} does not go with idx [*, {L}], cb_prev {tuple(cb_prev.shape)} and cb_last "
                              f"{tuple(cb_last.shape)}")
    (tmem, toff), (smem, soff) = tables
    dev = idx.device
    counters = _counters_out(counters_out, dev)
    need = lib.lcrec_spill_nearest_free_workspace(n)
    if workspace is not None:
        workspace = _own_workspace(workspace, dev, need, "lcrec_spill_nearest_free_workspace")
    with _on(dev):
        ws = workspace if workspace is not None else _workspace(need, dev)
        rc = lib.lcrec_spill_nearest_free(_ptr(idx), n, n_frozen, L, _ints(ks), _ptr(resid_prev), _ptr(resid_last), e, _ptr(cb_prev),
                                          _ptr(cb_last), _ptr(tmem), _ptr(toff), max(toff.numel() - 1, 0), _ptr(smem), _ptr(soff),
                                          max(soff.numel() - 1, 0), _ptr(counters), _ptr(ws), ws.numel(), _stream_ptr())
    _lib.check(rc, "lcrec_spill_nearest_free")
    if counters_out is not None:
        return None
    moved, unresolved = counters.tolist()
    return moved, unresolved


def finish_beam(idx, ks, members, offsets, err_held, cand, cand_err, counters_out=None, choice_out=None, workspace=None):
    """The beam finishing pass (lcrec_finish_beam of include/lcrec.h, which states the rule): of every shared tuple -- group
    `members[offsets[g]:offsets[g+1]]`, ids ascending -- the member with the smallest err_held keeps it and the others move, in
    synchronous rounds, to the first candidate of their own list that no item holds and no other mover has taken.

    idx int64 [n, L] is updated IN PLACE (the rows of the items that move); members / offsets are int64 device tensors in
    collision_groups' "device" layout over the full idx; err_held float32 [M], cand int64 [M, width, L] and cand_err float32
    [M, width] go by member POSITION (M = members.numel()): rq_audit's err of the held tuple and rq_beam's tuples and err of that
    item's latent.  width in BEAM_WIDTHS.
    Returns (choice int32 [M]: -1 keeper or no part, b >= 0 moved to candidate b, -2 unresolved; dict of movers, moved, unresolved,
    rounds).  counters_out: an int64 [4] tensor on idx's device that receives the four counters instead; the binding then reads
    nothing back and returns (choice, None) -- the form of the call that a graph capture can record, given choice_out and workspace
    too.  choice_out: an int32 tensor of at least M elements, written instead of a fresh one (it may be LARGER, so that a test can
    look at what lies past the end).  workspace: a uint8 device tensor of at least lcrec_finish_beam_workspace's bytes, passed as
    the workspace as it is, its size included; None: the binding's own grow-only buffer of the stream."""
    return _finish_beam(None, idx, ks, members, offsets, err_held, cand, cand_err, counters_out, choice_out, workspace)


def extend_finish_beam(idx, n_frozen, ks, members, offsets, err_held, cand, cand_err, counters_out=None, choice_out=None,
                       workspace=None):
    """The frozen-aware beam finishing pass (lcrec_extend_finish_beam of include/lcrec.h, which states the rule): finish_beam with
    items 0 .. n_frozen-1 of idx frozen.  They never move; a new item that shares its tuple with a frozen one moves, and among new
    holders only the one with the smallest err_held keeps the tuple.  The positions of frozen members in err_held, cand and
    cand_err are never read: they may hold anything.

    Arguments, return value and the capturable form (counters_out, choice_out and workspace given) as finish_beam; members / offsets
    list the groups over all n items; the workspace query is lcrec_extend_finish_beam_workspace."""
    return _finish_beam(n_frozen, idx, ks, members, offsets, err_held, cand, cand_err, counters_out, choice_out, workspace)


def _finish_beam(n_frozen, idx, ks, members, offsets, err_held, cand, cand_err, counters_out, choice_out, workspace):
    """finish_beam (n_frozen None) and extend_finish_beam: one set of checks, the entry and its workspace query differ"""
    lib = _lib.load()
    n, L = _inplace_idx(idx)
    entry = "lcrec_finish_beam" if n_frozen is None else "lcrec_extend_finish_beam"
    if n_frozen is not None:
        n_frozen = _frozen_count(n_frozen, n, L)
    dev = idx.device
    members, offsets = _group_table(members, offsets)
    err_held, cand_err = _dev(err_held, "err_held"), _dev(cand_err, "cand_err")
    M = members.numel()
    if not (isinstance(cand, torch.Tensor) and cand.is_cuda and cand.dtype == torch.int64 and cand.dim() == 3 and cand.is_contiguous()
            and cand.shape[0] == M and cand.shape[2] == L):
        raise _lib.LcrecError(f"cand must be a contiguous int64 [{M}, width, {L}] device tensor (one list per member of idx {(n, L)})")
    width = int(cand.shape[1])
    if width not in BEAM_WIDTHS:
        raise _lib.LcrecError(f"width={width!r} (supported: 1, 2, 4, 8)")
    if tuple(err_held.shape) != (M,) or tuple(cand_err.shape) != (M, width):
        raise _lib.LcrecError(f"err_held {tuple(err_held.shape)} and cand_err {tuple(cand_err.shape)} do not go with cand "
                              f"{tuple(cand.shape)}: one error per member and per candidate")
    if len(ks) != L:
        raise _lib.LcrecError(f"ks {list(ks)} does not go with idx [*, {L}]")
    counters = _counters_out(counters_out, dev, 4)
    if choice_out is None:
        choice_out = torch.full((M,), -1, dtype=torch.int32, device=dev)   # (no group: the library does not touch it)
    elif not (isinstance(choice_out, torch.Tensor) and choice_out.device == dev and choice_out.dtype == torch.int32
              and choice_out.dim() == 1 and choice_out.is_contiguous() and choice_out.numel() >= M):
        raise _lib.LcrecError(f"choice_out must be a contiguous int32 tensor on idx's device with at least {M} elements")
    need = getattr(lib, entry + "_workspace")(n, M, L, width)
    if workspace is not None:
        workspace = _own_workspace(workspace, dev, need, entry + "_workspace")
    with _on(dev):
        ws = workspace if workspace is not None else _workspace(need, dev)
        head = (_ptr(idx), n) + (() if n_frozen is None else (n_frozen,))
        rc = getattr(lib, entry)(*head, L, _ints(ks), _ptr(members), _ptr(offsets), max(offsets.numel() - 1, 0), M, _ptr(err_held),
                                 _ptr(cand), _ptr(cand_err), width, _ptr(choice_out), _ptr(counters), _ptr(ws), ws.numel(),
                                 _stream_ptr())
    _lib.check(rc, entry)
    if counters_out is not None:
        return choice_out[:M], None
    movers, moved, unresolved, rounds = counters.tolist()
    return choice_out[:M], {"movers": movers, "moved": moved, "unresolved": unresolved, "rounds": rounds}


def rq_audit(z, codebooks_flat, ks, idx, want_best=False, want_resid=False):
    """The index audit (lcrec_rq_audit of include/lcrec.h, which states the rule): the GIVEN tuples `idx` walked through the
    residual quantiser from the latents z.  Per item and level: the distance of the held code, the best distance and the held
    code's rank in the level's distance order (0 = the code rq_assign picks on that residual); the residual follows the held code.

    z float32 [n, e]; codebooks_flat / ks as rq_assign; idx int64 [n, L], contiguous or a column block of a wider contiguous
    matrix (matrix[:, c:c + L]); it is only read.  Returns a dict of device tensors: "d_held", "d_best" float32 [n, L], "rank"
    int32 [n, L], "err" float32 [n] (the squared norm of the residual left after the last level), "flags" int32 [n] (bit l: the
    code of level l was outside [0, ks[l]) and was clamped), and on request "best" int64 [n, L] and "resid" float32 [n, e]."""
    z = _dev(z, "z")
    if z.dim() != 2:
        raise _lib.LcrecError(f"z must be [n, e], got {tuple(z.shape)}")
    n, e = z.shape
    L = len(ks)
    dev = z.device
    out = {"d_held": torch.empty((n, L), dtype=torch.float32, device=dev), "d_best": torch.empty((n, L), dtype=torch.float32, device=dev),
           "rank": torch.empty((n, L), dtype=torch.int32, device=dev), "err": torch.empty(n, dtype=torch.float32, device=dev),
           "flags": torch.empty(n, dtype=torch.int32, device=dev)}
    if want_best:
        out["best"] = torch.empty((n, L), dtype=torch.int64, device=dev)
    if want_resid:
        out["resid"] = torch.empty((n, e), dtype=torch.float32, device=dev)
    rq_audit_into(z, codebooks_flat, ks, idx, out)
    return out


def rq_audit_into(z, codebooks_flat, ks, idx, out, workspace=None):
    """lcrec_rq_audit into buffers the caller owns, as rq_assign_into does for lcrec_rq_assign: `out` holds "d_held", "d_best"
    float32, "rank" int32, "err" float32, "flags" int32 and may hold "best" int64 and "resid" float32 (one that is missing is passed
    as NULL), each contiguous on z's device with at least the elements the call writes -- it may be LARGER, so that a test can look
    at what lies past the end.  workspace: a uint8 device tensor of at least lcrec_rq_audit_workspace's bytes, passed as the
    workspace as it is, its size included; None: the binding's own grow-only buffer of the stream, which a captured graph must not
    point into.  Nothing is returned."""
    lib = _lib.load()
    z = _dev(z, "z")
    cb = _dev(codebooks_flat, "codebooks")
    if z.dim() != 2:
        raise _lib.LcrecError(f"z must be [n, e], got {tuple(z.shape)}")
    n, e = z.shape
    L = len(ks)
    dev = z.device
    if cb.numel() != sum(int(k) for k in ks) * e:
        raise _lib.LcrecError(f"codebooks hold {cb.numel()} floats, {list(ks)} x {e} need {sum(int(k) for k in ks) * e}")
    if not (isinstance(idx, torch.Tensor) and idx.is_cuda and idx.device == dev and idx.dtype == torch.int64 and idx.dim() == 2
            and tuple(idx.shape) == (n, L) and (n <= 1 or idx.stride(0) >= L) and (L == 1 or idx.stride(1) == 1)):
        raise _lib.LcrecError(f"idx must be an int64 [{n}, {L}] tensor on z's device, contiguous or a column block of a wider "
                              "contiguous matrix")
    idx_stride = int(idx.stride(0)) if n > 1 else L
    sizes = {"d_held": (torch.float32, n * L), "d_best": (torch.float32, n * L), "rank": (torch.int32, n * L),
             "err": (torch.float32, n), "flags": (torch.int32, n), "best": (torch.int64, n * L), "resid": (torch.float32, n * e)}
    if set(sizes) - {"best", "resid"} - set(out) or set(out) - set(sizes):
        raise _lib.LcrecError(f"out must hold d_held, d_best, rank, err, flags and may hold best, resid; got {sorted(out)}")
    for name, t in out.items():
        dtype, need = sizes[name]
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev and t.dtype == dtype and t.is_contiguous()
                and t.numel() >= need):
            raise _lib.LcrecError(f"out[{name!r}] must be a contiguous {dtype} tensor on z's device with at least {need} elements")
    karr = _ints(ks)
    need = lib.lcrec_rq_audit_workspace(n, e, karr, L)
    if workspace is not None:
        workspace = _own_workspace(workspace, dev, need, "lcrec_rq_audit_workspace")
    if n == 0:                                             # (an empty tensor has no address to pass)
        return
    with _on(dev):
        ws = workspace if workspace is not None else _workspace(need, dev)
        rc = lib.lcrec_rq_audit(_ptr(z), n, e, _ptr(cb), karr, L, _ptr(idx), idx_stride, _ptr(out["d_held"]), _ptr(out["d_best"]),
                                _ptr(out["rank"]), _ptr(out.get("best")), _ptr(out["err"]), _ptr(out.get("resid")),
                                _ptr(out["flags"]), _ptr(ws), ws.numel(), _stream_ptr())
    _lib.check(rc, "lcrec_rq_audit")


BEAM_WIDTHS = (1, 2, 4, 8)
BEAM_WORKSPACE_BOUND = 256 << 20   # bytes of lcrec_rq_beam workspace that rq_beam's chunk walk stays within


def rq_beam(z, codebooks_flat, ks, width, want_resid=False):
    """The beam-search quantiser (lcrec_rq_beam of include/lcrec.h, which states the rule): the `width` best whole tuples of every
    item, best first, each with the score of its last candidate and the squared norm of the residual it leaves.

    z float32 [n, e]; codebooks_flat / ks as rq_assign; width in BEAM_WIDTHS.  Returns a dict of device tensors: "tuples" int64
    [n, width, L], "score", "err" float32 [n, width] and on request "resid" float32 [n, width, e].  Rows past the live count (which
    depends on width and ks alone) hold -1 / +inf.  n is walked in chunks of whole items sized so that the library's workspace (the
    residuals of all beams between the levels and their links) stays within BEAM_WORKSPACE_BOUND = 256 MiB -- 125 202 items per
    chunk at width 8, e = 32, four levels; a single item always goes, whatever it needs."""
    z = _dev(z, "z")
    if z.dim() != 2:
        raise _lib.LcrecError(f"z must be [n, e], got {tuple(z.shape)}")
    if width not in BEAM_WIDTHS:
        raise _lib.LcrecError(f"width={width!r} (supported: 1, 2, 4, 8)")
    n, e = z.shape
    L = len(ks)
    dev = z.device
    out = {"tuples": torch.empty((n, width, L), dtype=torch.int64, device=dev),
           "score": torch.empty((n, width), dtype=torch.float32, device=dev),
           "err": torch.empty((n, width), dtype=torch.float32, device=dev)}
    if want_resid:
        out["resid"] = torch.empty((n, width, e), dtype=torch.float32, device=dev)
    rq_beam_into(z, codebooks_flat, ks, width, out)
    return out


def beam_chunk_rows(e, L, width, bound=None):
    """Items per lcrec_rq_beam call such that its workspace stays within `bound` bytes (None: BEAM_WORKSPACE_BOUND; at least one
    item).  Host only."""
    bound = BEAM_WORKSPACE_BOUND if bound is None else bound
    halves = 0 if L < 2 else (1 if L == 2 else 2)
    per_item = halves * width * e * 4 + max(L - 1, 0) * width * 4
    slack = 256 * (halves + 1)                              # each part is rounded up to 256 bytes
    return max((bound - slack) // per_item, 1) if per_item else 1 << 62


def rq_beam_into(z, codebooks_flat, ks, width, out, workspace=None):
    """lcrec_rq_beam into buffers the caller owns: `out` holds "tuples" int64, "score", "err" float32 and may hold "resid" float32
    (missing: passed as NULL), each contiguous on z's device with at least the elements the call writes -- it may be LARGER, so
    that a test can look at what lies past the end.  workspace: a uint8 device tensor passed as the workspace as it is, its size
    included, for ONE call over all rows; None: the binding's own, and the chunk walk of rq_beam.  Nothing is returned."""
    lib = _lib.load()
    z = _dev(z, "z")
    cb = _dev(codebooks_flat, "codebooks")
    if z.dim() != 2:
        raise _lib.LcrecError(f"z must be [n, e], got {tuple(z.shape)}")
    n, e = z.shape
    L = len(ks)
    dev = z.device
    width = int(width)
    if cb.numel() != sum(int(k) for k in ks) * e:
        raise _lib.LcrecError(f"codebooks hold {cb.numel()} floats, {list(ks)} x {e} need {sum(int(k) for k in ks) * e}")
    sizes = {"tuples": (torch.int64, width * L), "score": (torch.float32, width), "err": (torch.float32, width),
             "resid": (torch.float32, width * e)}
    if set(sizes) - {"resid"} - set(out) or set(out) - set(sizes):
        raise _lib.LcrecError(f"out must hold tuples, score, err and may hold resid; got {sorted(out)}")
    for name, t in out.items():
        dtype, per = sizes[name]
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev and t.dtype == dtype and t.is_contiguous()
                and t.numel() >= n * per):
            raise _lib.LcrecError(f"out[{name!r}] must be a contiguous {dtype} tensor on z's device with at least {n * per} elements")
    if workspace is not None and not _is_workspace(workspace, dev):                    # (one call over all rows: no size to ask for)
        raise _lib.LcrecError("workspace must be a contiguous uint8 tensor on z's device")
    if n == 0:                                             # (an empty tensor has no address to pass)
        return
    karr = _ints(ks)
    step = n if workspace is not None else min(n, beam_chunk_rows(e, L, width))
    flat = {name: t.view(-1) for name, t in out.items()}
    with _on(dev):
        for a in range(0, n, step):
            rows = min(step, n - a)
            ws = workspace if workspace is not None else _workspace(lib.lcrec_rq_beam_workspace(rows, e, karr, L, width), dev)
            part = {name: flat[name][a * sizes[name][1]:] for name in flat}
            rc = lib.lcrec_rq_beam(_ptr(z[a:a + rows]), rows, e, _ptr(cb), karr, L, width, _ptr(part["tuples"]), _ptr(part["score"]),
                                   _ptr(part["err"]), _ptr(part.get("resid")), _ptr(ws) if ws.numel() else _ptr(None), ws.numel(),
                                   _stream_ptr())
            _lib.check(rc, "lcrec_rq_beam")


def beam_choose(z, codebooks_flat, ks, greedy, width):
    """The chosen tuples of a beam of `width` over the latents z, given their greedy tuples `greedy` int64 [n, L] (rq_assign's /
    encode_assign's): item i gets beam 0's tuple unless err_greedy[i] < err_beam0[i] (strict; a NaN counts as +inf), in which case it
    keeps the greedy one -- a beam is not monotone, and this way no item's final error exceeds its greedy error.  err_greedy is
    rq_audit's err of the greedy tuples: the same fma chain as the beam's, so at width 1 nothing is ever replaced.
    Returns (chosen int64 [n, L], dict of "err_greedy", "err_chosen" float32 [n], "kept_greedy" bool [n], "beams": rq_beam's dict)."""
    beams = rq_beam(z, codebooks_flat, ks, width)
    err_g = rq_audit(z, codebooks_flat, ks, greedy)["err"]
    err_b = beams["err"][:, 0]
    inf = torch.full_like(err_g, float("inf"))
    eg, eb = torch.where(torch.isnan(err_g), inf, err_g), torch.where(torch.isnan(err_b), inf, err_b)
    keep = eg < eb
    chosen = torch.where(keep[:, None], greedy, beams["tuples"][:, 0, :])
    return chosen, {"err_greedy": err_g, "err_chosen": torch.where(keep, err_g, err_b), "kept_greedy": keep, "beams": beams}


def decode_plan(n, dims, ks, want_out=True, chunk_rows=0):
    """How decode_tuples walks n rows through a decoder of widths `dims` (e_dim, hidden sizes ..., the embedding width) and where
    everything lies in its workspace (include/lcrec.h, lcrec_debug_decode_tuples_plan): dict of the fields of lcrec_decode_plan.
    chunk_rows: 0 = the built-in chunk.  Host only: no GPU is needed.  LcrecError for shapes lcrec_decode_tuples refuses."""
    lib = _lib.load()
    plan = _lib.DecodePlan()
    rc = lib.lcrec_debug_decode_tuples_plan(int(n), _ints(dims), len(dims) - 1, _ints(ks), len(ks), int(bool(want_out)),
                                            int(chunk_rows), ctypes.addressof(plan))
    _lib.check(rc, "lcrec_debug_decode_tuples_plan")
    out = {}
    for name, _ in _lib.DecodePlan._fields_:
        value = getattr(plan, name)
        out[name] = [int(v) for v in value] if name == "act_offset" else int(value)
    return out


def decode_tuples(idx, codebooks_flat, ks, weights, biases, bn_scales=None, bn_shifts=None, x=None, l1=False, want_out=True,
                  want_xq=False, chunk_rows=0, into=None, workspace=None):
    """The decode pass (lcrec_decode_tuples of include/lcrec.h, which states the rule): the GIVEN tuples `idx` back to embeddings --
    the sum of their code rows, then the decoder MLP -- and, with x, every item's reconstruction error against its row of x.

    idx int64 [n, L], contiguous or a column block of a wider contiguous matrix (matrix[:, c:c + L]); it is only read.
    codebooks_flat / ks as rq_assign.  weights[l] is nn.Linear.weight of DECODER layer l ([out_l, in_l]), biases[l] its bias or
    None; bn_scales / bn_shifts per-layer folded eval-mode BatchNorm affines or None (the whole list, or single entries) -- what
    MLPLayers.folded() returns.  x float32 [n, w] or None; l1: the L1 loss's error (sum |d|) instead of the squared one.
    chunk_rows: 0 = the built-in chunk, any other size gives the same bits (lcrec_debug_decode_tuples).
    into: a dict of buffers the caller owns, written instead of fresh ones -- "xq", "out", "err" float32, "flags" int32, each
    contiguous on idx's device with at least the elements the call writes (it may be LARGER, so that a test can look at what lies
    past the end); an output that is not in the dict is passed as NULL, and want_out / want_xq are not read.  workspace: a uint8
    device tensor passed as the workspace as it is, its size included.
    Returns a dict of device tensors "out" float32 [n, w], "xq" float32 [n, e], "err" float32 [n], "flags" int32 [n] (bit l: the
    code of level l was outside [0, ks[l]) and was clamped); what was not asked for is None."""
    lib = _lib.load()
    cb = _dev(codebooks_flat, "codebooks")
    nl, L, dev = len(weights), len(ks), cb.device
    if nl < 1 or len(biases) != nl:
        raise _lib.LcrecError(f"decoder: {nl} weights and {len(biases)} biases")
    ws_ = [_dev(w, "weight") for w in weights]
    bs_ = [None if b is None else _dev(b, "bias") for b in biases]
    scs = [None] * nl if bn_scales is None else [None if s is None else _dev(s, "bn_scale") for s in bn_scales]
    shs = [None] * nl if bn_shifts is None else [None if s is None else _dev(s, "bn_shift") for s in bn_shifts]
    dims = [int(ws_[0].shape[1])] + [int(w.shape[0]) for w in ws_]
    for l in range(nl):
        if ws_[l].dim() != 2 or ws_[l].shape[1] != dims[l]:
            raise _lib.LcrecError(f"decoder layer {l}: weight {tuple(ws_[l].shape)} does not chain")
    e, w = dims[0], dims[-1]
    if cb.numel() != sum(int(k) for k in ks) * e:
        raise _lib.LcrecError(f"codebooks hold {cb.numel()} floats, {list(ks)} x {e} need {sum(int(k) for k in ks) * e}")
    if not (isinstance(idx, torch.Tensor) and idx.is_cuda and idx.device == dev and idx.dtype == torch.int64 and idx.dim() == 2
            and idx.shape[1] == L and (idx.shape[0] <= 1 or idx.stride(0) >= L) and (L == 1 or idx.stride(1) == 1)):
        raise _lib.LcrecError(f"idx must be an int64 [n, {L}] tensor on the codebooks' device, contiguous or a column block of a "
                              "wider contiguous matrix")
    n = int(idx.shape[0])
    idx_stride = int(idx.stride(0)) if n > 1 else L
    if x is not None:
        x = _dev(x, "x")
        if tuple(x.shape) != (n, w):
            raise _lib.LcrecError(f"x is {tuple(x.shape)}, the decoder writes [{n}, {w}]")
    sizes = {"xq": (torch.float32, n * e), "out": (torch.float32, n * w), "err": (torch.float32, n), "flags": (torch.int32, n)}
    if into is None:
        res = {"out": torch.empty((n, w), dtype=torch.float32, device=dev) if want_out else None,
               "xq": torch.empty((n, e), dtype=torch.float32, device=dev) if want_xq else None,
               "err": torch.empty(n, dtype=torch.float32, device=dev) if x is not None else None,
               "flags": torch.empty(n, dtype=torch.int32, device=dev)}
    else:
        if set(into) - set(sizes):
            raise _lib.LcrecError(f"into may hold {sorted(sizes)}, got {sorted(into)}")
        for name, t in into.items():
            dtype, need = sizes[name]
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev and t.dtype == dtype and t.is_contiguous()
                    and t.numel() >= need):
                raise _lib.LcrecError(f"into[{name!r}] must be a contiguous {dtype} tensor on idx's device with at least {need} elements")
        res = {name: into.get(name) for name in sizes}
    if workspace is not None and not (isinstance(workspace, torch.Tensor) and workspace.is_cuda and workspace.device == dev
                                      and workspace.dtype == torch.uint8 and workspace.is_contiguous()):
        raise _lib.LcrecError("workspace must be a contiguous uint8 tensor on idx's device")
    if n == 0 and workspace is None:                       # (an empty tensor has no address to pass)
        return res
    PA = ctypes.c_void_p * nl
    wp = PA(*[t.data_ptr() for t in ws_])
    bp = PA(*[0 if t is None else t.data_ptr() for t in bs_])
    scp = None if bn_scales is None else PA(*[0 if t is None else t.data_ptr() for t in scs])    # (no list: the NULL array)
    shp = None if bn_shifts is None else PA(*[0 if t is None else t.data_ptr() for t in shs])
    darr, karr = _ints(dims), _ints(ks)
    with _on(dev):
        if workspace is not None:
            ws = workspace
        else:
            ws = _workspace(lib.lcrec_debug_decode_tuples_workspace(n, darr, nl, karr, L, int(res["out"] is not None), int(chunk_rows)),
                            dev)
        args = (_ptr(idx), idx_stride, n, _ptr(cb), karr, L, darr, nl, wp, bp, scp, shp, _ptr(res["xq"]), _ptr(res["out"]), _ptr(x),
                int(bool(l1)), _ptr(res["err"]), _ptr(res["flags"]), _ptr(ws), ws.numel(), _stream_ptr())
        if chunk_rows:
            rc, what = lib.lcrec_debug_decode_tuples(*args, int(chunk_rows)), "lcrec_debug_decode_tuples"
        else:
            rc, what = lib.lcrec_decode_tuples(*args), "lcrec_decode_tuples"
    _lib.check(rc, what)
    return res


TRIE_ARRAYS = (("order", torch.int64), ("counts", torch.int64), ("child", torch.int64), ("code", torch.int32), ("first", torch.int64))


def trie_array_sizes(n, L):
    """Elements of the five arrays of lcrec_index_trie for n items of L levels (an array is never empty: it has an address)."""
    n, L = int(n), int(L)
    return {"order": max(n, 1), "counts": L + 1, "child": L * (n + 1), "code": max(L * n, 1), "first": n + 1}


class Trie:
    """lcrec_index_trie of include/lcrec.h with the device tensors its pointers name: `record` (the ctypes record the library
    reads), `arrays` (name -> tensor), n, L, ks, device."""
    __slots__ = ("record", "arrays", "n", "L", "ks", "device")


def trie_build(idx, ks, arrays=None, workspace=None):
    """lcrec_index_trie_build: the prefix trie of an int64 [n, L] device matrix (include/lcrec.h states the layout).

    idx may be a view of a wider matrix -- rows idx.stride(0) apart, columns adjacent; it is never written.  arrays: the five
    tensors to fill (trie_array_sizes; each contiguous on idx's device, of its dtype, at least that large), None: fresh ones.
    workspace: a uint8 device tensor passed as it is, None: the binding's own.  Returns a Trie; nothing is read back."""
    lib = _lib.load()
    if not (isinstance(idx, torch.Tensor) and idx.is_cuda and idx.dtype == torch.int64 and idx.dim() == 2):
        raise _lib.LcrecError("idx must be an int64 [n, L] tensor on a HIP device (lcrec_amd has no CPU path)")
    n, L = idx.shape
    if L != len(ks):
        raise _lib.LcrecError(f"idx has {L} columns but ks {len(ks)} levels")
    if n > 1 and idx.stride(1) != 1 or (n > 1 and idx.stride(0) < L):
        idx = idx.contiguous()
    stride = idx.stride(0) if n > 1 else L
    dev = idx.device
    sizes = trie_array_sizes(n, L)
    if arrays is None:
        arrays = {name: torch.empty(sizes[name], dtype=dtype, device=dev) for name, dtype in TRIE_ARRAYS}
    for name, dtype in TRIE_ARRAYS:
        t = arrays.get(name)
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dtype and t.is_contiguous() and t.numel() >= sizes[name]):
            raise _lib.LcrecError(f"arrays[{name!r}] must be a contiguous {dtype} tensor on idx's device with at least {sizes[name]} elements")
    trie = Trie()
    trie.record = _lib.IndexTrie()
    for name, _ in TRIE_ARRAYS:
        setattr(trie.record, name, arrays[name].data_ptr())
    trie.arrays, trie.n, trie.L, trie.ks, trie.device = arrays, n, L, [int(k) for k in ks], dev
    karr = _ints(ks)
    with _on(dev):
        need = lib.lcrec_index_trie_build_workspace(n, L)
        ws = _workspace(need, dev) if workspace is None else _own_workspace(workspace, dev, need, "lcrec_index_trie_build_workspace")
        rc = lib.lcrec_index_trie_build(_ptr(idx) if n else _ptr(None), stride, n, L, karr, ctypes.addressof(trie.record),
                                        _ptr(ws) if ws.numel() else _ptr(None), ws.numel(), _stream_ptr())
    _lib.check(rc, "lcrec_index_trie_build")
    return trie


def _trie_rows(t, name, trie):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == trie.device and t.dtype == torch.int64):
        raise _lib.LcrecError(f"{name} must be an int64 tensor on the trie's device ({trie.device})")
    return t


def trie_find(trie, prefix, depth, longest=False, node_out=None, depth_out=None, rows=None):
    """lcrec_index_trie_find: longest-prefix descent of every row of `prefix` (int64 [B, >= depth] on the trie's device, rows
    prefix.stride(0) apart; None with rows=B when depth == 0).  Returns node int64 [B] -- -1 where the full depth was not
    reached -- or, with longest, (node, depth reached int32 [B]).  node_out / depth_out: contiguous buffers of at least B
    elements to write into (they may be larger); they are returned as given."""
    lib = _lib.load()
    depth = int(depth)
    if prefix is None:
        B, stride = int(rows or 0), 0
    else:
        _trie_rows(prefix, "prefix", trie)
        if prefix.dim() != 2 or prefix.shape[1] < depth:
            raise _lib.LcrecError(f"prefix must be [B, >= {depth}], got {tuple(prefix.shape)}")
        if prefix.shape[0] > 1 and prefix.shape[1] > 0 and (prefix.stride(1) != 1 or prefix.stride(0) < depth):
            prefix = prefix.contiguous()
        B = prefix.shape[0]
        stride = prefix.stride(0) if B > 1 and prefix.shape[1] > 0 else max(depth, 0)
    dev = trie.device
    if node_out is None:
        node_out = torch.empty(max(B, 1), dtype=torch.int64, device=dev)[:B]
    if longest and depth_out is None:
        depth_out = torch.empty(max(B, 1), dtype=torch.int32, device=dev)[:B]
    for name, t, dtype in (("node_out", node_out, torch.int64), ("depth_out", depth_out, torch.int32)):
        if t is not None and not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dtype and t.is_contiguous()
                                  and t.numel() >= B):
            raise _lib.LcrecError(f"{name} must be a contiguous {dtype} tensor on the trie's device with at least {B} elements")
    with _on(dev):
        rc = lib.lcrec_index_trie_find(ctypes.addressof(trie.record), _ptr(prefix) if prefix is not None and B and depth else _ptr(None),
                                       stride, B, depth, _ptr(node_out) if B else _ptr(None),
                                       _ptr(depth_out) if longest and B else _ptr(None), _stream_ptr())
    _lib.check(rc, "lcrec_index_trie_find")
    return (node_out, depth_out) if longest else node_out


def trie_mask_logits_(trie, logits, node, depth, token_ids=None, eos=-1):
    """lcrec_index_trie_mask_logits, in place: logits float32 [B, V] on the trie's device, columns adjacent and rows
    logits.stride(0) >= V apart (a view of a wider or offset buffer goes as it is); node int64 [B]; token_ids int32 [ks[depth]] or
    None for the identity map.  Everything outside the allowed set of a row becomes -inf; nothing is returned."""
    lib = _lib.load()
    dev = trie.device
    if not (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.device == dev and logits.dtype == torch.float32
            and logits.dim() == 2):
        raise _lib.LcrecError(f"logits must be a float32 [B, V] tensor on the trie's device ({dev})")
    B, V = logits.shape
    if V > 1 and logits.stride(1) != 1 or (B > 1 and logits.stride(0) < V):
        raise _lib.LcrecError("logits is masked in place: its columns must be adjacent and its rows must not overlap")
    ld = logits.stride(0) if B > 1 else V
    _trie_rows(node, "node", trie)
    if node.dim() != 1 or node.shape[0] != B or not node.is_contiguous():
        raise _lib.LcrecError(f"node must be a contiguous int64 [{B}] tensor")
    depth = int(depth)
    if token_ids is not None:
        need = trie.ks[depth] if 0 <= depth < trie.L else 0
        if not (isinstance(token_ids, torch.Tensor) and token_ids.device == dev and token_ids.dtype == torch.int32
                and token_ids.is_contiguous() and token_ids.numel() >= need):
            raise _lib.LcrecError(f"token_ids must be a contiguous int32 tensor on the trie's device with at least {need} elements")
    with _on(dev):
        rc = lib.lcrec_index_trie_mask_logits(ctypes.addressof(trie.record), _ptr(node) if B else _ptr(None), B, depth, _ptr(token_ids),
                                              int(eos), _ptr(logits) if B else _ptr(None), ld, V, _stream_ptr())
    _lib.check(rc, "lcrec_index_trie_mask_logits")


def index_json_text(idx_rows, first_item=0):
    """bytes of the `.index.json` entries of items first_item.. for a HOST int64 [n, L] array
    (generate_indices.py:83-92,138-145; see lcrec_index_json_format in include/lcrec.h)."""
    import numpy as np
    lib = _lib.load()
    a = np.ascontiguousarray(idx_rows, dtype=np.int64)
    if a.ndim != 2:
        raise _lib.LcrecError("idx_rows must be [n, L]")
    n, L = a.shape
    if n == 0:
        return b""
    cap = lib.lcrec_index_json_bound(n, L)
    buf = np.empty(cap, dtype=np.uint8)
    got = lib.lcrec_index_json_format(a.ctypes.data, n, L, int(first_item), buf.ctypes.data, cap)
    if got < 0:
        _lib.check(int(got), "lcrec_index_json_format")
    return buf[:got].tobytes()


def index_json_parse(text, L):
    """int64 [n, L] numpy array of the codes in an `.index.json` text (bytes), by the library's strict reader
    (lcrec_index_json_parse of include/lcrec.h): exactly the texts index_json_text / json.dump with default separators write for
    keys "0", "1", ... in order.  Anything else raises LcrecError, whose text names the byte offset."""
    import numpy as np
    lib = _lib.load()
    if not isinstance(text, (bytes, bytearray, memoryview)):
        raise _lib.LcrecError("text must be bytes")
    L = int(L)
    if not 1 <= L <= 26:
        raise _lib.LcrecError(f"L={L}: 1 .. 26 levels (prefix letters a .. z)")
    raw = np.frombuffer(text, dtype=np.uint8)
    cap = raw.size // (9 * L + 7) + 1                      # the shortest item, `"0": ["<a_0>", ...], `, takes 9 L + 7 bytes
    out = np.empty((cap, L), dtype=np.int64)
    got = lib.lcrec_index_json_parse(raw.ctypes.data, raw.size, L, out.ctypes.data, cap)
    if got < 0:
        _lib.check(int(got), "lcrec_index_json_parse")
    return out[:got].copy()


# ---- training-step kernels (csrc/train_ops.hip)
def _vec(t, name, F):
    if t is None:
        return None
    t = _dev(t, name)
    if t.numel() != F:
        raise _lib.LcrecError(f"{name} must have {F} elements")
    return t


def bn_relu_forward(t, gamma, beta, eps=1e-5, momentum=0.1, running_mean=None, running_var=None, relu=True):
    """Training-mode BatchNorm1d (+ReLU) of a Linear's output (layers.py:25-30): returns (y, mean, rstd); the running
    statistics (contiguous fp32 buffers of the module) are updated in place."""
    lib = _lib.load()
    t = _dev(t, "t")
    n, F = t.shape
    gamma, beta = _vec(gamma, "gamma", F), _vec(beta, "beta", F)
    for name, buf in (("running_mean", running_mean), ("running_var", running_var)):
        if buf is not None and not (buf.is_cuda and buf.is_contiguous() and buf.dtype == torch.float32 and buf.numel() == F):
            raise _lib.LcrecError(f"{name} must be a contiguous float32 device buffer of {F} elements")
    y = torch.empty_like(t)
    mean = torch.empty(F, dtype=torch.float32, device=t.device)
    rstd = torch.empty(F, dtype=torch.float32, device=t.device)
    with _on(t.device):
        rc = lib.lcrec_bn_relu_forward(_ptr(t), n, F, _ptr(gamma), _ptr(beta), float(eps), float(momentum), _ptr(running_mean),
                                       _ptr(running_var), _ptr(y), _ptr(mean), _ptr(rstd), int(bool(relu)), _stream_ptr())
    _lib.check(rc, "lcrec_bn_relu_forward")
    return y, mean, rstd


def bn_relu_backward(gy, t, y, gamma, mean, rstd, relu=True, dgamma_out=None, dbeta_out=None, dbias_out=None, fold=None, beta=None):
    """(dt, dgamma, dbeta, dbias) of y = [relu](bn(t)) for gy = dL/dy (see lcrec_bn_relu_backward); the three vector
    outputs may be given (views of a flat gradient buffer).  y None + fold = (scale, shift): the ReLU mask is recomputed as
    [t * scale + shift > 0].  y None + beta: the mask is recomputed with bn_relu_forward's own expression -- the bits of
    the y it wrote, without reading it."""
    lib = _lib.load()
    gy, t = _dev(gy, "gy"), _dev(t, "t")
    y = None if y is None else _dev(y, "y")
    n, F = t.shape
    gamma = _vec(gamma, "gamma", F)
    mk = lambda o: o if o is not None else torch.empty(F, dtype=torch.float32, device=t.device)
    dgamma, dbeta, dbias = mk(dgamma_out), mk(dbeta_out), mk(dbias_out)
    dt = torch.empty_like(t)
    with _on(t.device):
        rc = lib.lcrec_bn_relu_backward(_ptr(gy), _ptr(t), _ptr(y), n, F, _ptr(gamma), _ptr(_vec(mean, "mean", F)),
                                        _ptr(_vec(rstd, "rstd", F)), int(bool(relu)), _ptr(dt), _ptr(dgamma), _ptr(dbeta),
                                        _ptr(dbias), _ptr(None if fold is None else _vec(fold[0], "fold_scale", F)),
                                        _ptr(_vec(fold[1], "fold_shift", F) if fold is not None else
                                             (_vec(beta, "beta", F) if (y is None and beta is not None) else None)), _stream_ptr())
    _lib.check(rc, "lcrec_bn_relu_backward")
    return dt, dgamma, dbeta, dbias


def bn_stats(t, row_out=None):
    """(mean, m2) of this rank's rows: m2 = sum (t - mean)^2 (lcrec_bn_stats).
    row_out: a float32 [2F+1] exchange row (n_r, mean[F], m2[F]) to write them into (slot 0 is the caller's)."""
    lib = _lib.load()
    t = _dev(t, "t")
    n, F = t.shape
    if row_out is not None:
        if not (row_out.is_cuda and row_out.dtype == torch.float32 and row_out.is_contiguous() and row_out.numel() == 2 * F + 1):
            raise _lib.LcrecError("row_out must be a contiguous float32 [2F+1] device tensor")
        mean, m2 = row_out[1:F + 1], row_out[F + 1:]
    else:
        mean = torch.empty(F, dtype=torch.float32, device=t.device)
        m2 = torch.empty(F, dtype=torch.float32, device=t.device)
    with _on(t.device):
        rc = lib.lcrec_bn_stats(_ptr(t), n, F, _ptr(mean), _ptr(m2), _stream_ptr())
    _lib.check(rc, "lcrec_bn_stats")
    return mean, m2


BN_CALLS = ("forward", "backward", "stats", "reduce", "apply")      # LCREC_BN_* of include/lcrec.h, in order


def bn_plan(call, n, F, aligned=True):
    """The kernel form the BatchNorm strip call `call` (one of BN_CALLS) takes for [n, F] rows, `aligned` saying whether every
    pointer of the call sits on 16 bytes (include/lcrec.h, lcrec_debug_bn_plan), as a dict of the fields of lcrec_bn_plan.
    Host only: no GPU is needed."""
    plan = _lib.BnPlan()
    rc = _lib.load().lcrec_debug_bn_plan(BN_CALLS.index(call), int(n), int(F), int(bool(aligned)), ctypes.addressof(plan))
    _lib.check(rc, "lcrec_debug_bn_plan")
    return {name: int(getattr(plan, name)) for name, _ in _lib.BnPlan._fields_}


TAIL_CALLS = ("relu_bias_backward", "recon_loss_grad", "grad_norm_clip", "quantizer_input_grad_bias", "rq_apply_level", "code_stats",
              "code_stats_levels")                                   # LCREC_TAIL_* of include/lcrec.h, in order
TAIL_FAMILIES = ("strip", "reduce", "qgb_one", "qg_two", "apply_level", "cs_sorted", "cs_streaming", "cs_levels", "cs_per_level")   # LCREC_TAILK_*


def step_tail_plan(call, n_or_count, width=0, aligned=True, K=0):
    """The launch the step-tail call `call` (one of TAIL_CALLS) picks for its size (include/lcrec.h, lcrec_debug_step_tail_plan),
    as a dict of the fields of lcrec_step_tail_plan with `family` as its name in TAIL_FAMILIES.  K: the codebook size, for the two
    code_stats calls.  Host only: no GPU is needed."""
    plan = _lib.StepTailPlan()
    plan.K = int(K)
    rc = _lib.load().lcrec_debug_step_tail_plan(TAIL_CALLS.index(call), int(n_or_count), int(width), int(bool(aligned)), ctypes.addressof(plan))
    _lib.check(rc, "lcrec_debug_step_tail_plan")
    out = {name: int(getattr(plan, name)) for name, _ in _lib.StepTailPlan._fields_}
    out["family"] = TAIL_FAMILIES[out["family"]]
    return out


def optim_plan(count, aligned=True, has_ticket=True):
    """The launch of the optimiser step kernel for `count` elements (include/lcrec.h, lcrec_debug_optim_plan), as a dict of the
    fields of lcrec_optim_plan.  Host only: no GPU is needed."""
    plan = _lib.OptimPlan()
    rc = _lib.load().lcrec_debug_optim_plan(int(count), int(bool(aligned)), int(bool(has_ticket)), ctypes.addressof(plan))
    _lib.check(rc, "lcrec_debug_optim_plan")
    return {name: int(getattr(plan, name)) for name, _ in _lib.OptimPlan._fields_}


def bn_merge_stats(rows, eps, momentum=0.0, running_mean=None, running_var=None):
    """(mean, rstd) of the union of the ranks' rows from rows [world, 2F+1] = (n_r, mean_r, m2_r); updates the running
    statistics in place when given (lcrec_bn_merge_stats)."""
    lib = _lib.load()
    rows = _dev(rows, "rows")
    world, width = rows.shape
    F = (width - 1) // 2
    mean = torch.empty(F, dtype=torch.float32, device=rows.device)
    rstd = torch.empty(F, dtype=torch.float32, device=rows.device)
    with _on(rows.device):
        rc = lib.lcrec_bn_merge_stats(_ptr(rows), world, F, float(eps), float(momentum), _ptr(mean), _ptr(rstd),
                                      _ptr(None if running_mean is None else _vec(running_mean, "running_mean", F)),
                                      _ptr(None if running_var is None else _vec(running_var, "running_var", F)), _stream_ptr())
    _lib.check(rc, "lcrec_bn_merge_stats")
    return mean, rstd


def bn_relu_apply(t, gamma, beta, mean, rstd, relu=True):
    lib = _lib.load()
    t = _dev(t, "t")
    n, F = t.shape
    y = torch.empty_like(t)
    with _on(t.device):
        rc = lib.lcrec_bn_relu_apply(_ptr(t), n, F, _ptr(_vec(gamma, "gamma", F)), _ptr(_vec(beta, "beta", F)),
                                     _ptr(_vec(mean, "mean", F)), _ptr(_vec(rstd, "rstd", F)), int(bool(relu)), _ptr(y),
                                     _stream_ptr())
    _lib.check(rc, "lcrec_bn_relu_apply")
    return y


def bn_backward_reduce(gy, t, y, mean, rstd, relu=True, dbeta_out=None, dgamma_out=None):
    """float32 [2, F]: (sum g, sum g * xhat) over this rank's rows (lcrec_bn_backward_reduce); dbeta_out / dgamma_out
    receive a copy of the two rows (this rank's share of the BatchNorm parameter gradients)."""
    lib = _lib.load()
    gy, t = _dev(gy, "gy"), _dev(t, "t")
    n, F = t.shape
    sums = torch.empty((2, F), dtype=torch.float32, device=t.device)
    with _on(t.device):
        rc = lib.lcrec_bn_backward_reduce(_ptr(gy), _ptr(t), _ptr(None if y is None else _dev(y, "y")), n, F,
                                          _ptr(_vec(mean, "mean", F)), _ptr(_vec(rstd, "rstd", F)), int(bool(relu)),
                                          _ptr(sums[0]), _ptr(sums[1]),
                                          _ptr(None if dbeta_out is None else _vec(dbeta_out, "dbeta_out", F)),
                                          _ptr(None if dgamma_out is None else _vec(dgamma_out, "dgamma_out", F)), _stream_ptr())
    _lib.check(rc, "lcrec_bn_backward_reduce")
    return sums


def bn_backward_apply(gy, t, y, gamma, mean, rstd, sums, n_total, relu=True, dbias_out=None):
    """(dt, dbias) from the all-reduced [2, F] sums (lcrec_bn_backward_apply)."""
    lib = _lib.load()
    gy, t = _dev(gy, "gy"), _dev(t, "t")
    n, F = t.shape
    sums = _dev(sums, "sums")
    dt = torch.empty_like(t)
    dbias = _vec(dbias_out, "dbias_out", F) if dbias_out is not None else torch.empty(F, dtype=torch.float32, device=t.device)
    with _on(t.device):
        rc = lib.lcrec_bn_backward_apply(_ptr(gy), _ptr(t), _ptr(None if y is None else _dev(y, "y")), n, F,
                                         _ptr(_vec(gamma, "gamma", F)), _ptr(_vec(mean, "mean", F)), _ptr(_vec(rstd, "rstd", F)),
                                         int(bool(relu)), _ptr(sums[0]), _ptr(sums[1]), float(n_total), _ptr(dt), _ptr(dbias),
                                         _stream_ptr())
    _lib.check(rc, "lcrec_bn_backward_apply")
    return dt, dbias


def relu_bias_backward(gy, y, relu=True, dbias_out=None, inplace=False):
    """(g, dbias): g = gy * [y > 0] (or gy itself when relu is False), dbias = column sums of g."""
    lib = _lib.load()
    gy = _dev(gy, "gy")
    n, F = gy.shape
    y = _dev(y, "y") if relu else None
    g = gy if (inplace or not relu) else torch.empty_like(gy)
    dbias = dbias_out if dbias_out is not None else torch.empty(F, dtype=torch.float32, device=gy.device)
    with _on(gy.device):
        rc = lib.lcrec_relu_bias_backward(_ptr(gy), _ptr(y), n, F, int(bool(relu)), _ptr(g) if relu else None, _ptr(dbias),
                                          _stream_ptr())
    _lib.check(rc, "lcrec_relu_bias_backward")
    return g, dbias


def recon_loss_grad(out, x, loss_type="mse", want_grad=True, global_rows=None):
    """(loss float32 scalar tensor, grad | None) of rqvae.py:74-85's reconstruction term.  global_rows: rows of the global
    batch when `out` is one rank's shard of it -- loss and gradient are then this rank's share of the global mean's."""
    lib = _lib.load()
    out, x = _dev(out, "out"), _dev(x, "x")
    if out.shape != x.shape:
        raise _lib.LcrecError(f"recon_loss_grad: shapes {tuple(out.shape)} vs {tuple(x.shape)}")
    if loss_type not in ("mse", "l1"):
        raise ValueError("incompatible loss type")
    g = torch.empty_like(out) if want_grad else None
    loss = torch.empty((), dtype=torch.float32, device=out.device)
    with _on(out.device):
        ws = _workspace(lib.lcrec_train_reduce_workspace(), out.device)
        total = 0 if global_rows is None else int(global_rows) * (out.numel() // max(1, out.shape[0]))
        rc = lib.lcrec_recon_loss_grad(_ptr(out), _ptr(x), out.numel(), total, int(loss_type == "l1"), _ptr(g), _ptr(loss), _ptr(ws),
                                       ws.numel(), _ptr(_ticket(out.device)), _stream_ptr())
    _lib.check(rc, "lcrec_recon_loss_grad")
    return loss, g


def grad_norm_clip(flat_grads, max_norm=1.0, out=None):
    """float32 [2] device tensor: (global L2 norm, clip coefficient) of a flat gradient buffer (trainer.py:118)."""
    lib = _lib.load()
    g = _dev(flat_grads, "grads")
    res = out if out is not None else torch.empty(2, dtype=torch.float32, device=g.device)
    with _on(g.device):
        ws = _workspace(lib.lcrec_train_reduce_workspace(), g.device)
        rc = lib.lcrec_grad_norm_clip(_ptr(g), g.numel(), float(max_norm), _ptr(res), _ptr(ws), ws.numel(), _ptr(_ticket(g.device)),
                                      _stream_ptr())
    _lib.check(rc, "lcrec_grad_norm_clip")
    return res


def codebook_grad(count, total, codebook, scale, weight, out):
    """out[k] = (scale * (count[k] * C[k] - sum[k])) * weight (see lcrec_codebook_grad); `out` is written in place."""
    lib = _lib.load()
    count, total, codebook = _dev(count, "count"), _dev(total, "sum"), _dev(codebook, "codebook")
    K, e = codebook.shape
    if not (out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (K, e)):
        raise _lib.LcrecError("out must be a contiguous float32 [K, e] device tensor")
    with _on(codebook.device):
        rc = lib.lcrec_codebook_grad(_ptr(count), _ptr(total), _ptr(codebook), K, e, float(scale), float(weight), _ptr(out),
                                     _stream_ptr())
    _lib.check(rc, "lcrec_codebook_grad")
    return out


def step_losses(sse, n, e, beta, quant_loss_weight, recon, losses_out, sums=None, nan_flag=None, poison_probe=None,
                poison_flag=None):
    """losses_out[3] = (loss, recon, rq_loss) from the per-level sse (float64 [L]) and the reconstruction loss; optional
    running sums (float64 [2], +=) and NaN flag (bool/uint8 scalar, set) -- lcrec_step_losses.  poison_probe (int64 [1]
    device view) / poison_flag (bool/uint8 scalar): the flag is set when the probed assignment is negative."""
    lib = _lib.load()
    if not (sse.is_cuda and sse.dtype == torch.float64 and sse.is_contiguous()):
        raise _lib.LcrecError("sse must be a contiguous float64 device tensor")
    with _on(sse.device):
        rc = lib.lcrec_step_losses(_ptr(sse), sse.numel(), int(n), int(e), float(beta), float(quant_loss_weight), _ptr(recon),
                                   _ptr(losses_out), _ptr(sums), _ptr(nan_flag), _ptr(poison_probe),
                                   _ptr(poison_flag) if poison_probe is not None else None, _stream_ptr())
    _lib.check(rc, "lcrec_step_losses")
    return losses_out


def quantizer_input_grad(z, codebook0, idx_col, coef, weight, g_xq, dbias_out=None):
    """(coef * (z - C0[idx0])) * weight + g_xq (lcrec_quantizer_input_grad); with dbias_out [e] also its column sums, the bias
    gradient of the encoder's last Linear, in the same launch (lcrec_quantizer_input_grad_bias)."""
    lib = _lib.load()
    z, codebook0, g_xq = _dev(z, "z"), _dev(codebook0, "codebook"), _dev(g_xq, "g_xq")
    n, e = z.shape
    idx_col, stride = _idx_col(idx_col, n)
    out = torch.empty_like(z)
    with _on(z.device):
        if dbias_out is None:
            rc = lib.lcrec_quantizer_input_grad(_ptr(z), _ptr(codebook0), _ptr(idx_col), stride, n, e, float(coef), float(weight),
                                                _ptr(g_xq), _ptr(out), _stream_ptr())
        else:
            rc = lib.lcrec_quantizer_input_grad_bias(_ptr(z), _ptr(codebook0), _ptr(idx_col), stride, n, e, float(coef), float(weight),
                                                     _ptr(g_xq), _ptr(out), _ptr(_vec(dbias_out, "dbias_out", e)), _stream_ptr())
    _lib.check(rc, "lcrec_quantizer_input_grad")
    return out


def _flat_check(params, **bufs):
    for name, t in (("params", params),) + tuple(bufs.items()):
        if t is None:
            continue
        if not (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.numel() == params.numel()):
            raise _lib.LcrecError(f"{name} must be a contiguous float32 device buffer of {params.numel()} elements")


def _step_check(step):
    if not (step.is_cuda and step.dtype == torch.int64 and step.numel() == 1):
        raise _lib.LcrecError("step must be a device int64 scalar")


def _optim_step(entry, params, grads, state, extra, step, lr, hyper, clip, schedule, warmup_steps, total_steps, lr_out, skip_flag):
    """What the four optimiser entry points of include/lcrec.h share: (params, grads, the rule's state buffers `state`
    {name: flat buffer | None} and further pointers `extra`, count, clip, step, lr, the rule's hyper-parameters `hyper`,
    schedule, warmup_steps, total_steps, lr_out, ticket, skip_flag, stream)."""
    lib = _lib.load()
    _flat_check(params, grads=grads, **state)
    _step_check(step)
    with _on(params.device):
        rc = getattr(lib, entry)(_ptr(params), _ptr(grads), *[_ptr(t) for t in (*state.values(), *extra)], params.numel(),
                                 _ptr(clip), _ptr(step), float(lr), *hyper, int(schedule), int(warmup_steps), int(total_steps),
                                 _ptr(lr_out), _ptr(_ticket(params.device)), _ptr(skip_flag), _stream_ptr())
    _lib.check(rc, entry)


def adamw_step(params, grads, exp_avg, exp_avg_sq, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=True,
               clip=None, schedule=-1, warmup_steps=0, total_steps=0, lr_out=None, skip_flag=None):
    """One AdamW/Adam step on flat fp32 buffers, all updated in place (see lcrec_adamw_step); `step` is a device int64
    scalar the call increments.  skip_flag: a device bool/uint8 scalar; when set nothing is updated."""
    _optim_step("lcrec_adamw_step", params, grads, dict(exp_avg=exp_avg, exp_avg_sq=exp_avg_sq), (), step, lr,
                (float(betas[0]), float(betas[1]), float(eps), float(weight_decay), int(bool(decoupled))),
                clip, schedule, warmup_steps, total_steps, lr_out, skip_flag)


def sgd_step(params, grads, step, lr, momentum=0.0, dampening=0.0, nesterov=False, weight_decay=0.0, momentum_buffer=None,
             momentum_ready=None, clip=None, schedule=-1, warmup_steps=0, total_steps=0, lr_out=None, skip_flag=None):
    """One torch.optim.SGD step on flat fp32 buffers, updated in place (see lcrec_sgd_step).  With momentum != 0:
    momentum_buffer (flat fp32) and momentum_ready (a device bool/uint8 scalar, False until the buffer holds a value --
    torch's first step sets buf = g -- and set by the call)."""
    if momentum_ready is not None and not (momentum_ready.is_cuda and momentum_ready.element_size() == 1 and momentum_ready.numel() == 1):
        raise _lib.LcrecError("momentum_ready must be a device bool/uint8 scalar")
    _optim_step("lcrec_sgd_step", params, grads, dict(momentum_buffer=momentum_buffer), (momentum_ready,), step, lr,
                (float(momentum), float(dampening), int(bool(nesterov)), float(weight_decay)),
                clip, schedule, warmup_steps, total_steps, lr_out, skip_flag)


def adagrad_step(params, grads, state_sum, step, lr, lr_decay=0.0, eps=1e-10, weight_decay=0.0, clip=None, schedule=-1,
                 warmup_steps=0, total_steps=0, lr_out=None, skip_flag=None):
    """One torch.optim.Adagrad step on flat fp32 buffers, updated in place (see lcrec_adagrad_step)."""
    _optim_step("lcrec_adagrad_step", params, grads, dict(state_sum=state_sum), (), step, lr,
                (float(lr_decay), float(eps), float(weight_decay)), clip, schedule, warmup_steps, total_steps, lr_out, skip_flag)


def rmsprop_step(params, grads, square_avg, step, lr, alpha=0.99, eps=1e-8, weight_decay=0.0, momentum=0.0, centered=False,
                 momentum_buffer=None, grad_avg=None, clip=None, schedule=-1, warmup_steps=0, total_steps=0, lr_out=None,
                 skip_flag=None):
    """One torch.optim.RMSprop step on flat fp32 buffers, updated in place (see lcrec_rmsprop_step); momentum_buffer
    exactly when momentum > 0, grad_avg exactly when centered."""
    _optim_step("lcrec_rmsprop_step", params, grads, dict(square_avg=square_avg, momentum_buffer=momentum_buffer, grad_avg=grad_avg),
                (), step, lr, (float(alpha), float(eps), float(weight_decay), float(momentum), int(bool(centered))),
                clip, schedule, warmup_steps, total_steps, lr_out, skip_flag)


def dropout_threshold(p):
    """(T, s) of include/lcrec.h's keep rule for a drop probability 0 <= p < 1: an element is kept iff its Philox word
    u >= T = min(2^32 - 1, floor(p * 2^32)), and a kept value is x * s, s = (float)(1 / (1 - p))."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise _lib.LcrecError(f"dropout: p must satisfy 0 <= p < 1, got {p}")
    return min(2 ** 32 - 1, int(p * 4294967296.0)), 1.0 / (1.0 - p)


def _i64_scalar(v, name, device):
    """A device int64 scalar: `v` itself if it is one, else a new one holding the Python integer `v` (wrapped to 64 bits)."""
    if isinstance(v, torch.Tensor):
        if not (v.is_cuda and v.dtype == torch.int64 and v.numel() == 1):
            raise _lib.LcrecError(f"{name} must be a device int64 scalar (or a Python int)")
        return v
    v = int(v) & (2 ** 64 - 1)
    return torch.tensor(v - 2 ** 64 if v >= 2 ** 63 else v, dtype=torch.int64, device=device)


def _dropout_shape(shape, name):
    if len(shape) != 2 or shape[1] < 4 or shape[1] % 4:
        raise _lib.LcrecError(f"{name}: expected [rows, features] with features a positive multiple of 4, got {tuple(shape)}")
    return int(shape[0]), int(shape[1])


def dropout_apply(x, p, seed, step, position, row_offset=0, out=None):
    """mask * x * s for the mask of (seed, step, position) -- lcrec_dropout_apply; the backward of it is the same call on the
    gradient.  seed, step: device int64 scalars the kernel reads when it runs (or Python ints).  out: None (a new tensor), x
    itself (in place) or another contiguous tensor of x's shape."""
    lib = _lib.load()
    T, s = dropout_threshold(p)
    x = _dev(x, "x")
    n, F = _dropout_shape(x.shape, "dropout_apply")
    if out is None:
        out = torch.empty_like(x)
    elif not (out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.shape == x.shape):
        raise _lib.LcrecError("out must be a contiguous float32 device tensor of x's shape")
    with _on(x.device):
        # (held in names until the call is made: a temporary's block would go back to the allocator, and to the next one)
        seed, step = _i64_scalar(seed, "seed", x.device), _i64_scalar(step, "step", x.device)
        rc = lib.lcrec_dropout_apply(_ptr(x), _ptr(out), n, F, T, s, _ptr(seed), _ptr(step), int(position), int(row_offset),
                                     _stream_ptr())
    _lib.check(rc, "lcrec_dropout_apply")
    return out


def dropout_mask(shape, p, seed, step, position, row_offset=0, device=None):
    """uint8 [rows, features]: 1 where dropout_apply keeps the element for (seed, step, position) -- lcrec_dropout_mask."""
    lib = _lib.load()
    T, _ = dropout_threshold(p)
    n, F = _dropout_shape(tuple(shape), "dropout_mask")
    if device is None:
        device = seed.device if isinstance(seed, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    keep = torch.empty((n, F), dtype=torch.uint8, device=device)
    with _on(device):
        seed, step = _i64_scalar(seed, "seed", device), _i64_scalar(step, "step", device)       # (see dropout_apply)
        rc = lib.lcrec_dropout_mask(_ptr(keep), n, F, T, _ptr(seed), _ptr(step), int(position), int(row_offset), _stream_ptr())
    _lib.check(rc, "lcrec_dropout_mask")
    return keep


_CAST_DTYPES = {torch.float16: _lib.CONSTANTS["LCREC_DTYPE_F16"], torch.float64: _lib.CONSTANTS["LCREC_DTYPE_F64"]}


def cast_rows(src, out=None):
    """float32 copy of a contiguous float16 / float64 device tensor -- lcrec_cast_rows: what numpy's astype(float32) gives,
    bit for bit, made in HBM.  out: None (a new tensor of src's shape) or a contiguous float32 tensor on src's device with as
    many elements, of any shape (a row range `matrix[lo:hi]` of a larger one is fine); src and out must not overlap."""
    lib = _lib.load()
    if not isinstance(src, torch.Tensor) or not src.is_cuda:
        raise _lib.LcrecError("src must be a tensor on a HIP device (lcrec_amd has no CPU path)")
    code = _CAST_DTYPES.get(src.dtype)
    if code is None:
        raise _lib.LcrecError(f"src must be float16 or float64, got {src.dtype}")
    if not src.is_contiguous():
        raise _lib.LcrecError("src must be contiguous")
    if out is None:
        out = torch.empty(src.shape, dtype=torch.float32, device=src.device)
    elif not (isinstance(out, torch.Tensor) and out.device == src.device and out.is_contiguous() and out.dtype == torch.float32
              and out.numel() == src.numel()):
        raise _lib.LcrecError("out must be a contiguous float32 tensor on src's device with src's number of elements")
    with _on(src.device):
        rc = lib.lcrec_cast_rows(_ptr(src), code, src.numel(), _ptr(out), _stream_ptr())
    _lib.check(rc, "lcrec_cast_rows")
    return out


def trace_enable(on=True):
    """Bracket every kernel launch with hipEvents (include/lcrec.h, lcrec_trace_enable)."""
    _lib.check(_lib.load().lcrec_trace_enable(int(bool(on))), "lcrec_trace_enable")


def trace_collect():
    """{kernel name: (launches, total_ms)} since trace_enable(); waits for the recorded events."""
    buf = (_lib.TraceEntry * 32)()
    n = _lib.load().lcrec_trace_collect(ctypes.cast(buf, ctypes.c_void_p), 32)
    if n < 0:
        _lib.check(n, "lcrec_trace_collect")
    return {buf[i].kernel.decode(): (int(buf[i].launches), float(buf[i].total_ms)) for i in range(n)}


def _check_names(constants):
    """The display-name tables above against the header's enumerators of their prefix (`constants` of _lib.parse_header): one
    name per enumerator, numbered 0 .. len-1 -- so an enumerator added in C without its name here fails at import."""
    for what, names, prefix in (("GEMM_ROLES", GEMM_ROLES, "LCREC_GEMMR_"), ("GEMM_FAMILIES", GEMM_FAMILIES, "LCREC_GEMMK_"),
                                ("BN_CALLS", BN_CALLS, "LCREC_BN_"), ("TAIL_CALLS", TAIL_CALLS, "LCREC_TAIL_"),
                                ("TAIL_FAMILIES", TAIL_FAMILIES, "LCREC_TAILK_"), ("SK_TABLE_TRANSPORTS", SK_TABLE_TRANSPORTS, "LCREC_SK_TABLE_")):
        declared = {k: v for k, v in constants.items() if k.startswith(prefix)}
        if sorted(declared.values()) != (sorted(names) if isinstance(names, dict) else list(range(len(names)))):
            raise _lib.LcrecError(f"ops.{what} names {len(names)} values, include/lcrec.h declares {prefix}* as {declared}")


_check_names(_lib.CONSTANTS)
