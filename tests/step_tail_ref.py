"""References of the step-tail kernels (csrc/train_ops.hip, csrc/vq_train.hip), in numpy on the CPU, for tests/step_tail_cases.py.

Element-wise outputs: a float32 model of the kernel's own expression, every operation rounded once (the library is built with
-ffp-contract=off and IEEE division and square root), compared bit for bit.  fp64-accumulated scalars: the exact sum (math.fsum over
float64 products, which are exact for float32 factors).  Nothing here reads a GPU result except where a function says so."""
import math

import numpy as np

F32 = np.float32


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def bits(a):
    """The raw bits of a float32 / float64 array, for bit-for-bit comparisons (NaNs and signed zeros included)."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays, exactly: the product of two float32 is exact in float64; the sum is rounded to odd in
    float64 (TwoSum gives the sign of what the addition lost), which float32 rounding then sees as the exact value."""
    a, b, c = (np.asarray(v, dtype=np.float64) for v in (a, b, c))
    s = a * b
    r = s + c
    bb = r - s
    err = (s - (r - bb)) + (c - bb)
    even = (np.ascontiguousarray(r).view(np.int64).reshape(np.shape(r)) & 1) == 0
    toward = np.where(err > 0, np.inf, -np.inf)
    r = np.where((err != 0) & even & np.isfinite(r), np.nextafter(r, toward), r)
    return r.astype(np.float32)


def ulp32(x):
    """The spacing of float32 at |x| (the distance to the next float32 away from zero)."""
    x = np.float32(abs(x))
    return float(np.nextafter(x, np.float32(np.inf)) - x)


def exact_sum(values):
    """The correctly rounded float64 of the exact sum of float64 values."""
    return math.fsum(np.asarray(values, dtype=np.float64).ravel().tolist())


# ---------------------------------------------------------------- recon_loss_grad

def recon_loss_grad(out, x, count_total, l1):
    """(grad float32 model, exact loss as float64, float32 model of the loss): recon_loss_grad_kernel's `one`."""
    d = f32(out) - f32(x)
    ct = F32(count_total)                                   # (float)count_total
    if l1:
        scale = F32(1.0) / ct
        g = np.where(d > 0, scale, np.where(d < 0, -scale, F32(0.0))).astype(np.float32)
        terms = np.abs(d).astype(np.float64)
    else:
        scale = F32(2.0) / ct
        g = d * scale
        terms = d.astype(np.float64) * d.astype(np.float64)
    exact = exact_sum(terms) / float(count_total)
    model = F32(np.sum(terms) / float(count_total))         # fp64 accumulation in numpy's pairwise order
    return g, exact, model


# ---------------------------------------------------------------- grad_norm_clip

def grad_norm(g):
    """(exact norm as float64, float32 model)."""
    t = f32(g).astype(np.float64)
    return math.sqrt(exact_sum(t * t)), F32(math.sqrt(float(np.sum(t * t))))


def clip_coef(norm32, max_norm):
    """norm_and_coef's coefficient from the float32 norm the kernel returned."""
    coef = F32(max_norm) / (F32(norm32) + F32(1e-6))
    return F32(1.0) if coef > F32(1.0) else coef


# ---------------------------------------------------------------- relu_bias_backward

def relu_bias_backward(gy, y, relu):
    """g = gy where y > 0 else +0.0 (relu), gy itself otherwise."""
    gy = f32(gy)
    if not relu:
        return gy.copy()
    return np.where(f32(y) > 0, gy, F32(0.0)).astype(np.float32)


def colsum_bounds(v):
    """(fp64 column sums, per-column bound (n - 1) * 2^-24 * sum |v|): any order of fp32 additions stays inside."""
    v64 = np.asarray(v, dtype=np.float64)
    return v64.sum(0), (v64.shape[0] - 1) * 2.0 ** -24 * np.abs(v64).sum(0)


def colsum_model(v):
    """A float32 column sum in plain row order: one of the orders the bound covers."""
    acc = np.zeros(v.shape[1], dtype=np.float32)
    for row in f32(v):
        acc = acc + row
    return acc


# ---------------------------------------------------------------- quantizer_input_grad, codebook_grad

def quantizer_input_grad(z, cb0, idx, coef, weight, g_xq):
    t = f32(z) - f32(cb0)[np.asarray(idx, dtype=np.int64)]
    u = F32(coef) * t
    v = u * F32(weight)
    return v + f32(g_xq)


def codebook_grad(count, total, cb, scale, weight):
    t = f32(count)[:, None] * f32(cb) - f32(total)
    return (F32(scale) * t) * F32(weight)


# ---------------------------------------------------------------- step_losses

def step_losses(sse, n, e, beta, qlw, recon):
    """out3 = (loss, recon, rq_loss) as float32, step_losses_kernel's order."""
    count = float(n) * float(e)
    beta, qlw, recon = F32(beta), F32(qlw), F32(recon)
    acc = F32(0.0)
    with np.errstate(invalid="ignore"):
        for s in np.asarray(sse, dtype=np.float64):
            mse = F32(s / count)
            acc = acc + (mse + beta * mse)
        rq = acc / F32(len(sse))
        loss = recon + qlw * rq
    return np.array([loss, recon, rq], dtype=np.float32)


# ---------------------------------------------------------------- rq_apply_level, code_stats, ema_update

def clamp_codes(idx, K):
    """The one rule of lcrec_rq_apply_level / lcrec_code_stats(_levels): on the int64 value, below 0 -> 0, >= K -> K - 1."""
    return np.clip(np.asarray(idx, dtype=np.int64), 0, K - 1)


def apply_level(resid, cb, idx, xq_in):
    """(xq, resid_out, exact sse): apply_level_kernel's expression; xq_in None = start from zero."""
    r = f32(resid)
    c = f32(cb)[clamp_codes(idx, cb.shape[0])]
    tt = c - r
    s = r + tt
    xo = (np.zeros_like(r) if xq_in is None else f32(xq_in)) + s
    ro = r - s
    return xo, ro, exact_sum(tt.astype(np.float64) ** 2)


def code_stats(idx, resid, K):
    """count and per-code sums in item order in float32 (np.add.at is unbuffered and sequential)."""
    k = clamp_codes(idx, K)
    resid = f32(resid)
    count = np.bincount(k, minlength=K).astype(np.float32)
    total = np.zeros((K, resid.shape[1]), dtype=np.float32)
    np.add.at(total, k, resid)
    return count, total


def ema_rates(decay):
    """The python-double rates of the reference rounded to float32 at the ABI (ops.ema_update)."""
    return F32(decay), F32(1 - decay), F32(1 - (1 - decay))


def ema_update(ema_count, ema_sum, cb, count, total, decay, eps):
    """(ema_count, ema_sum, codebook, en) after ema_update_kernel."""
    dec, alpha, keep = ema_rates(decay)
    eps = F32(eps)
    en = fma32(f32(count), alpha, f32(ema_count) * dec)
    ew = fma32(f32(total), alpha, f32(ema_sum) * dec)
    with np.errstate(divide="ignore", invalid="ignore"):
        nw = ew / (en + eps)[:, None]
        blended = f32(cb) * keep + nw * alpha
    new_cb = np.where((en > eps)[:, None], blended, f32(cb)).astype(np.float32)
    return en, ew, new_cb, en
