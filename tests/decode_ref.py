"""The rule of lcrec_decode_tuples (include/lcrec.h) in numpy, written from the rule, not from the kernels.
1. held code: clamped on the int64 value, flag bit l;  2. q = C_0[h_0], then q + C_l[h_l] in float32, levels ascending;  3. the
decoder, every layer oracle.linear (lcrec_linear_forward's fma chains), ReLU after every layer but the last;  4. d = y - x in
float32 and one chain per row over the columns ascending: fma(d, d, err), or err + |d| for the L1 loss.

The squared chain is oracle.distances(d, zeros((1, w)))[:, 0]: with cc = 0 and dot = 0 the distance (xx + cc) - 2 dot is xx, the fp32
fma chain of d_j * d_j over j ascending from 0.  That holds while d is finite (a square that overflows included: xx = +inf, dot = 0).
For a d that is not finite the oracle's dot = d * 0 is a NaN, which the rule's chain never forms; the rule gives NaN when some d_j is
NaN and otherwise +inf (err never goes below 0, so fma(+-inf, +-inf, err) = +inf and stays), and that is written out below."""
import numpy as np

from oracle import cpu_oracle


def gather_ref(codebooks, idx):
    """-> (q float32 [n, e], flags uint32 [n]): rules 1 and 2"""
    idx = np.asarray(idx, dtype=np.int64)
    n, L = idx.shape
    assert L == len(codebooks) >= 1
    flags = np.zeros(n, np.uint32)
    q = None
    for l, cb in enumerate(codebooks):
        cb = np.ascontiguousarray(cb, dtype=np.float32)
        K = cb.shape[0]
        v = idx[:, l]
        h = np.where(v < 0, 0, np.where(v >= K, K - 1, v))
        flags |= np.where((v < 0) | (v >= K), np.uint32(1 << l), np.uint32(0)).astype(np.uint32)
        with np.errstate(invalid="ignore", over="ignore"):
            q = cb[h].copy() if l == 0 else (q + cb[h]).astype(np.float32)
    return q, flags


def decoder_ref(q, weights, biases, bn_scales=None, bn_shifts=None):
    """rule 3: y float32 [n, w]"""
    nl = len(weights)
    y = q
    for l in range(nl):
        sc = None if bn_scales is None else bn_scales[l]
        sh = None if bn_shifts is None else bn_shifts[l]
        y = cpu_oracle.linear(y, weights[l], None if biases[l] is None else biases[l], sc, sh, relu=l != nl - 1)
    return y


def row_error_ref(y, x, l1=False):
    """rule 4: err float32 [n]"""
    y, x = np.ascontiguousarray(y, dtype=np.float32), np.ascontiguousarray(x, dtype=np.float32)
    n, w = y.shape
    assert x.shape == (n, w)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (y - x).astype(np.float32)
        if l1:
            err = np.zeros(n, np.float32)
            for j in range(w):
                err = (err + np.abs(d[:, j])).astype(np.float32)
            return err
        finite = np.isfinite(d).all(1)
        err = cpu_oracle.distances(np.where(finite[:, None], d, np.float32(0)), np.zeros((1, w), np.float32))[:, 0].copy()
        err[~finite] = np.where(np.isnan(d[~finite]).any(1), np.float32(np.nan), np.float32(np.inf))
    return err


def decode_ref(idx, codebooks, weights, biases, bn_scales=None, bn_shifts=None, x=None):
    """idx int [n, L] (any int64 values), codebooks: list of [K_l, e], the decoder's weights [out_l, in_l] and biases, folded
    BatchNorm affines per layer or None, x [n, w] or None -> dict of xq float32 [n, e], flags uint32 [n], out float32 [n, w] and,
    with x, err (squared chain) and err_l1, float32 [n]."""
    q, flags = gather_ref(codebooks, idx)
    out = {"xq": q, "flags": flags, "out": decoder_ref(q, weights, biases, bn_scales, bn_shifts)}
    if x is not None:
        out["err"] = row_error_ref(out["out"], x, l1=False)
        out["err_l1"] = row_error_ref(out["out"], x, l1=True)
    return out


def recon_report_ref(err_file, err_greedy, held, greedy, flags, in_dim, loss_type, first_item=0, worst=10):
    """The `recon` report of decode_indices from reference arrays alone: float64 host sums of the per-item float32 errors."""
    ef, eg = np.asarray(err_file, dtype=np.float64), np.asarray(err_greedy, dtype=np.float64)
    held, greedy = np.asarray(held, dtype=np.int64), np.asarray(greedy, dtype=np.int64)
    n = len(ef)
    rf, rg = float(ef.sum() / (n * in_dim)), float(eg.sum() / (n * in_dim))
    added = ef - eg
    order = sorted(range(n), key=lambda i: (-added[i], i))[:worst]
    return {"items": n, "in_dim": int(in_dim), "loss_type": loss_type, "recon_file": rf, "recon_greedy": rg,
            "recon_added_rel": rf / rg - 1.0 if rg > 0 else 0.0, "moved_items": int((held != greedy).any(1).sum()),
            "clamped_items": int((np.asarray(flags) != 0).sum()),
            "worst": [{"item": int(i) + first_item, "tuple": held[i].tolist(), "greedy_tuple": greedy[i].tolist(),
                       "err_file": float(ef[i]), "err_greedy": float(eg[i])} for i in order]}
