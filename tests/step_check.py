"""Judging one training step of ANY configuration against oracle/torch_ref.py evaluated at test time: tests/f11_check.py's
rule without a fixture.  The step (forward, loss, backward; trainer.py:111-117) is evaluated on the CPU twice with the codes
FORCED to those the path under test chose -- in fp64, the yardstick, and in fp32, which says how far from it fp32 arithmetic
lands tensor by tensor -- and every parameter gradient of the path has to sit within f11_check.SLACK x that distance
(at least f11_check.FLOOR) of the fp64 one; a tensor whose true gradient is zero (a Linear bias in front of BatchNorm) is
rounding noise, bounded by f11_check.NOISE x the fp32 evaluation's.  Full tensors, no sampling.  Forcing the codes must not
hide a wrong assignment kernel, so the path's codes are compared with the fp32 evaluation's own (unforced) ones."""
import numpy as np
import torch

from f11_check import FLOOR, NOISE, SLACK, table  # noqa: F401  (table: the same per-tensor print-out)
from oracle import torch_ref


def spec_of(c, sk_iters):
    """torch_ref.Spec of a golden_inputs.SUPPORT_MATRIX-style configuration dict."""
    return torch_ref.Spec(c["in_dim"], c["codes"], c["e_dim"], c["layers"], bn=c["bn"], loss_type=c["loss"],
                          quant_loss_weight=c["qlw"], beta=c["beta"], sk_epsilons=c["sk"], sk_iters=sk_iters)


def _leaves(sd, dtype):
    leaf = {}
    for k, v in sd.items():
        v = torch.from_numpy(np.array(v))
        if v.dtype.is_floating_point:
            v = v.to(dtype)
            if "running" not in k:
                v.requires_grad_(True)
        leaf[k] = v
    return leaf


def evaluate(spec, sd, x, idx, dtype, masks=None):
    """The step with the codes forced to `idx` [rows, levels] in `dtype`: ([loss, recon, rq_loss, gradient norm], name ->
    gradient as float64 array).  `sd`: name -> numpy array (left as it is); masks: torch_ref.mlp's."""
    leaf = _leaves(sd, dtype)
    xt = torch.from_numpy(np.asarray(x)).to(dtype)
    out, rq_loss, _ = torch_ref.forward(spec, leaf, xt, use_sk=True, training=True, force_idx=torch.from_numpy(np.asarray(idx)),
                                        masks=masks)
    loss, recon = torch_ref.compute_loss(spec, out, rq_loss, xt)
    loss.backward()
    grads = {k: v.grad.double().numpy() for k, v in leaf.items() if v.requires_grad}
    norm = np.sqrt(sum(float((g ** 2).sum()) for g in grads.values()))
    return [loss.item(), recon.item(), rq_loss.item(), norm], grads


def free_codes(spec, sd, x, dtype=torch.float32, masks=None):
    """The codes the CPU evaluation itself chooses (argmin / Sinkhorn, nothing forced): int64 [rows, levels]."""
    leaf = _leaves(sd, dtype)
    with torch.no_grad():
        _, _, idx = torch_ref.forward(spec, leaf, torch.from_numpy(np.asarray(x)).to(dtype), use_sk=True, training=True, masks=masks)
    return idx.numpy()


def report(grads, g64, g32):
    """f11_check.report on full tensors: rows (name, kind, path distance, reference-fp32 distance, bound) and the violations."""
    rows, bad = [], []
    assert sorted(grads) == sorted(g64), (sorted(grads), sorted(g64))
    for k in g64:
        t64, t32 = g64[k].reshape(-1), g32[k].reshape(-1)
        tp = np.asarray(grads[k]).astype(np.float64).reshape(-1)
        assert tp.shape == t64.shape, (k, tp.shape, t64.shape)
        n64, n32 = np.linalg.norm(t64), np.linalg.norm(t32)
        if n64 < 1e-6 * n32 or n64 == 0.0:         # the true gradient is zero; the fp32 values are pure rounding noise
            path, ref, bound, kind = np.linalg.norm(tp), n32, NOISE * n32, "noise"
        else:
            path, ref = np.linalg.norm(tp - t64) / n64, np.linalg.norm(t32 - t64) / n64
            bound, kind = SLACK * max(ref, FLOOR), "rel"
        rows.append((k, kind, path, ref, bound))
        if not path <= bound:
            bad.append((k, kind, path, ref, bound))
    return rows, bad


class Judge:
    """One configuration's yardsticks, computed once per (codes, masks) and shared by every path and step judged on it."""

    def __init__(self, spec, sd, x, exact_codes):
        """exact_codes: the path's codes must be the fp32 evaluation's on every row (else: on all but at most one)."""
        self.spec, self.sd, self.x, self.exact_codes = spec, sd, x, exact_codes
        self._cache = {}

    def yardsticks(self, idx, masks=None, mask_key=None):
        key = (np.asarray(idx).tobytes(), mask_key)
        if key not in self._cache:
            free = free_codes(self.spec, self.sd, self.x, masks=masks)
            s64, g64 = evaluate(self.spec, self.sd, self.x, idx, torch.float64, masks)
            _, g32 = evaluate(self.spec, self.sd, self.x, idx, torch.float32, masks)
            self._cache[key] = (free, s64, g64, g32)
        return self._cache[key]

    def __call__(self, grads, scalars, idx, what, masks=None, mask_key=None):
        """grads: name -> gradient of the path (before clipping); scalars: its [loss, recon, rq_loss, gradient norm before
        clipping]; idx: the codes it chose.  mask_key: anything hashable naming `masks` (the step they were drawn for)."""
        idx = np.asarray(idx).astype(np.int64)
        free, s64, g64, g32 = self.yardsticks(idx, masks, mask_key)
        differ = int((idx != free).any(1).sum())
        rows, bad = report(grads, g64, g32)
        print(f"\n[{what}] rows assigned differently from the fp32 evaluation's own codes: {differ} of {idx.shape[0]}; "
              f"loss, recon, rq_loss, norm: path {['%.9g' % v for v in scalars]} fp64 {['%.9g' % v for v in s64]}\n" + table(rows))
        assert differ <= (0 if self.exact_codes else 1), (what, differ)
        np.testing.assert_allclose(scalars[:3], s64[:3], rtol=1e-5, err_msg=what)         # loss, recon, rq_loss
        np.testing.assert_allclose(scalars[3], s64[3], rtol=1e-4, err_msg=what)           # gradient norm before clipping
        assert not bad, what + "\n" + table(bad)
        return rows
