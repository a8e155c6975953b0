"""Judging one training step of ANY configuration against oracle/torch_ref.py evaluated at test time: tests/f11_check.py's
rule without a fixture.  The step (forward, loss, backward; trainer.py:111-117) is evaluated on the CPU twice with the codes
FORCED to those the path under test chose -- in fp64, the yardstick, and in fp32, which says how far from it fp32 arithmetic
lands tensor by tensor -- and every parameter gradient of the path has to sit within f11_check.SLACK x that distance
(at least f11_check.FLOOR) of the fp64 one; a tensor whose true gradient is zero (a Linear bias in front of BatchNorm) is
rounding noise, bounded by f11_check.NOISE x the fp32 evaluation's.  Full tensors, no sampling.

Forcing the codes must not hide a wrong assignment kernel.  The path's codes are compared with the fp32 evaluation's own
(unforced) ones, and the rows that differ are capped by a count; on top of that EVERY assigned code is judged by its fp64
regret (CodeRule below).  The two forced evaluations hand over, through torch_ref.rq's hook, the residual R_l entering each
level, and from it a cost matrix C [rows, K] per level and dtype, held as float64, in torch_ref.vq's own expressions:

    argmin level (sk_epsilon <= 0)   C = torch_ref.distances(R_l, codebook_l)
    Sinkhorn level                   C = -ln Q,  Q = torch_ref.sinkhorn(torch_ref.centre_distances(d).double(), eps, iters),
                                     d as above in the evaluation's dtype

With b_i the first minimum of C64[i, :] and D = |C32 - C64|, code k is ACCEPTABLE for row i iff

    C64[i, k] - C64[i, b_i]  <=  SLACK * (D[i, k] + D[i, b_i]) + floor(i, k)

SLACK is f11_check.SLACK: a path may sit that many times further from fp64 than the reference's own fp32 evaluation does.  D
is per row and per code -- what fp32 arithmetic does to the very two numbers being compared -- and is measured on the
reference evaluation, never on the device.  floor on an argmin level is 2^-22 * (||R64_i||^2 + ||c_k||^2): four fp32 ulps at
the magnitude at which that distance is rounded, the scale of lcrec.h's near-tie word; on a Sinkhorn level it is 1e-9, the
margin lcrec.h states for the solver forms.  A row with one acceptable code is decidable: only b_i passes there, whatever the
count caps would still allow.  tests/test_step_check_host.py shows that the reference alone satisfies the rule, that
undecidable rows are rare, and that the rule refuses a decidable row sent anywhere else."""
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


def level_costs(residual, codebook, sk_epsilon, sk_iters):
    """One level's cost matrix in the dtype of `residual` and `codebook`, in torch_ref.vq's own expressions, held as float64:
    (C [rows, K], ||R_i||^2 [rows], ||c_k||^2 [K]) as arrays; the two norms are taken in float64 (CodeRule's floor)."""
    with torch.no_grad():
        r, cb = residual.detach().reshape(-1, codebook.shape[1]), codebook.detach()
        d = torch_ref.distances(r, cb)
        if sk_epsilon > 0:
            C = -torch.log(torch_ref.sinkhorn(torch_ref.centre_distances(d).double(), sk_epsilon, sk_iters))
        else:
            C = d.double()
        return C.numpy(), (r.double() ** 2).sum(1).numpy(), (cb.double() ** 2).sum(1).numpy()


def evaluate(spec, sd, x, idx, dtype, masks=None, costs=None):
    """The step with the codes forced to `idx` [rows, levels] in `dtype`: ([loss, recon, rq_loss, gradient norm], name ->
    gradient as float64 array).  `sd`: name -> numpy array (left as it is); masks: torch_ref.mlp's.  `costs`: a list that
    receives level_costs of every level of this very evaluation, in order (through torch_ref.rq's hook)."""
    leaf = _leaves(sd, dtype)
    xt = torch.from_numpy(np.asarray(x)).to(dtype)
    hook = None
    if costs is not None:
        books = spec.codebooks(leaf)
        hook = lambda l, residual, _: costs.append(level_costs(residual, books[l], spec.sk_epsilons[l], spec.sk_iters))
    out, rq_loss, _ = torch_ref.forward(spec, leaf, xt, use_sk=True, training=True, hook=hook,
                                        force_idx=torch.from_numpy(np.asarray(idx)), masks=masks)
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


ARGMIN_FLOOR = 2.0 ** -22     # x (||R64_i||^2 + ||c_k||^2): four fp32 ulps where that distance is rounded (lcrec.h's near-tie word)
SINKHORN_FLOOR = 1e-9         # in -ln Q: the margin lcrec.h states for the solver forms


class CodeRule:
    """Which codes are acceptable per row and level (this module's docstring), from the level_costs of the fp64 and the fp32
    evaluation with the SAME forced codes.  Per level: best [n] (the first minimum of C64), regret, threshold and ok [n, K],
    margin [n] (fp64 runner-up minus best), finite (every cost of both evaluations)."""

    def __init__(self, spec, costs64, costs32):
        assert len(costs64) == len(costs32) == spec.levels, (len(costs64), len(costs32), spec.levels)
        self.levels = []
        for l, ((c64, rr, cc), (c32, _, _)) in enumerate(zip(costs64, costs32)):
            assert c64.shape == c32.shape and c64.dtype == c32.dtype == np.float64, (l, c64.shape, c32.shape)
            rows = np.arange(c64.shape[0])
            with np.errstate(invalid="ignore"):                # (inf - inf of a non-finite cost: refused below as not finite)
                best = c64.argmin(1)
                D = np.abs(c32 - c64)
                floor = SINKHORN_FLOOR if spec.sk_epsilons[l] > 0 else ARGMIN_FLOOR * (rr[:, None] + cc[None, :])
                regret = c64 - c64[rows, best][:, None]
                threshold = SLACK * (D + D[rows, best][:, None]) + floor
                two = np.sort(c64, 1)[:, :2]
            self.levels.append(dict(best=best, regret=regret, threshold=threshold, ok=regret <= threshold,
                                    margin=two[:, 1] - two[:, 0] if c64.shape[1] > 1 else np.full(len(rows), np.inf),
                                    finite=bool(np.isfinite(c64).all() and np.isfinite(c32).all())))

    def undecidable(self, level):
        """Rows of `level` with more than one acceptable code."""
        return np.flatnonzero(self.levels[level]["ok"].sum(1) > 1)

    def check(self, idx, what):
        """Every code of `idx` [n, L] must be acceptable.  Refuses with the row, the level, the regret, the threshold and the
        row's fp64 top-2 margin; else prints and returns, per level, (rows where idx != best, the largest regret / threshold
        among them, rows with more than one acceptable code)."""
        idx = np.asarray(idx).astype(np.int64)
        assert idx.shape == (len(self.levels[0]["best"]), len(self.levels)), (what, idx.shape)
        bad, stats = [], []
        for l, v in enumerate(self.levels):
            assert v["finite"], f"{what}: level {l}: a cost of the reference evaluations is not finite"
            rows = np.arange(idx.shape[0])
            assert 0 <= idx[:, l].min() and idx[:, l].max() < v["ok"].shape[1], (what, l)
            regret, threshold = v["regret"][rows, idx[:, l]], v["threshold"][rows, idx[:, l]]
            for i in np.flatnonzero(~v["ok"][rows, idx[:, l]]):
                bad.append(f"row {i} level {l}: code {idx[i, l]} is not acceptable: fp64 regret {regret[i]:.6e} > threshold "
                           f"{threshold[i]:.6e} (fp64 best code {v['best'][i]}, fp64 top-2 margin {v['margin'][i]:.6e})")
            moved = np.flatnonzero(idx[:, l] != v["best"])
            stats.append((len(moved), float((regret[moved] / threshold[moved]).max()) if len(moved) else 0.0,
                          len(self.undecidable(l))))
        assert not bad, f"{what}: {len(bad)} assigned code(s) refused by their fp64 regret\n" + "\n".join(bad[:16])
        print(f"[{what}] codes by fp64 regret, per level (rows off the fp64 best, largest regret / threshold among them, rows with "
              f"more than one acceptable code): " + "; ".join(f"L{l}: {m}, {r:.3g}, {u}" for l, (m, r, u) in enumerate(stats)))
        return stats


class Judge:
    """One configuration's yardsticks, computed once per (codes, masks) and shared by every path and step judged on it."""

    def __init__(self, spec, sd, x, exact_codes):
        """exact_codes: the path's codes must be the fp32 evaluation's on every row (else: on all but at most one); either way
        every code has to be acceptable by its fp64 regret (CodeRule)."""
        self.spec, self.sd, self.x, self.exact_codes = spec, sd, x, exact_codes
        self._cache = {}

    def yardsticks(self, idx, masks=None, mask_key=None):
        key = (np.asarray(idx).tobytes(), mask_key)
        if key not in self._cache:
            free = free_codes(self.spec, self.sd, self.x, masks=masks)
            c64, c32 = [], []
            s64, g64 = evaluate(self.spec, self.sd, self.x, idx, torch.float64, masks, c64)
            _, g32 = evaluate(self.spec, self.sd, self.x, idx, torch.float32, masks, c32)
            self._cache[key] = (free, s64, g64, g32, CodeRule(self.spec, c64, c32))
        return self._cache[key]

    def __call__(self, grads, scalars, idx, what, masks=None, mask_key=None):
        """grads: name -> gradient of the path (before clipping); scalars: its [loss, recon, rq_loss, gradient norm before
        clipping]; idx: the codes it chose.  mask_key: anything hashable naming `masks` (the step they were drawn for)."""
        idx = np.asarray(idx).astype(np.int64)
        free, s64, g64, g32, rule = self.yardsticks(idx, masks, mask_key)
        differ = int((idx != free).any(1).sum())
        rows, bad = report(grads, g64, g32)
        print(f"\n[{what}] rows assigned differently from the fp32 evaluation's own codes: {differ} of {idx.shape[0]}; "
              f"loss, recon, rq_loss, norm: path {['%.9g' % v for v in scalars]} fp64 {['%.9g' % v for v in s64]}\n" + table(rows))
        assert differ <= (0 if self.exact_codes else 1), (what, differ)
        rule.check(idx, what)                      # ... and a row that does differ has to be a near-tie in fp64: CodeRule
        np.testing.assert_allclose(scalars[:3], s64[:3], rtol=1e-5, err_msg=what)         # loss, recon, rq_loss
        np.testing.assert_allclose(scalars[3], s64[3], rtol=1e-4, err_msg=what)           # gradient norm before clipping
        assert not bad, what + "\n" + table(bad)
        return rows
