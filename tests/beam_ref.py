"""The rule of lcrec_rq_beam (include/lcrec.h) in numpy, on the oracle's distances: written from the rule, not from the kernel.
d = oracle.distances (xx, cc, dot as fp32 fma chains; d = (xx + cc) - 2 dot); a NaN counts as +inf wherever distances are compared and
is reported as +inf; a stable argsort of the flat candidate index p * K + k breaks ties by parent, then by code; the residual follows
the candidate's code by three fp32 operations per element."""
import numpy as np

from oracle import cpu_oracle


def live_counts(ks, W):
    """[L] live beams after each level: min(W, K[0] * ... * K[l]), capped at W after every level -- W and K alone decide"""
    out, live = [], 1
    for k in ks:
        live = min(W, live * int(k))
        out.append(live)
    return out


def beam_ref(z, cbs, W):
    """z [n, e], cbs: list of [K_l, e], W -> dict of tuples int64 [n, W, L], score, err float32 [n, W], resid float32 [n, W, e];
    rows past the live count hold -1 / +inf."""
    z = np.ascontiguousarray(z, dtype=np.float32)
    n, e = z.shape
    R = z[:, None, :].copy()
    tup = np.zeros((n, 1, 0), np.int64)
    rows = np.arange(n)[:, None]
    score = np.zeros((n, 1), np.float32)
    for cb in cbs:
        cb = np.ascontiguousarray(cb, dtype=np.float32)
        K, P = cb.shape[0], R.shape[1]
        d = cpu_oracle.distances(np.ascontiguousarray(R.reshape(n * P, e)), cb).reshape(n, P * K)
        d = np.where(np.isnan(d), np.float32(np.inf), d)
        order = np.argsort(d, axis=1, kind="stable")[:, :min(W, P * K)]      # flat index p*K+k: ties by p, then k
        par, code = order // K, order % K
        score = d[rows, order]
        c, r = cb[code], R[rows, par]
        with np.errstate(invalid="ignore", over="ignore"):
            t = (c - r).astype(np.float32)
            s = (r + t).astype(np.float32)
            R = (r - s).astype(np.float32)
        tup = np.concatenate([tup[rows, par], code[:, :, None]], axis=2)
    live = R.shape[1]
    err = cpu_oracle.distances(np.ascontiguousarray(R.reshape(-1, e)), np.zeros((1, e), np.float32))[:, 0].reshape(n, live)
    out = {"tuples": np.full((n, W, len(cbs)), -1, np.int64), "score": np.full((n, W), np.inf, np.float32),
           "err": np.full((n, W), np.inf, np.float32), "resid": np.full((n, W, e), np.inf, np.float32)}
    out["tuples"][:, :live] = tup
    out["score"][:, :live] = score
    out["err"][:, :live] = err
    out["resid"][:, :live] = R
    return out


def choose_ref(beams, greedy, err_greedy):
    """The chosen-tuple rule of RQVAE.get_indices_beam: beam 0's tuple unless err_greedy < err_beam0 (strict, a NaN counts as +inf).
    -> (chosen int64 [n, L], err_chosen float32 [n], kept_greedy bool [n])"""
    eg = np.where(np.isnan(err_greedy), np.float32(np.inf), err_greedy)
    eb = np.where(np.isnan(beams["err"][:, 0]), np.float32(np.inf), beams["err"][:, 0])
    keep = eg < eb
    return np.where(keep[:, None], greedy, beams["tuples"][:, 0]), np.where(keep, err_greedy, beams["err"][:, 0]), keep


def stats_ref(chosen, err_chosen, greedy, err_greedy, keep, W):
    """generate(beam=W)'s statistics from the arrays of choose_ref"""
    ok = np.isfinite(err_chosen) & np.isfinite(err_greedy)
    n = len(chosen)
    return {"beam_width": W, "beam_changed": int((chosen != greedy).any(1).sum()), "beam_kept_greedy": int(keep.sum()),
            "beam_err_ratio": float(err_chosen[ok].astype(np.float64).sum() / err_greedy[ok].astype(np.float64).sum()),
            "collision_rate_pass1": (n - len(np.unique(chosen, axis=0))) / n}
