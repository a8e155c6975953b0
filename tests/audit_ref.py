"""The rule of lcrec_rq_audit (include/lcrec.h) in numpy, on the oracle's distances: written from the rule, not from the kernel.
d = oracle.distances (xx, cc, dot as fp32 fma chains; d = (xx + cc) - 2 dot); a NaN counts as +inf wherever distances are compared and
is reported as +inf; np.argmin takes the first minimum; the residual follows the HELD code by three fp32 operations per element."""
import numpy as np

from oracle import cpu_oracle


def audit_ref(z, codebooks, idx):
    """z [n, e], codebooks: list of [K_l, e], idx int [n, L] (any int64 values) -> dict of d_held, d_best float32 [n, L], rank int32
    [n, L], best int64 [n, L], err float32 [n], resid float32 [n, e] (r_L), flags uint32 [n]."""
    r = np.ascontiguousarray(z, dtype=np.float32).copy()
    idx = np.asarray(idx, dtype=np.int64)
    n, e = r.shape
    L = len(codebooks)
    assert idx.shape == (n, L)
    rows = np.arange(n)
    out = {"d_held": np.empty((n, L), np.float32), "d_best": np.empty((n, L), np.float32), "rank": np.empty((n, L), np.int32),
           "best": np.empty((n, L), np.int64), "flags": np.zeros(n, np.uint32)}
    for l, cb in enumerate(codebooks):
        cb = np.ascontiguousarray(cb, dtype=np.float32)
        K = cb.shape[0]
        d = cpu_oracle.distances(r, cb)                                               # 1. distances
        d = np.where(np.isnan(d), np.float32(np.inf), d)
        h = np.where(idx[:, l] < 0, 0, np.where(idx[:, l] >= K, K - 1, idx[:, l]))    # 2. held code, on the int64 value
        out["flags"] |= np.where((idx[:, l] < 0) | (idx[:, l] >= K), np.uint32(1 << l), np.uint32(0)).astype(np.uint32)
        dh = d[rows, h]                                                               # 3. outputs
        best = np.argmin(d, axis=1)
        out["d_held"][:, l] = dh
        out["best"][:, l] = best
        out["d_best"][:, l] = d[rows, best]
        codes = np.arange(K)[None, :]
        out["rank"][:, l] = (d < dh[:, None]).sum(1) + ((d == dh[:, None]) & (codes < h[:, None])).sum(1)
        c = cb[h]                                                                     # 4. residual: t = c - r; s = r + t; r = r - s
        with np.errstate(invalid="ignore", over="ignore"):
            t = (c - r).astype(np.float32)
            s = (r + t).astype(np.float32)
            r = (r - s).astype(np.float32)
    out["resid"] = r
    out["err"] = cpu_oracle.distances(r, np.zeros((1, e), np.float32))[:, 0].copy()
    return out


def first_divergence(rank):
    """[L] counts: items whose first level with rank > 0 is l."""
    rank = np.asarray(rank)
    n, L = rank.shape
    off = rank > 0
    first = np.where(off.any(1), off.argmax(1), L)
    return [int((first == l).sum()) for l in range(L)]


def report_ref(file, greedy, held, ks):
    """The aggregates of audit_indices' report in float64, formed here from audit_ref's arrays: `file` for the held tuples `held`
    (int64 [n, L]) and `greedy` for the greedy tuples of the same latents.  Every key but the near-tie count and `worst`."""
    rank = file["rank"].astype(np.int64)
    n, L = rank.shape
    held = np.asarray(held, dtype=np.int64)
    counts = np.unique(held, axis=0, return_counts=True)[1]
    dh, db = file["d_held"].astype(np.float64), file["d_best"].astype(np.float64)
    rep = {"items": n, "levels": L, "codes": [int(k) for k in ks], "distinct_tuples": int(counts.size),
           "colliding_items": int(n - counts.size), "max_conflicts": int(counts.max()), "collision_rate": (n - counts.size) / n,
           "clamped_items": int((file["flags"] != 0).sum()), "greedy_items": int((rank == 0).all(1).sum()),
           "first_divergence": first_divergence(rank), "rank0_items": [int((rank[:, l] == 0).sum()) for l in range(L)],
           "rank_max": [int(rank[:, l].max()) for l in range(L)], "rank_mean": [float(rank[:, l].sum() / n) for l in range(L)],
           "regret_mean": [], "codes_used": []}
    for l in range(L):
        ok = np.isfinite(dh[:, l]) & np.isfinite(db[:, l])
        rep["regret_mean"].append(float((dh[ok, l] - db[ok, l]).sum() / ok.sum()) if ok.any() else 0.0)
        rep["codes_used"].append(len(set(np.clip(held[:, l], 0, int(ks[l]) - 1).tolist())))
    ef, eg = file["err"].astype(np.float64), greedy["err"].astype(np.float64)
    ok = np.isfinite(ef) & np.isfinite(eg)
    rep["err_file_mean"] = float(ef[ok].sum() / ok.sum()) if ok.any() else 0.0
    rep["err_greedy_mean"] = float(eg[ok].sum() / ok.sum()) if ok.any() else 0.0
    div = (rank > 0).any(1) & ok
    rep["err_added_mean_diverged"] = float((ef[div] - eg[div]).sum() / div.sum()) if div.any() else 0.0
    rep["early_divergence"] = int(sum(rep["first_divergence"][:max(L - 2, 0)]))
    return rep
