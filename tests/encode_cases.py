"""The case table of the encode pass (lcrec_encode_assign of csrc/abi.hip: the batch cut into chunks, chunk c on pipeline c % P, an
activation ping-pong pair per pipeline, the last layer written straight into the latent matrix at row0 * e, one quantiser pass over
all rows), shared by tests/test_encode_plan_host.py (CPU: the plan of every row -- lcrec_debug_encode_assign_plan, the function the
launch code launches by -- tiles the rows and lays the workspace out without overlap) and tests/test_gpu_encode_forms.py (GPU:
every row through lcrec_debug_encode_assign, which takes the chunk size at run time, every output row against the oracle).

Rows of a batch are independent, so ONE oracle evaluation per (model, BatchNorm fold) over all of the model's rows serves every
chunking of every prefix of them: reference() evaluates cpu_oracle.encode_assign once (threads=8, want_margin=True), marks the
arrays read-only, and every row of the table slices it.  tests/test_encode_plan_host.py checks on the small models that the
oracle's result for a prefix is the prefix of its result for all rows, bit for bit.

Model W = [384, 2048, 128, 64, 32], K = [256, 256, 64]: its first layer is the smallest shape the persistent ping-pong GEMM admits
(in_dim a multiple of 64 and >= 384, out_dim a multiple of 128, 4096 rows x 2048 columns = 256 tiles), so a chunk of 4096 rows
takes it, one of 4571 a persistent head and a generic tail (64 x 64 tiles, as chunks of 1000 and 257 rows do), chunks of 33 rows
and the narrow layers the 32 x 64 kernel; N3's first layer takes the 128 x 32 tiles.  The tests do not assume which kernel runs: they ask lcrec_debug_linear_forward_plan for
every chunk and layer and hold the trace to it.  Models N1 = [64, 32] (one Linear: no activation buffer, the last layer is the
first) and N3 = [128, 96, 48, 16] (no width a multiple of a tile width, e = 16), K = [48, 7].

Codebooks: level l is K_l distinct oracle latents (drawn without replacement: with replacement a quarter of the rows tie exactly,
which is legal but hides everything else) scaled by 0.7^l and ordered by norm, then its last two codes are overwritten with copies of two codes of
middling norm (dup_sources), so the items nearest to those codes tie exactly -- in every chunk, on either side of every chunk boundary -- and must take the
lower index with margin 0.

Values: latent, idx, xq and margin must be np.array_equal to the oracle's on all n rows, the near-tie word must be what the oracle's
margin and scale give under TAU (bit l = margin_l <= float32(TAU) * scale_l, as tests/rq_cases.py and tests/test_gpu_neartie.py
state it), the per-level sums of squares are held to rtol 1e-6 (tests/test_gpu_kernels.py::test_encode_assign_bit_exact's bound)."""
from collections import namedtuple

import numpy as np

SSE_RTOL = 1e-6
TAU = 2.0 ** -9                      # the near-tie threshold: flags the exact ties and a few percent of the other rows
PARENT_COMMIT = "9a5c0ce"            # the commit whose build printed PRODUCTION's workspace sizes
HIDDEN = [2048, 1024, 512, 256, 128, 64, 32]
# (name, n, dims, Ks, lcrec_encode_assign_workspace in bytes at PARENT_COMMIT or None)
PRODUCTION = [("C3", 1_000_000, [768] + HIDDEN, [256] * 4, 17_563_877_376),
              ("C4-shard", 1_250_000, [4096] + HIDDEN, [256] * 4, 17_659_877_376),
              ("one-chunk", 524_288, [768] + HIDDEN, [256] * 4, 17_381_203_968),
              ("one-chunk-plus-1", 524_289, [768] + HIDDEN, [256] * 4, 17_381_204_736)]

MODELS = {
    # rows: W's largest case is 4571 + 4571 + 475 (the oracle takes about a second for them with 8 threads)
    "W": dict(dims=[384, 2048, 128, 64, 32], Ks=[256, 256, 64], rows=9617, seed=11),
    "N1": dict(dims=[64, 32], Ks=[48, 7], rows=1500, seed=12),
    "N3": dict(dims=[128, 96, 48, 16], Ks=[48, 7], rows=1500, seed=13),
}

# outs: which optional outputs the call is given -- l latent_out, x xq, s sse, m margin, t neartie (idx always); without `l` the
# latent lives in the workspace slab.  n2: the rows of the second call on the same workspace (fewer chunks).  stream: the calls
# run on a torch stream of their own.  release: ops.release_contexts() first, so the context and its helper streams are rebuilt.
Case = namedtuple("Case", "model n chunk_rows pipelines bn outs n2 stream release note")


def _c(model, n, chunk_rows, pipelines, bn, outs, n2, note, stream=False, release=False):
    assert set(outs) <= set("lxsmt") and n2 < n
    return Case(model, n, chunk_rows, pipelines, bool(bn), outs, n2, bool(stream), bool(release), note)


CASES = [
    # one chunk
    _c("W", 9200, 0, 1, True, "lxsmt", 4096, "the built-in chunk: one chunk, a persistent head and a tail"),
    _c("W", 4096, 5000, 1, False, "l", 300, "chunk_rows > n: one chunk of exactly one round of persistent tiles"),
    _c("N3", 1500, 0, 2, True, "lxt", 77, "P = 2 asked for, one chunk: P falls back to 1"),
    _c("N1", 1500, 4000, 1, False, "xsm", 1, "one Linear, one chunk, latent in the slab"),
    # exact multiples
    _c("W", 8192, 4096, 1, True, "lxs", 4096, "two full chunks on one pipeline"),
    _c("W", 8192, 4096, 2, False, "lmt", 4096, "P = 2, an even chunk count: a persistent chunk on each stream"),
    _c("N3", 1500, 500, 1, False, "lxsmt", 1000, "three full chunks"),
    _c("N1", 1500, 500, 2, True, "", 501, "three full chunks (an odd count) on two pipelines, every optional output NULL"),
    # a ragged last chunk
    _c("W", 8193, 4096, 2, True, "lxsmt", 4097, "P = 2, an odd chunk count, a last chunk of one row"),
    _c("W", 8193, 4096, 1, False, "xm", 8192, "a last chunk of one row, latent in the slab"),
    _c("W", 9617, 4571, 1, False, "xs", 4572, "4571 + 4571 + 475: persistent head and generic tail per chunk, latent in the slab"),
    _c("W", 9617, 4571, 2, True, "lt", 9142, "4571 + 4571 + 475 on two pipelines", stream=True),
    # chunks that are no multiple of any tile height, the last one shorter than 32 rows
    _c("W", 3017, 1000, 2, False, "lxs", 2017, "1000 + 1000 + 1000 + 17", release=True),
    _c("W", 1037, 257, 1, True, "lsm", 300, "4 x 257 + 9"),
    _c("W", 130, 33, 2, True, "xt", 67, "3 x 33 + 31, latent in the slab"),
    _c("N3", 1490, 33, 2, False, "lxsmt", 700, "45 x 33 + 5 on two pipelines"),
    _c("N1", 1037, 257, 2, True, "lm", 515, "one Linear: 4 x 257 + 9 on two pipelines", stream=True),
    # one row per chunk
    _c("N1", 5, 1, 2, False, "lxsmt", 2, "five chunks of one row on two pipelines"),
    _c("N3", 5, 1, 1, True, "sm", 1, "five chunks of one row, latent in the slab"),
]


def dup_sources(K):
    """The two codes of a level of K codes that its last two codes are copies of: of middling norm, so that some rows tie on them
    at every level and most rows do not."""
    return (K - 2) // 2, (K - 2) // 2 + 1


def case_id(c):
    return (f"{c.model}-n{c.n}-c{c.chunk_rows}-p{c.pipelines}-bn{int(c.bn)}-{c.outs or 'idx'}"
            + ("-stream" if c.stream else "") + ("-release" if c.release else ""))


def _frozen(a):
    a.flags.writeable = False
    return a


_models, _references = {}, {}


def model(name, oracle):
    """The inputs of a model as read-only numpy arrays: x [rows][dims[0]], Ws, bs, the folded BatchNorm affines scs / shs (an
    entry for every layer but the last, None for the last) and the codebooks."""
    if name in _models:
        return _models[name]
    m = MODELS[name]
    dims, Ks, rows = m["dims"], m["Ks"], m["rows"]
    rs = np.random.RandomState(m["seed"])
    nl = len(dims) - 1
    x = rs.standard_normal((rows, dims[0])).astype(np.float32)
    Ws = [(rs.standard_normal((dims[l + 1], dims[l])) * np.sqrt(2.0 / (dims[l] + dims[l + 1]))).astype(np.float32) for l in range(nl)]
    bs = [(0.05 * rs.standard_normal(dims[l + 1])).astype(np.float32) for l in range(nl)]
    scs = [(1 + 0.1 * rs.standard_normal(dims[l + 1])).astype(np.float32) if l < nl - 1 else None for l in range(nl)]
    shs = [(0.1 * rs.standard_normal(dims[l + 1])).astype(np.float32) if l < nl - 1 else None for l in range(nl)]
    # codebooks at the scale of the latents: distinct latents of the first rows, the last two codes copies of the first two
    lat = oracle.encode_assign(x[:2048], Ws, bs, [np.zeros((2, dims[-1]), np.float32)], threads=8)["latent"]
    assert len(np.unique(lat, axis=0)) == len(lat)
    cbs = []
    for l, K in enumerate(Ks):
        cb = (lat[rs.choice(len(lat), size=K, replace=False)] * np.float32(0.7 ** l)).astype(np.float32)
        cb = cb[np.argsort((cb.astype(np.float64) ** 2).sum(1), kind="stable")]       # by norm: the residuals of the levels after
        a, b = dup_sources(K)                                                          # the first crowd onto the shortest codes
        cb[K - 1], cb[K - 2] = cb[a], cb[b]
        cbs.append(cb)
    out = dict(name=name, dims=dims, Ks=Ks, rows=rows, x=_frozen(x), Ws=[_frozen(w) for w in Ws], bs=[_frozen(b) for b in bs],
               scs=[s if s is None else _frozen(s) for s in scs], shs=[s if s is None else _frozen(s) for s in shs],
               cbs=[_frozen(c) for c in cbs])
    _models[name] = out
    return out


def reference(name, bn, oracle):
    """The oracle's outputs for ALL rows of the model, evaluated once and read-only: idx, latent, xq, margin, scale (and sse, the
    sums over all rows); every case slices it.  `neartie` is the flag word under TAU."""
    key = (name, bool(bn))
    if key not in _references:
        m = model(name, oracle)
        r = oracle.encode_assign(m["x"], m["Ws"], m["bs"], m["cbs"], m["scs"] if bn else None, m["shs"] if bn else None, threads=8,
                                 want_margin=True)
        flags = r["margin"] <= np.float32(TAU) * r["scale"]
        r["neartie"] = (flags.astype(np.int64) << np.arange(len(m["Ks"]))).sum(1).astype(np.int32)
        _references[key] = {k: _frozen(np.ascontiguousarray(v)) for k, v in r.items()}
    return _references[key]


def expected(case, n, oracle):
    """What a correct call over the first n rows leaves: the reference's first n rows.  The sums of squares are sums over the
    rows of the call, so they come from the oracle's quantiser alone over the reference's first n latents (the same C code; it
    must reproduce the reference's codes and x_q, which is asserted)."""
    ref = reference(case.model, case.bn, oracle)
    out = {k: ref[k][:n] for k in ("idx", "latent", "xq", "margin", "neartie")}
    m = model(case.model, oracle)
    rq = oracle.rq_assign(ref["latent"][:n], m["cbs"])
    assert np.array_equal(rq["idx"], out["idx"]) and np.array_equal(rq["xq"].view(np.uint32), out["xq"].view(np.uint32))
    out["sse"] = rq["sse"]
    return out


def widest_hidden(dims):
    """The widest hidden width (1 for a single Linear): what an activation buffer is sized by."""
    return max(dims[1:-1], default=1)


def align256(v):
    return (v + 255) // 256 * 256


def check_plan(n, dims, Ks, chunk_rows, pipelines, plan, chunks, builtin_chunk):
    """The plan of one call against what include/lcrec.h states: a list of complaints (empty: none)."""
    bad = []
    want_chunk = min(chunk_rows or builtin_chunk, max(n, 1))
    if plan["n"] != n or plan["chunk_rows"] != want_chunk:
        bad.append(f"n {plan['n']}, chunk_rows {plan['chunk_rows']}: want {n}, {want_chunk}")
    count = -(-n // want_chunk)
    if plan["n_chunks"] != count or len(chunks) != count:
        bad.append(f"{plan['n_chunks']} chunks planned, {len(chunks)} listed: want {count}")
    P = max(1, min(pipelines, count, 2))
    if plan["pipelines"] != P:
        bad.append(f"pipelines {plan['pipelines']}: want min({pipelines}, {count} chunks, 2) = {P}")
    row = 0
    for c, k in enumerate(chunks):
        rows = want_chunk if c < count - 1 else n - want_chunk * (count - 1)
        if (k["row0"], k["rows"], k["pipeline"], k["first_act"]) != (row, rows, c % P, 2 * (c % P)):
            bad.append(f"chunk {c}: {k}, want row0 {row}, rows {rows}, pipeline {c % P}, first_act {2 * (c % P)}")
        row += k["rows"]
    if row != n:
        bad.append(f"the chunks cover {row} rows of {n}")
    e = dims[-1]
    if plan["act_bytes"] != align256(want_chunk * widest_hidden(dims) * 4):
        bad.append(f"act_bytes {plan['act_bytes']}: want {want_chunk} x {widest_hidden(dims)} floats rounded up to 256")
    if plan["latent_bytes"] < max(n, 1) * e * 4:
        bad.append(f"latent_bytes {plan['latent_bytes']} < {n} x {e} floats")
    ranges = [(off, off + plan["act_bytes"], f"activation buffer {i}") for i, off in enumerate(plan["act_offset"])]
    ranges.append((plan["latent_offset"], plan["latent_offset"] + plan["latent_bytes"], "latent slab"))
    ranges.append((plan["rq_offset"], plan["rq_offset"] + plan["rq_bytes"], "quantiser workspace"))
    if len(plan["act_offset"]) != 4:
        bad.append(f"{len(plan['act_offset'])} activation buffers: want a pair for each of 2 pipelines")
    for lo, hi, what in ranges:
        if lo % 256 or lo < 0 or hi <= lo or hi > plan["total_bytes"]:
            bad.append(f"{what}: [{lo}, {hi}) is not a 256-byte aligned range inside the {plan['total_bytes']} bytes")
    for i, (lo, hi, what) in enumerate(ranges):
        for lo2, hi2, what2 in ranges[i + 1:]:
            if lo < hi2 and lo2 < hi:
                bad.append(f"{what} [{lo}, {hi}) overlaps {what2} [{lo2}, {hi2})")
    if sum(hi - lo for lo, hi, _ in ranges) != plan["total_bytes"]:
        bad.append(f"the ranges hold {sum(hi - lo for lo, hi, _ in ranges)} bytes, the total is {plan['total_bytes']}")
    return bad


def expected_trace(ops, n, dims, Ks, chunks, cus, want_sse):
    """{trace label: launches} of one call: for every chunk and layer what lcrec_debug_linear_forward_plan lists, then the
    quantiser's launches (and, the pass giving it no ticket, a finishing launch each when the sums of squares are asked for)."""
    out = {}
    for k in chunks:
        for l in range(len(dims) - 1):
            for launch in ops.linear_forward_plan(k["rows"], dims[l], dims[l + 1], cus):
                out[launch["label"]] = out.get(launch["label"], 0) + 1
    launches = ops.rq_assign_plan(n, dims[-1], Ks)["launches"]
    out["rq_assign"] = launches
    if want_sse:
        out["rq_sse_finalize"] = launches
    return out
