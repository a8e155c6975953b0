"""CPU: the plan of the encode pass (lcrec_debug_encode_assign_plan: the function lcrec_encode_assign walks its chunks and lays its
workspace out by, nothing launched) for every row of tests/encode_cases.py, for both calls a row makes, and for the production
sizes: the chunks tile [0, n) in order, every chunk but the last is full, chunk c is on pipeline c % P with P clipped to the chunk
count, the activation buffers, the latent slab and the quantiser's workspace are disjoint, 256-byte aligned and add up to the
total, which both workspace queries return; the production sizes are byte for byte what the parent commit's build printed; every
refusal comes back with its code and a text naming the argument; and the oracle's result for a prefix of the rows is the prefix of
its result for all rows, which is what lets one evaluation per model serve every row of the table."""
import ctypes
import threading

import numpy as np
import pytest

import encode_cases as ec


@pytest.fixture(scope="module")
def lcrec():
    import lcrec_amd
    lcrec_amd._lib.load()
    return lcrec_amd


def _in_thread(fn):
    """fn() in a thread of its own: the library's last-error text is per thread and is never cleared, and
    tests/test_host_logic.py::test_library_exports_every_declared_symbol asserts that the main thread's is still empty."""
    box = {}

    def run():
        try:
            box["value"] = fn()
        except Exception as exc:                    # noqa: BLE001 -- handed to the caller
            box["error"] = exc
    t = threading.Thread(target=run)
    t.start()
    t.join()
    if "error" in box:
        raise box["error"]
    return box["value"]


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def _queries(lib, n, dims, Ks, chunk_rows):
    d, k = _ints(dims), _ints(Ks)
    return (lib.lcrec_encode_assign_workspace(n, d, len(dims) - 1, k, len(Ks)),
            lib.lcrec_debug_encode_assign_workspace(n, d, len(dims) - 1, k, len(Ks), chunk_rows))


def _check(lcrec, n, dims, Ks, chunk_rows, pipelines):
    lib = lcrec._lib.load()
    builtin = lib.lcrec_encode_assign_chunk_rows()
    plan, chunks = lcrec.ops.encode_plan(n, dims, Ks, chunk_rows=chunk_rows, pipelines=pipelines)
    bad = ec.check_plan(n, dims, Ks, chunk_rows, pipelines, plan, chunks, builtin)
    assert not bad, "\n  ".join(bad) + f"\n  plan: {plan}\n  chunks: {chunks[:8]}"
    production, debug = _queries(lib, n, dims, Ks, chunk_rows)
    assert debug == plan["total_bytes"]
    assert _queries(lib, n, dims, Ks, 0)[1] == production             # chunk_rows = 0 is the built-in chunk
    if chunk_rows in (0, builtin) or n <= min(chunk_rows, builtin):
        assert production == plan["total_bytes"]
    # the quantiser's share is lcrec_rq_assign's own figure, and the layout does not depend on the pipelines asked for
    assert plan["rq_bytes"] == lib.lcrec_rq_assign_workspace(n, dims[-1], _ints(Ks), len(Ks))
    other = lcrec.ops.encode_plan(n, dims, Ks, chunk_rows=chunk_rows, pipelines=3 - pipelines)[0]
    assert {k: v for k, v in other.items() if k != "pipelines"} == {k: v for k, v in plan.items() if k != "pipelines"}
    return plan, chunks


@pytest.mark.parametrize("case", ec.CASES, ids=ec.case_id)
def test_plan_of_every_row(lcrec, case):
    m = ec.MODELS[case.model]
    assert case.n <= m["rows"]
    plan, chunks = _check(lcrec, case.n, m["dims"], m["Ks"], case.chunk_rows, case.pipelines)
    again, fewer = _check(lcrec, case.n2, m["dims"], m["Ks"], case.chunk_rows, case.pipelines)
    # the second call of the GPU test runs in the first call's workspace with fewer chunks
    assert again["total_bytes"] <= plan["total_bytes"] and (len(fewer) < len(chunks) or len(chunks) == 1)


def test_the_table_holds_the_rows_it_is_for(lcrec):
    """One chunk (built-in and chunk_rows > n), exact multiples, ragged last chunks of 1 and of 475 rows, chunks that are no multiple
    of a tile height with a last chunk under 32 rows, one row per chunk, P = 2 with an even count, an odd count and one chunk,
    every optional output given and NULL, a non-default stream, a rebuilt context."""
    builtin = lcrec._lib.load().lcrec_encode_assign_chunk_rows()
    rows = []
    for c in ec.CASES:
        chunk = min(c.chunk_rows or builtin, c.n)
        rows.append((c, chunk, -(-c.n // chunk), c.n - chunk * (-(-c.n // chunk) - 1)))
    assert any(c.chunk_rows == 0 and count == 1 for c, _, count, _ in rows) and any(c.chunk_rows > c.n for c, _, _, _ in rows)
    assert any((c.model, c.n, c.chunk_rows) == ("W", 8192, 4096) for c, _, _, _ in rows)
    assert any((c.n, c.chunk_rows) == (1500, 500) for c, _, _, _ in rows)
    assert any((c.model, c.n, c.chunk_rows, last) == ("W", 8193, 4096, 1) for c, _, _, last in rows)
    assert any((c.model, c.n, c.chunk_rows, count, last) == ("W", 9617, 4571, 3, 475) for c, _, count, last in rows)
    for size in (1000, 257, 33):
        assert any(c.chunk_rows == size and count > 1 and last < 32 for c, _, count, last in rows), size
    assert any((c.model, c.n, c.chunk_rows) == ("N1", 5, 1) for c, _, _, _ in rows)
    two = [(c, count) for c, _, count, _ in rows if c.pipelines == 2]
    assert any(count % 2 == 0 for _, count in two) and any(count % 2 == 1 and count > 1 for _, count in two) and any(count == 1 for _, count in two)
    assert any(c.model == "W" and c.chunk_rows == 4096 and count == 2 for c, count in two)       # a persistent chunk on each stream
    for flag in "lxsmt":
        assert any(flag in c.outs for c in ec.CASES) and any(flag not in c.outs for c in ec.CASES), flag
    assert any(c.bn for c in ec.CASES) and any(not c.bn for c in ec.CASES)
    assert any(c.stream for c in ec.CASES) and any(c.release and c.pipelines == 2 for c in ec.CASES)
    assert len({ec.case_id(c) for c in ec.CASES}) == len(ec.CASES)


def test_model_w_reaches_the_persistent_kernel_and_its_tail(lcrec):
    """What the table's shapes were chosen for, asked of the GEMM's own plan on a 256-CU device: 4096 rows of W's first layer are one
    persistent launch, 4571 rows a persistent head of 4096 and a tail of 475, 1000 rows neither."""
    d = ec.MODELS["W"]["dims"]
    one = lcrec.ops.linear_forward_plan(4096, d[0], d[1], 256)
    assert [(l["family"], l["form"], l["m"]) for l in one] == [("pp", 3, 4096)]
    two = lcrec.ops.linear_forward_plan(4571, d[0], d[1], 256)
    assert [(l["form"], l["row0"], l["m"]) for l in two] == [(3, 0, 4096), (0, 4096, 475)]
    assert all(l["family"] != "pp" for l in lcrec.ops.linear_forward_plan(1000, d[0], d[1], 256))
    families = {l["family"] for rows in (4096, 475, 33, 1) for i in range(4) for l in lcrec.ops.linear_forward_plan(rows, d[i], d[i + 1], 256)}
    assert {"tile_body", "32x64"} <= families


@pytest.mark.parametrize("name,n,dims,Ks,parent_bytes", ec.PRODUCTION, ids=[p[0] for p in ec.PRODUCTION])
def test_production_sizes(lcrec, name, n, dims, Ks, parent_bytes):
    for pipelines in (1, 2):
        plan, chunks = _check(lcrec, n, dims, Ks, 0, pipelines)
        assert plan["chunk_rows"] == min(n, 524288) and len(chunks) == -(-n // 524288)
    # byte for byte what lcrec_encode_assign_workspace returned in a build of commit encode_cases.PARENT_COMMIT
    assert plan["total_bytes"] == parent_bytes
    assert _queries(lcrec._lib.load(), n, dims, Ks, 0) == (parent_bytes, parent_bytes)


def test_refusals_name_their_argument(lcrec):
    lib = lcrec._lib.load()
    E = lcrec._lib.CONSTANTS
    dims, Ks = [64, 48, 32], [48, 7]
    too_many = E["LCREC_MAX_LAYERS"] + 1
    ok = dict(n=100, dims=dims, n_layers=2, K=Ks, L=2, chunk_rows=33, pipelines=2, plan=True, chunks=True, capacity=4)
    refused = [(dict(n=-1), "n < 0"), (dict(n_layers=0), "n_layers=0"), (dict(n_layers=too_many, dims=[32] * (too_many + 1)), f"n_layers={too_many}"),
               (dict(dims=None), "dims"), (dict(K=None), "K"), (dict(L=0), "L=0"), (dict(chunk_rows=-1), "chunk_rows=-1"),
               (dict(pipelines=0), "pipelines=0"), (dict(pipelines=3), "pipelines=3"), (dict(capacity=3), "capacity 3"),
               (dict(plan=False), "plan_out")]

    def call(**change):
        a = dict(ok, **change)
        plan, chunks = lcrec._lib.EncodePlan(), (lcrec._lib.EncodeChunk * 4)()
        rc = lib.lcrec_debug_encode_assign_plan(a["n"], a["dims"] and _ints(a["dims"]), a["n_layers"], a["K"] and _ints(a["K"]), a["L"],
                                                a["chunk_rows"], a["pipelines"], ctypes.addressof(plan) if a["plan"] else None,
                                                ctypes.addressof(chunks) if a["chunks"] else None, a["capacity"])
        return rc, lib.lcrec_last_error().decode(), plan, chunks

    def walk():
        out = [call()]
        out += [call(**change) for change, _ in refused]
        # the workspace queries answer 0 for what the plan refuses; the launch entry refuses chunk_rows < 0 before anything else
        d, k = _ints(dims), _ints(Ks)
        out.append([lib.lcrec_debug_encode_assign_workspace(100, d, 2, k, 2, -1), lib.lcrec_debug_encode_assign_workspace(-1, d, 2, k, 2, 0),
                    lib.lcrec_encode_assign_workspace(100, None, 2, k, 2), lib.lcrec_encode_assign_workspace(100, d, 0, k, 2),
                    lib.lcrec_encode_assign_workspace(100, d, too_many, k, 2), lib.lcrec_encode_assign_workspace(100, d, 2, None, 2),
                    lib.lcrec_encode_assign_workspace(100, d, 2, k, 0)])
        rc = lib.lcrec_debug_encode_assign(None, 100, d, 2, None, None, None, None, None, k, 2, None, None, None, None, None, None, 0.0,
                                           None, 0, None, None, -5)
        out.append((rc, lib.lcrec_last_error().decode()))
        return out

    got = _in_thread(walk)
    rc, _, plan, chunks = got[0]
    assert rc == 0 and plan.n_chunks == 4 and [chunks[c].rows for c in range(4)] == [33, 33, 33, 1]
    for (change, word), (rc, text, _, _) in zip(refused, got[1:]):
        assert rc == E["LCREC_EINVAL"] and word in text and "encode_assign" in text, (change, rc, text)
    assert got[-2] == [0] * 7
    assert got[-1][0] == E["LCREC_EINVAL"] and "chunk_rows=-5" in got[-1][1]
    # chunks_out NULL: the plan alone, capacity not read
    rc, _, plan, _ = _in_thread(lambda: call(chunks=False, capacity=0))
    assert rc == 0 and plan.n_chunks == 4 and plan.pipelines == 2
    with pytest.raises(lcrec.LcrecError, match="chunk_rows=-1"):
        _in_thread(lambda: lcrec.ops.encode_plan(100, dims, Ks, chunk_rows=-1))


@pytest.mark.parametrize("name", ["N1", "N3"])
def test_oracle_prefix_is_the_prefix(oracle, name):
    """Rows are independent in the oracle too: its outputs for the first n rows are the first n rows of its outputs for all rows,
    bit for bit, BatchNorm fold on and off -- and the inputs do what the table says: distinct codes but for the two deliberate
    duplicates per level, whose exact ties (margin 0, lower index) occur on both sides of chunk boundaries."""
    m = ec.model(name, oracle)
    for bn in (False, True):
        ref = ec.reference(name, bn, oracle)
        for n in (1, 33, 500, 1037):
            part = oracle.encode_assign(m["x"][:n], m["Ws"], m["bs"], m["cbs"], m["scs"] if bn else None, m["shs"] if bn else None,
                                        threads=3, want_margin=True)
            for key in ("idx", "latent", "xq", "margin", "scale"):
                assert np.array_equal(part[key], ref[key][:n]), (name, bn, n, key)
        for l, K in enumerate(m["Ks"]):
            cb = m["cbs"][l]
            a, b = ec.dup_sources(K)
            assert np.array_equal(cb[K - 1], cb[a]) and np.array_equal(cb[K - 2], cb[b]) and len(np.unique(cb, axis=0)) == K - 2
            assert not np.isin(ref["idx"][:, l], [K - 1, K - 2]).any()             # the lower index wins
            print(name, bn, "level", l, "exact ties", (ref["margin"][:, l] == 0).mean(), "flagged", ((ref["neartie"] >> l) & 1).mean())
        tied = np.flatnonzero(np.isin(ref["idx"][:, 0], ec.dup_sources(m["Ks"][0])))
        assert (ref["margin"][tied, 0] == 0).all() and ((ref["neartie"][tied] & 1) == 1).all()
        assert (tied < 500).any() and ((tied >= 500) & (tied < 1000)).any() and (tied >= 1000).any()
        assert 0 < (ref["neartie"] != 0).mean() < 0.5 and (ref["margin"] > 0).mean() > 0.5
    assert not np.array_equal(ec.reference(name, False, oracle)["latent"], ec.reference(name, True, oracle)["latent"]) or name == "N1"
