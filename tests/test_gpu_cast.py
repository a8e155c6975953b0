"""MI355X: fp16 / fp64 -> fp32 in HBM (lcrec_cast_rows, ops.cast_rows) and EmbDataset.to_device's device cast.

Every comparison is bitwise: both sides viewed as uint32, except that where numpy's astype(np.float32) of the same array --
the cast the host path and the reference perform -- gives a NaN, a NaN is required and its payload is not compared."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [np.float16, np.float64]
VEC = {np.float16: 8, np.float64: 4}          # elements a thread converts per trip of the 16-byte path (train_ops.hip, CastVec)


def _assert_same_bits(got, src, what=""):
    """got: float32 ndarray from the device; src: the fp16 / fp64 ndarray it was made from."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        want = src.astype(np.float32)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).ravel() & ~nan.ravel())
    assert bad.size == 0, (what, bad[:5], src.ravel()[bad[:5]], got.ravel()[bad[:5]], want.ravel()[bad[:5]])


def _mixed(dtype, count, seed):
    """Values of every magnitude the target can and cannot hold, with zeros, infinities and NaNs sprinkled in."""
    rs = np.random.default_rng(seed)
    if dtype == np.float16:
        return rs.integers(0, 65536, size=count, dtype=np.uint16).view(np.float16)
    with np.errstate(over="ignore"):
        a = rs.standard_normal(count) * 10.0 ** rs.uniform(-45, 39, size=count)
    a[::97] = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, 2.0 ** -150])[np.arange(len(a[::97])) % 7]
    return a


def test_all_fp16_bit_patterns(hip):
    """+-0, every subnormal, 65504, +-inf and every NaN: the 65 536 halves in one call."""
    a = np.arange(65536, dtype=np.uint16).view(np.float16)
    got = hip.ops.cast_rows(torch.from_numpy(a).to(DEV))
    assert got.dtype == torch.float32 and got.shape == (65536,)
    _assert_same_bits(got.cpu().numpy(), a)
    # (fp16 -> fp32 is exact: every finite half widens to the same real number)
    fin = np.isfinite(a)
    assert np.array_equal(got.cpu().numpy()[fin].astype(np.float64), a[fin].astype(np.float64))


def test_fp64_edge_values_round_to_nearest_even(hip):
    fmax = float(np.finfo(np.float32).max)
    edges = np.array([0.0, -0.0, 1.0, -1.0,
                      1 + 2.0 ** -24,                      # a tie: to even, down
                      1 + 3 * 2.0 ** -24,                  # a tie: to even, up
                      1 + 2.0 ** -24 + 2.0 ** -50,         # just above the tie: up
                      fmax, fmax + 2.0 ** 102,             # below the half-ulp boundary: stays finite
                      fmax + 2.0 ** 103,                   # the tie: rounds to inf
                      1e39, -1e39, 2.0 ** -126,
                      1e-40, 2.0 ** -149,                  # fp32 subnormal results: kept, not flushed
                      2.0 ** -150,                         # a tie: rounds to 0
                      1.5 * 2.0 ** -150,                   # rounds to 2^-149
                      1e-320,                              # an fp64 subnormal: rounds to 0
                      np.inf, -np.inf, np.nan], dtype=np.float64)
    rs = np.random.default_rng(20260101)
    with np.errstate(over="ignore"):
        draws = rs.standard_normal(4096) * 10.0 ** rs.uniform(-45, 39, size=4096)
    a = np.concatenate([edges, draws])
    got = hip.ops.cast_rows(torch.from_numpy(a).to(DEV)).cpu().numpy()
    _assert_same_bits(got, a)
    # the expectations spelled out, so that this does not rest on numpy alone
    f = lambda v: np.float32(v).view(np.uint32)
    named = {4: f(1.0), 5: f(1 + 2.0 ** -22), 6: f(1 + 2.0 ** -23), 7: f(fmax), 8: f(fmax), 9: f(np.inf), 10: f(np.inf), 11: f(-np.inf),
             13: np.uint32(71362), 14: np.uint32(1), 15: np.uint32(0), 16: np.uint32(1), 17: np.uint32(0)}
    for i, bits in named.items():
        assert got.view(np.uint32)[i] == bits, (i, a[i], got[i])
    assert got.view(np.uint32)[1] == 0x80000000 and np.isnan(got[20])


COUNTS = [0, 1, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1023, 4099]
SENTINEL = np.uint32(0xDEADBEEF)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_alignment_and_every_tail(hip, dtype):
    """Source and destination are slices of two large buffers (whose starts the allocator aligns to far more than 16 bytes) at every
    element offset that changes either pointer's position inside a 16-byte line; each destination has a region of its own inside
    one sentinel-filled buffer, 8 floats (and more) of sentinel on each side, read back once and required untouched."""
    src_offsets = range(8) if dtype == np.float16 else range(2)
    pool = _mixed(dtype, max(COUNTS) + 8, seed=7)
    src = torch.from_numpy(pool).to(DEV)
    assert src.data_ptr() % 16 == 0
    cases, at = [], 0
    for count in COUNTS:
        for so in src_offsets:
            for do in range(4):
                cases.append((count, so, do, at + 8 + do))            # `at` is a multiple of 4 floats: 16-byte aligned
                at += (8 + 3 + count + 8 + 3) // 4 * 4
    dst = torch.full((at + 8,), int(SENTINEL.astype(np.int64)) - 2 ** 32, dtype=torch.int32, device=DEV).view(torch.float32)
    assert dst.data_ptr() % 16 == 0
    for count, so, do, start in cases:
        out = dst[start:start + count]
        assert count == 0 or (out.data_ptr() % 16 == 4 * do and src[so:].data_ptr() % 16 == (so * pool.itemsize) % 16)
        assert hip.ops.cast_rows(src[so:so + count], out=out) is out
    got = dst.cpu().numpy()
    touched = np.zeros(got.shape, dtype=bool)
    for count, so, do, start in cases:
        _assert_same_bits(got[start:start + count], pool[so:so + count], (dtype.__name__, count, so, do))
        touched[start:start + count] = True
    outside = got.view(np.uint32)[~touched]
    assert outside.size >= 16 * len(cases) and (outside == SENTINEL).all(), "a launch wrote outside its range"


@pytest.mark.parametrize("dtype", DTYPES)
def test_more_elements_than_one_pass_of_the_grid(hip, dtype):
    """The launcher caps the grid at 4 workgroups of 256 threads per CU (dropout_grid in csrc/train_ops.hip: the device's
    multiprocessor count x DROP_BLOCKS_PER_CU), and a thread of the 16-byte path converts one vector -- 8 halves / 4 doubles -- per
    trip.  The count is taken in vectors: cap x 256 of them are one trip for every thread of the capped grid, 300 more put
    four whole waves and part of a fifth on a second trip of the vector loop, and 5 elements behind them are a ragged tail
    (for fp64 one more vector and one element).  The same count from a source one element off runs the one-element-per-thread
    path, which is then several trips deep."""
    cap = torch.cuda.get_device_properties(0).multi_processor_count * 4
    count = (cap * 256 + 300) * VEC[dtype] + 5
    pool = _mixed(dtype, count + 1, seed=8)
    src = torch.from_numpy(pool).to(DEV)
    out = torch.empty(count + 16, dtype=torch.float32, device=DEV)
    for so in (0, 1):
        out.view(torch.int32).fill_(int(SENTINEL.astype(np.int64)) - 2 ** 32)
        hip.ops.cast_rows(src[so:so + count], out=out[8:8 + count])
        got = out.cpu().numpy()
        _assert_same_bits(got[8:8 + count], pool[so:so + count], (dtype.__name__, so))
        assert (got.view(np.uint32)[:8] == SENTINEL).all() and (got.view(np.uint32)[8 + count:] == SENTINEL).all()


def test_cast_rows_checks_its_tensors(hip):
    half = torch.zeros(4, 6, dtype=torch.float16, device=DEV)
    assert hip.ops.cast_rows(half).shape == (4, 6)
    assert hip.ops.cast_rows(half[:0]).shape == (0, 6)
    for bad_src in (half.float(), half.t(), half.to(torch.bfloat16)):
        with pytest.raises(hip.LcrecError):
            hip.ops.cast_rows(bad_src)
    for bad_out in (torch.zeros(4, 5, device=DEV), torch.zeros(4, 6, dtype=torch.float64, device=DEV), torch.zeros(4, 6),
                    torch.zeros(6, 4, device=DEV).t()):
        with pytest.raises(hip.LcrecError):
            hip.ops.cast_rows(half, out=bad_out)


@pytest.mark.parametrize("mmap", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_to_device_converts_in_hbm_chunk_by_chunk(hip, tmp_path, monkeypatch, dtype, mmap):
    """1 003 x 100: an fp16 row is 200 bytes, so rows are not 16-byte aligned, and lo * dim is odd for odd lo."""
    from lcrec_amd.datasets import EmbDataset
    n, dim = 1003, 100
    a = _mixed(dtype, n * dim, seed=9).reshape(n, dim)
    path = str(tmp_path / "T.emb-x-td.npy")
    np.save(path, a)
    calls = []
    real = hip.ops.cast_rows

    def spy(src, out=None):
        calls.append(tuple(src.shape))
        return real(src, out=out)

    monkeypatch.setattr(hip.ops, "cast_rows", spy)
    selections = (None, (301, 1002), (7, 7))
    host = {}
    for rows in selections:
        t = EmbDataset(path, mmap=mmap).to_device(DEV, rows=rows, cast="host")
        host[rows] = (t * 1).cpu().numpy()
        lo, hi = rows or (0, n)
        _assert_same_bits(host[rows], a[lo:hi], ("host", rows))
    assert calls == []
    for chunk in (7, 250):
        for workers in (1, 3):
            for stages in (2, 5):
                for rows in selections:
                    lo, hi = rows or (0, n)
                    for cast in ("auto", "device"):
                        del calls[:]
                        got = EmbDataset(path, mmap=mmap).to_device(DEV, chunk_rows=chunk, rows=rows, workers=workers,
                                                                    stages=stages, cast=cast)
                        res = (got * 1).cpu().numpy()                          # on the current stream, no synchronisation here
                        what = (chunk, workers, stages, rows, cast)
                        assert got.dtype == torch.float32 and got.shape == (hi - lo, dim), what
                        _assert_same_bits(res, a[lo:hi], what)
                        assert np.array_equal(res.view(np.uint32), host[rows].view(np.uint32)), what
                        step = min(chunk, hi - lo)
                        assert calls == [(min(step, hi - lo - s), dim) for s in range(0, hi - lo, step or 1)], what
    # the defaults (one chunk here), and the kept copy
    del calls[:]
    ds = EmbDataset(path, mmap=mmap)
    got = ds.to_device(DEV)
    _assert_same_bits((got * 1).cpu().numpy(), a, "defaults")
    assert calls == [(n, dim)] and ds.to_device(DEV) is got and ds.to_device(DEV, cast="host") is got


@pytest.mark.parametrize("dtype", DTYPES)
def test_to_device_with_an_odd_width_peels_heads_and_falls_back(hip, tmp_path, dtype):
    """101 columns and 7-row chunks: out[lo:hi] starts at lo * 404 bytes, so the chunks meet every destination alignment against
    a raw buffer that is always aligned: the 16-byte path without a head (lo % 4 == 0), with a head of 2 floats (fp64, lo % 4
    == 2), and the one-element path for the rest.  The default chunking (a multiple of 4 rows: one chunk here) stays aligned."""
    from lcrec_amd.datasets import EmbDataset
    n, dim = 203, 101
    a = _mixed(dtype, n * dim, seed=13).reshape(n, dim)
    path = str(tmp_path / "T.emb-x-td.npy")
    np.save(path, a)
    for kwargs in ({"chunk_rows": 7, "workers": 2, "stages": 3}, {"chunk_rows": 7, "rows": (3, 200)}, {}):
        lo, hi = kwargs.get("rows", (0, n))
        got = EmbDataset(path, mmap=True).to_device(DEV, **kwargs)
        res = (got * 1).cpu().numpy()
        _assert_same_bits(res, a[lo:hi], kwargs)
        host = EmbDataset(path, mmap=True).to_device(DEV, cast="host", **kwargs)
        assert np.array_equal(res.view(np.uint32), (host * 1).cpu().numpy().view(np.uint32)), kwargs


def test_to_device_leaves_other_files_on_the_host_path(hip, tmp_path, monkeypatch):
    from lcrec_amd.datasets import EmbDataset
    a = np.random.default_rng(10).standard_normal((1003, 100))
    calls = []
    monkeypatch.setattr(hip.ops, "cast_rows", lambda *args, **kw: calls.append(args) or pytest.fail("device cast on the host path"))
    for name, arr in (("f32", a.astype(np.float32)), ("be", a.astype(">f2")), ("fortran", np.asfortranarray(a))):
        path = str(tmp_path / f"{name}.npy")
        np.save(path, arr)
        for mmap in (True, False):
            got = EmbDataset(path, mmap=mmap).to_device(DEV, chunk_rows=250)
            want = np.asarray(arr).astype(np.float32)
            assert np.array_equal((got * 1).cpu().numpy().view(np.uint32), want.view(np.uint32)), (name, mmap)
            with pytest.raises(ValueError):
                EmbDataset(path, mmap=mmap).to_device(DEV, cast="device")
    assert calls == []


@pytest.mark.parametrize("dtype", DTYPES)
def test_cast_rows_is_capturable(hip, dtype):
    """One graph, two replays, the source refilled in between."""
    count = 4099
    a, b = _mixed(dtype, count, seed=11), _mixed(dtype, count, seed=12)
    src = torch.from_numpy(a).to(DEV)
    out = torch.zeros(count, dtype=torch.float32, device=DEV)
    hip.ops.cast_rows(src[:8])                                   # (library loaded, nothing left to initialise inside the capture)
    gc.collect()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=side):
        hip.ops.cast_rows(src, out=out)
    graph.replay()
    first = out.clone()
    src.copy_(torch.from_numpy(b))
    graph.replay()
    second = out.clone()
    torch.cuda.synchronize()
    _assert_same_bits(first.cpu().numpy(), a, "first replay")
    _assert_same_bits(second.cpu().numpy(), b, "second replay")
    del graph
