"""CPU: the launch-side rules of csrc/gemm_f32.hip that are part of an arithmetic contract, restated and compared with
the library's exported pure functions -- nothing is launched."""
import os

CAP = int(os.environ.get("LCREC_GEMM_SPLITK", "16"))        # the library's default cap on S is 16


def _cdiv(a, b):
    return -(-a // b)


def _forward_tile(M, N):
    """The forward rule: the tile shape of an [M][N] output of the generic kernel."""
    if N > 64:
        if _cdiv(M, 128) * _cdiv(N, 128) >= 512:
            return "128x128"
        return "64x128" if _cdiv(M, 64) * _cdiv(N, 128) >= 256 else "64x64"
    if N > 32:
        return "64x64" if _cdiv(M, 128) < 256 else "128x64"
    return "128x32"


def _splits(n, in_dim, out_dim, real_tiles=False):
    """S of lcrec_linear_backward_splits: dW is an [out_dim][in_dim] output; its tiles are counted in the shape the forward
    rule gives it -- except that a 64x128 launch is counted as 128x32 tiles (real_tiles=True: as what it is)."""
    shape = _forward_tile(out_dim, in_dim)
    bm, bn = {"64x64": (64, 64), "128x128": (128, 128), "128x64": (128, 64), "128x32": (128, 32),
              "64x128": (64, 128) if real_tiles else (128, 32)}[shape]
    tiles = _cdiv(out_dim, bm) * _cdiv(in_dim, bn)
    nk = _cdiv(n, 32)
    s = min(512 // max(tiles, 1), nk // 4, CAP)
    if s < 2:
        return 1
    per = _cdiv(nk, s)                # K-tiles per run; no run is empty
    return _cdiv(nk, per)


def test_linear_backward_splits_is_the_documented_rule():
    """S = lcrec_linear_backward_splits(n, in_dim, out_dim) decides how many fma chains a weight-gradient element is the
    ordered sum of, so it is part of lcrec_linear_backward's arithmetic contract.  The grid covers every tile shape the
    rule can pick for a dW output, batches below and above the 4-K-tiles-per-run limit, and layers whose dW goes out on
    64x128 tiles but is counted as 128x32 tiles -- among them some where counting the real tiles would change S (those
    have exactly 256 tiles of 64x128, i.e. a 2048 x 1024 gradient: hence the width 1024 in the grid)."""
    import lcrec_amd
    lib = lcrec_amd._lib.load()
    dims = (4, 32, 36, 64, 68, 128, 132, 768, 1024, 2048, 4096)
    wide, quirk = 0, 0
    for n in (1, 31, 128, 129, 1024, 2048, 16859):
        for in_dim in dims:
            for out_dim in dims:
                want = _splits(n, in_dim, out_dim)
                assert lib.lcrec_linear_backward_splits(n, in_dim, out_dim) == want, (n, in_dim, out_dim, want)
                assert lib.lcrec_linear_backward_workspace(n, in_dim, out_dim) == (want * out_dim * in_dim * 4 if want > 1 else 0)
                wide += _forward_tile(out_dim, in_dim) == "64x128"
                quirk += _splits(n, in_dim, out_dim, real_tiles=True) != want
    assert wide > 0 and quirk > 0, (wide, quirk)
