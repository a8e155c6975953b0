"""MI355X: the frozen-aware nearest-free-code pass (lcrec_extend_nearest_free, ops.extend_nearest_free, generate(extend=...)).

Every comparison is exact: the kernel and tests/extend_ref.py evaluate the same fp32 fma chains and every tie is defined, so
`idx`, `moved` and `unresolved` must agree bit for bit -- there is no tolerance anywhere in this file.

Buffers: idx carries 64 pre-filled guard rows past n, which must come back untouched; the rows of the new items lie inside a
larger allocation with NaN-filled guard rows before them (n_frozen + 64) and after them (n_frozen + 64).  A kernel that indexed
the residuals by id instead of id - n_frozen, in either direction, would read allocated NaNs and produce a wrong tuple; it could
not read outside an allocation."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

import extend_cases as ec
import finish_cases as fc
import golden_inputs as gi
from extend_ref import extend_ref
from finish_ref import colliding_items

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
FILL = -7


def _tables(hip, idx_dev, ks, buckets=None):
    n, L = idx_dev.shape
    if buckets is not None:
        flat = [i for b in buckets for i in b]
        offs = np.cumsum([0] + [len(b) for b in buckets])
        return torch.tensor(flat, dtype=torch.int64, device=DEV), torch.tensor(offs, dtype=torch.int64, device=DEV)
    if L == 1:
        return torch.arange(n, dtype=torch.int64, device=DEV), torch.tensor([0, n], dtype=torch.int64, device=DEV)
    found = hip.ops.collision_groups(idx_dev[:, :L - 1].contiguous(), ks[:-1], want_groups="device")
    return found["members"], found["offsets"]


def _run(hip, idx, n_frozen, resid_new, cb, ks, buckets=None):
    n, L = idx.shape
    e = cb.shape[1]
    store_i = torch.full((n + GUARD, L), FILL, dtype=torch.int64, device=DEV)
    store_i[:n] = torch.from_numpy(idx)
    d_idx = store_i[:n]
    pad = n_frozen + GUARD
    store_r = torch.full((pad + (n - n_frozen) + pad, e), float("nan"), dtype=torch.float32, device=DEV)
    store_r[pad:pad + n - n_frozen] = torch.from_numpy(resid_new)
    d_res = store_r[pad:pad + n - n_frozen]
    members, offsets = _tables(hip, d_idx, ks, buckets)
    moved, unresolved = hip.ops.extend_nearest_free(d_idx, n_frozen, d_res, torch.from_numpy(cb).to(DEV), ks, members, offsets)
    assert bool((store_i[n:] == FILL).all())                                      # the guard rows past n
    return d_idx.cpu().numpy(), moved, unresolved


def _check(hip, idx, n_frozen, resid_new, cb, ks, what="", buckets=None):
    want, movers, want_unres = extend_ref(idx, n_frozen, resid_new, cb, buckets=buckets)
    got, moved, unresolved = _run(hip, idx, n_frozen, resid_new, cb, ks, buckets)
    print(what, "movers", len(movers), "moved", moved, "unresolved", unresolved, "(reference:", len(movers) - want_unres, want_unres, ")")
    assert (moved, unresolved) == (len(movers) - want_unres, want_unres), what
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]], idx[bad[:8]])
    assert np.array_equal(got[:n_frozen], idx[:n_frozen])                         # frozen rows: bit-identical
    return want, movers, want_unres


@pytest.mark.parametrize("K", [48, 256])
@pytest.mark.parametrize("e", [16, 32, 64])
def test_without_frozen_items_it_is_the_finishing_pass(hip, oracle, e, K):
    ks = [4, K]
    idx, resid, cb = fc.random_case(3 * K, ks, e, seed=2000 + e + K)
    want, movers, unres = _check(hip, idx, 0, resid, cb, ks, (e, K))
    assert len(movers) > 0 and unres == 0
    d_idx = torch.from_numpy(idx).to(DEV)
    members, offsets = _tables(hip, d_idx, ks)
    fin = hip.ops.finish_nearest_free(d_idx, torch.from_numpy(resid).to(DEV), torch.from_numpy(cb).to(DEV), ks, members, offsets)
    assert fin == (len(movers), 0) and np.array_equal(d_idx.cpu().numpy(), want)
    assert colliding_items(want) == 0


def test_a_frozen_holder_beats_the_nearest_new_one(hip, oracle):
    """Frozen item 0 and new item 1 hold code 2; the new item's residual IS codebook row 2, the smallest distance there can be.
    It moves all the same.  Then {frozen, new, new} on one code: both new items move."""
    K, e = 12, 16
    idx, resid_new, cb = ec.one_bucket([2, 2], 1, K, e, seed=31)
    resid_new[0] = cb[2]
    want, movers, unres = _check(hip, idx, 1, resid_new, cb, [2, K])
    assert movers == [1] and unres == 0 and want[0, 1] == 2 and want[1, 1] != 2
    idx, resid_new, cb = ec.one_bucket([5, 5, 5], 1, K, e, seed=32)
    want, movers, unres = _check(hip, idx, 1, resid_new, cb, [2, K])
    assert movers == [1, 2] and len({5, int(want[1, 1]), int(want[2, 1])}) == 3


def test_exact_ties_among_new_holders_and_among_free_codes(hip, oracle):
    """Small integers (every product and sum exact in fp32).  {new, new, new} on one code with one residual row three times: the
    lowest id keeps.  Codebook rows 3, 7 and 9 are equal and nearest to the movers: the lower code is taken first."""
    K, e = 12, 32
    r = gi.rs(33)
    cb = gi.f32(r.randint(-2, 3, size=(K, e)))
    cb[7] = cb[3]
    cb[9] = cb[3]
    idx = np.array([[0, 0], [0, 1], [0, 5], [0, 5], [0, 5]], dtype=np.int64)       # two frozen bystanders, three new on code 5
    resid_new = gi.f32(np.stack([cb[3]] * 3))
    want, movers, unres = _check(hip, idx, 2, resid_new, cb, [2, K])
    assert movers == [3, 4] and want[2, 1] == 5 and want[3, 1] == 3 and want[4, 1] == 7


def test_buckets_that_must_not_be_touched(hip, oracle):
    K, e = 12, 16
    # two frozen items share a code; the bucket's only new item holds another code alone
    idx, resid_new, cb = ec.one_bucket([4, 4, 6], 2, K, e, seed=34)
    got, moved, unresolved = _run(hip, idx, 2, resid_new, cb, [2, K])
    assert (moved, unresolved) == (0, 0) and np.array_equal(got, idx)
    # a bucket of colliding frozen items only (it leaves before the histogram), beside a bucket with a new item and no shared code
    idx = np.array([[0, 3], [0, 3], [0, 3], [1, 2], [1, 5]], dtype=np.int64)
    got, moved, unresolved = _run(hip, idx, 4, gi.f32(gi.rs(35).standard_normal((1, e))), cb, [2, K])
    assert (moved, unresolved) == (0, 0) and np.array_equal(got, idx)
    # ... and the frozen-only bucket stays so beside one that IS touched
    idx = np.array([[0, 3], [0, 3], [0, 3], [1, 2], [1, 2], [1, 2]], dtype=np.int64)
    want, movers, unres = _check(hip, idx, 4, gi.f32(gi.rs(36).standard_normal((2, e))), cb, [2, K])
    assert movers == [4, 5] and np.array_equal(want[:3], idx[:3])


def test_movers_that_straddle_a_chunk_of_256_positions(hip, oracle):
    """250 frozen items on codes 0 .. 249 and 30 new ones that hold frozen codes, K = 320: the movers sit at positions 250 .. 279
    of their bucket, on both sides of the first chunk's end."""
    K, e = 320, 16
    r = gi.rs(37)
    codes = list(range(250)) + r.randint(0, 250, size=30).tolist()
    idx, resid_new, cb = ec.one_bucket(codes, 250, K, e, seed=38)
    want, movers, unres = _check(hip, idx, 250, resid_new, cb, [2, K])
    assert movers == list(range(250, 280)) and unres == 0 and colliding_items(want) == 0


def test_a_600_member_bucket_frozen_up_to_its_third_chunk(hip, oracle):
    K, e, n0 = 640, 16, 530
    r = gi.rs(39)
    codes = r.randint(0, 600, size=600).tolist()                                   # the frozen items collide among themselves too
    idx, resid_new, cb = ec.one_bucket(codes, n0, K, e, seed=40)
    want, movers, unres = _check(hip, idx, n0, resid_new, cb, [2, K])
    assert len(movers) > 30 and min(movers) >= n0 and unres == 0
    assert colliding_items(want) == ec.colliding_among(idx, n0)


def test_no_free_code_at_all(hip, oracle):
    """K = 7, every code held by a frozen item, two new holders: both unresolved, nothing written.  And K = 1."""
    K, e = 7, 32
    idx, resid_new, cb = ec.one_bucket(list(range(K)) + [3, 3], K, K, e, seed=41)
    want, movers, unres = _check(hip, idx, K, resid_new, cb, [2, K])
    assert movers == [K, K + 1] and unres == 2 and np.array_equal(want, idx)
    idx, resid_new, cb = ec.one_bucket([0, 0, 0], 1, 1, e, seed=42)
    want, movers, unres = _check(hip, idx, 1, resid_new, cb, [2, 1])
    assert movers == [1, 2] and unres == 2 and np.array_equal(want, idx)
    idx, resid_new, cb = ec.one_bucket([0, 0, 0], 0, 1, e, seed=43)                 # K = 1 among new items: one keeps, two stay put
    want, movers, unres = _check(hip, idx, 0, resid_new, cb, [2, 1])
    assert len(movers) == 2 and unres == 2


def test_free_codes_run_out_in_the_first_chunk(hip, oracle):
    """K = 48: 40 frozen items on codes 0 .. 39, 300 new items on those codes too.  Eight free codes: the first eight movers take
    them, the other 208 of the first chunk are counted one by one, the 84 of the second chunk in parallel."""
    K, e = 48, 16
    r = gi.rs(44)
    codes = list(range(40)) + r.randint(0, 40, size=300).tolist()
    idx, resid_new, cb = ec.one_bucket(codes, 40, K, e, seed=45)
    want, movers, unres = _check(hip, idx, 40, resid_new, cb, [2, K])
    assert movers == list(range(40, 340)) and unres == 292
    assert sorted(want[40:48, 1].tolist()) == list(range(40, 48)) and np.array_equal(want[48:], idx[48:])
    assert colliding_items(want) == unres


@pytest.mark.parametrize("ks,n,n0,e", [([100], 90, 50, 16), ([100], 150, 70, 32), ([7, 48], 200, 120, 64), ([3, 3, 48], 400, 250, 32),
                                       ([5, 100], 300, 1, 16), ([5, 100], 300, 290, 64)])
def test_one_two_and_three_levels_at_every_width(hip, oracle, ks, n, n0, e):
    """L = 1 is a single bucket of all items (150 items on 100 codes: some stay unresolved); the frozen items collide among
    themselves, as a base file may, and the count afterwards is theirs plus `unresolved`."""
    idx, resid_new, cb = ec.random_split_case(n, n0, ks, e, seed=46 + n + n0)
    want, movers, unres = _check(hip, idx, n0, resid_new, cb, ks, (ks, n, n0, e))
    assert np.array_equal(want[:, :-1], idx[:, :-1])
    assert colliding_items(want) == ec.colliding_among(idx, n0) + unres
    assert (unres > 0) == (ks == [100] and n == 150)
    assert len(movers) > 0


def test_members_out_of_range_take_no_part(hip, oracle):
    """One listed bucket whose member list carries ids below 0 and past n, and items whose last code is outside [0, K), frozen
    and new: none of them is read as a holder or written."""
    K, e, n, n0 = 12, 16, 12, 5
    codes = [2, -1, 2, K, 4, 2, K + 3, 4, 4, -9, 7, 2]
    idx, resid_new, cb = ec.one_bucket(codes, n0, K, e, seed=47)
    members = [[-5, -1] + list(range(n)) + [n, n + 3, 1 << 40]]
    want, movers, unres = _check(hip, idx, n0, resid_new, cb, [2, K], buckets=members)
    assert movers == [5, 7, 8, 11] and unres == 0
    assert np.array_equal(want[[1, 3, 6, 9]], idx[[1, 3, 6, 9]])


def test_a_mover_with_a_nan_residual(hip, oracle):
    K, e = 12, 32
    idx, resid_new, cb = ec.one_bucket([1, 1, 1, 6, 6], 1, K, e, seed=48)
    resid_new[0] = np.nan                                                          # item 1: a mover, every distance +inf: code 0
    resid_new[2, 5] = np.nan                                                       # item 3: loses code 6 to the finite item 4
    want, movers, unres = _check(hip, idx, 1, resid_new, cb, [2, K])
    assert movers == [1, 2, 3] and want[1, 1] == 0 and want[4, 1] == 6 and unres == 0


def test_hundreds_of_buckets_of_which_few_hold_a_new_item(hip, oracle):
    ks = [20, 20, 32]
    n, n0 = 5000, 4960
    idx, resid_new, cb = ec.random_split_case(n, n0, ks, 32, seed=49)
    want, movers, unres = _check(hip, idx, n0, resid_new, cb, ks)
    prefixes = {tuple(row) for row in idx[:, :2]}
    with_new = {tuple(row) for row in idx[n0:, :2]}
    assert len(prefixes) >= 390 and len(with_new) <= 40 and 0 < len(movers) <= 40
    assert colliding_items(want) == ec.colliding_among(idx, n0) + unres
    again, moved, unresolved = _run(hip, idx, n0, resid_new, cb, ks)                # two runs: identical bytes
    assert again.tobytes() == want.tobytes() and (moved, unresolved) == (len(movers) - unres, unres)


def test_refusals_and_no_new_items_launch_nothing(hip):
    n, K = 64, 48
    idx = torch.zeros((n, 2), dtype=torch.int64, device=DEV)
    members = torch.arange(n, dtype=torch.int64, device=DEV)
    offsets = torch.tensor([0, n], dtype=torch.int64, device=DEV)
    f = hip.ops.extend_nearest_free
    z = lambda *shape: torch.zeros(shape, device=DEV)

    def refused(match, *args):
        with pytest.raises(hip.LcrecError, match=match):
            ec.in_thread(f, *args)

    hip.ops.trace_enable(True)
    try:
        for e in (8, 24, 128):
            refused(f"e_dim={e}", idx, 4, z(n - 4, e), z(K, e), [4, K], members, offsets)
        refused(r"level 1 \(K=4096, e=64\) does not fit", idx, 4, z(n - 4, 64), z(4096, 64), [4, 4096], members, offsets)
        refused(r"level 1 \(K=1900, e=16\) does not fit in 160 KB of LDS with the frozen-holder counts", idx, 4, z(n - 4, 16), z(1900, 16),
                [4, 1900], members, offsets)
        flat = torch.zeros(n * 16 + 4, device=DEV)
        refused("resid_last and codebook_last must be 16-byte aligned", idx, 0, flat[1:1 + n * 16].view(n, 16), z(K, 16), [4, K],
                members, offsets)
        # what the binding itself refuses: n_frozen out of range, one row per new item, shapes, host tensors, a strided matrix
        refused("n_frozen=-1", idx, -1, z(n, 16), z(K, 16), [4, K], members, offsets)
        refused("n_frozen=65", idx, n + 1, z(0, 16), z(K, 16), [4, K], members, offsets)
        refused("one row per new item", idx, 4, z(n, 16), z(K, 16), [4, K], members, offsets)
        refused("do not go with", idx, 4, z(n - 4, 16), z(K, 32), [4, K], members, offsets)
        refused("ks", idx, 4, z(n - 4, 16), z(K, 16), [4, K + 1], members, offsets)
        refused("idx must be", idx.cpu(), 4, z(n - 4, 16), z(K, 16), [4, K], members, offsets)
        refused("idx must be", torch.zeros((n, 4), dtype=torch.int64, device=DEV)[:, :2], 4, z(n - 4, 16), z(K, 16), [4, K], members, offsets)
        # no new item (N == N0): the counters are zeroed, nothing is launched
        assert f(idx, n, z(0, 16), z(K, 16), [4, K], members, offsets) == (0, 0)
        assert f(idx, 4, z(n - 4, 16), z(K, 16), [4, K], members[:0], offsets[:1]) == (0, 0)
        torch.cuda.synchronize()
        assert hip.ops.trace_collect() == {}
        # ... and a call that does launch is traced under its own name, once
        assert f(idx, 4, z(n - 4, 16), z(K, 16), [4, K], members, offsets) == (K - 1, n - 4 - (K - 1))
        torch.cuda.synchronize()
        seen = hip.ops.trace_collect()
        assert list(seen) == ["extend_nearest_free"] and seen["extend_nearest_free"][0] == 1
    finally:
        hip.ops.trace_enable(False)
    assert int(idx[:4].abs().sum()) == 0


def test_generate_extend_places_1000_new_f6_items_around_2000_frozen_ones(hip, oracle, tmp_path):
    """The F6 checkpoint, built as test_gpu_finish builds it.  generate(finish="nearest_free") on the first 2000 rows writes the
    base; generate(extend=base) on all 3000 follows."""
    from lcrec_amd import generate_indices as gen
    idx, resid, cb, g = fc.f6_case()
    meta = json.load(open(os.path.join(fc.GOLD, "manifest.json")))["fixtures"]["f6_generate.npz"]
    n0, n = 2000, 3000
    items = gi.toy_items(meta["seed"])
    npy0, npy = str(tmp_path / "Toy2000.emb.npy"), str(tmp_path / "Toy.emb.npy")
    np.save(npy0, items[:n0])
    np.save(npy, items)
    kw = {k: v for k, v in meta["model"].items() if k != "in_dim"}
    args = argparse.Namespace(data_path=npy, num_workers=0, **kw)
    sd = {k[4:]: torch.from_numpy(g[k].copy()) for k in g.files if k.startswith("sd__")}
    ckpt = str(tmp_path / "toy.pth")
    torch.save({"args": args, "epoch": 0, "best_loss": 0.0, "best_collision_rate": 0.0, "state_dict": sd, "optimizer": {}}, ckpt,
               pickle_protocol=4)
    base_file = str(tmp_path / "Base.index.json")
    s0 = gen.generate(ckpt, base_file, device="cuda:0", data_path=npy0, verbose=False, finish="nearest_free")
    assert s0["items"] == n0 and s0["collision_rate"] == 0
    base_bytes = open(base_file, "rb").read()
    base = gen.load_index_json(base_file, [48, 48, 48])
    assert base.shape == (n0, 3)

    out = str(tmp_path / "Toy.index.json")
    hip.ops.trace_enable(True)
    try:
        stats = gen.generate(ckpt, out, device="cuda:0", verbose=False, extend=base_file, finish="nearest_free")
        torch.cuda.synchronize()
        seen = hip.ops.trace_collect()
    finally:
        hip.ops.trace_enable(False)
    assert seen["extend_nearest_free"][0] == 1 and "sinkhorn" not in " ".join(seen) and "finish_nearest_free" not in seen
    got = open(out, "rb").read()
    assert got[:len(base_bytes) - 1] == base_bytes[:-1]                             # the base's bytes, without its closing brace
    after = gen.load_index_json(out, [48, 48, 48])
    assert after.shape == (n, 3) and np.array_equal(after[:n0], base)
    pass1 = ec.f6_pass1()
    union = np.concatenate([base, pass1[n0:]])
    want, movers, unres = extend_ref(union, n0, gi.f32(resid[n0:]), cb)
    assert np.array_equal(after[n0:], want[n0:]) and unres == 0
    still = np.ones(n, dtype=bool)
    still[movers] = False
    assert np.array_equal(after[still][n0:], pass1[still][n0:])                     # not a mover: the pass-1 tuple
    assert stats["extend_unresolved"] == 0 and stats["collision_rate"] == 0 and stats["max_conflicts"] == 1
    assert stats["extend_moved"] == len(movers) > 0
    assert (stats["items"], stats["base_items"], stats["new_items"], stats["base_colliding"]) == (n, n0, n - n0, 0)
    assert stats["buckets"] > 0 and stats["largest_bucket"] == 41 and stats["neartie_items"] >= 0
    out2 = str(tmp_path / "Toy.again.index.json")
    stats2 = gen.generate(ckpt, out2, device="cuda:0", verbose=False, extend=base_file)
    assert open(out2, "rb").read() == got and stats2 == stats
    # N == N0: nothing is launched and the base is rewritten
    hip.ops.trace_enable(True)
    try:
        out3 = str(tmp_path / "Base.again.index.json")
        s3 = gen.generate(ckpt, out3, device="cuda:0", data_path=npy0, verbose=False, extend=base_file)
        torch.cuda.synchronize()
        assert hip.ops.trace_collect() == {}
    finally:
        hip.ops.trace_enable(False)
    assert open(out3, "rb").read() == base_bytes and (s3["new_items"], s3["extend_moved"], s3["collision_rate"]) == (0, 0, 0.0)
    with pytest.raises(ValueError, match="whole catalogue"):
        gen.generate(ckpt, out3, device="cuda:0", data_path=npy0, verbose=False, extend=out)
