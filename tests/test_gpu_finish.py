"""MI355X: the nearest-free-code finishing pass (lcrec_finish_nearest_free, ops.finish_nearest_free, generate(finish=...)).

Every comparison is exact: the kernel and tests/finish_ref.py evaluate the same fp32 fma chains and every tie is defined, so
`idx`, `moved` and `unresolved` must agree bit for bit -- there is no tolerance anywhere in this file."""
import argparse
import json
import os
import types

import numpy as np
import pytest
import torch

import finish_cases as fc
import golden_inputs as gi
from finish_ref import colliding_items, finish_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _tables(hip, idx_dev, ks):
    """(members, offsets) the way generate_indices.finish_collisions builds them."""
    n, L = idx_dev.shape
    if L == 1:
        return torch.arange(n, dtype=torch.int64, device=DEV), torch.tensor([0, n], dtype=torch.int64, device=DEV)
    found = hip.ops.collision_groups(idx_dev[:, :L - 1].contiguous(), ks[:-1], want_groups="device")
    return found["members"], found["offsets"]


def _run(hip, idx, resid, cb, ks):
    d_idx = torch.from_numpy(idx).to(DEV)
    members, offsets = _tables(hip, d_idx, ks)
    moved, unresolved = hip.ops.finish_nearest_free(d_idx, torch.from_numpy(resid).to(DEV), torch.from_numpy(cb).to(DEV), ks,
                                                    members, offsets)
    return d_idx.cpu().numpy(), moved, unresolved


def _check(hip, idx, resid, cb, ks, what=""):
    want, movers, want_unres = finish_ref(idx, resid, cb)
    got, moved, unresolved = _run(hip, idx, resid, cb, ks)
    print(what, "movers", len(movers), "moved", moved, "unresolved", unresolved, "(reference:", len(movers) - want_unres, want_unres, ")")
    assert (moved, unresolved) == (len(movers) - want_unres, want_unres), what
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]], idx[bad[:8]])
    assert colliding_items(got) == unresolved                       # the stated consequence of the rule
    return want, movers, want_unres


@pytest.mark.parametrize("K", [48, 100, 256, 1])
@pytest.mark.parametrize("e", [16, 32, 64])
def test_random_buckets_match_the_reference(hip, oracle, e, K):
    """Four buckets of about 0.75 K items over K codes: many shared codes, K not a multiple of the 64-lane code stride (48,
    100), more codes than threads' first trip (256 = one code per thread exactly), and K = 1 where nothing is ever free."""
    ks = [4, K]
    idx, resid, cb = fc.random_case(max(12, 3 * K), ks, e, seed=1000 + e + K)
    want, movers, unres = _check(hip, idx, resid, cb, ks, (e, K))
    assert len(movers) > 0 and (unres > 0) == (K == 1)


def test_a_bucket_of_exactly_k_items_and_one_of_k_plus_3(hip, oracle):
    K, e = 48, 16
    r = gi.rs(21)
    first = r.randint(0, K, size=K)                                 # K items on random codes: ends fully occupied
    second = r.randint(0, K, size=K + 3)                            # K + 3: three have nowhere to go
    idx = np.concatenate([np.stack([np.zeros(K, int), first], 1), np.stack([np.ones(K + 3, int), second], 1)]).astype(np.int64)
    perm = r.permutation(len(idx))                                  # the two buckets interleaved in item order
    idx = idx[perm]
    resid = gi.f32(r.standard_normal((len(idx), e)))
    cb = gi.f32(r.standard_normal((K, e)))
    want, movers, unres = _check(hip, idx, resid, cb, [2, K])
    assert unres == 3
    assert sorted(want[want[:, 0] == 0, 1].tolist()) == list(range(K))              # every code taken exactly once
    assert set(want[want[:, 0] == 1, 1].tolist()) == set(range(K))


@pytest.mark.parametrize("e", [16, 64])
def test_movers_whose_nearest_free_codes_coincide(hip, oracle, e):
    """One bucket; codes 0, 1, 2 are held by 2, 3 and 4 items.  All nine residuals lie near code 3, so each of the six movers has
    code 3 as its nearest free code at the start: they must be served one after the other, each seeing what the others took."""
    K = 12
    cb = np.zeros((K, e), dtype=np.float32)
    cb[:, 0] = [0.0, 1.0, 2.0, 10.0, 10.5, 11.0, 12.0, 13.5, 15.0, 40.0, 41.0, 42.0]
    cb[:, 1] = 0.25
    r = gi.rs(22)
    resid = np.zeros((9, e), dtype=np.float32)
    resid[:, 0] = 10.1 + 0.02 * r.standard_normal(9)
    resid[:, 2] = 0.01 * r.standard_normal(9)
    idx = np.array([[0], [1], [2], [1], [2], [2], [0], [1], [2]], dtype=np.int64)
    d = oracle.distances(resid, cb)
    assert (np.argmin(d[:, 3:], axis=1) == 0).all()                                 # everybody's nearest free code is code 3
    want, movers, unres = _check(hip, idx, resid, cb, [K], e)
    assert len(movers) == 6 and unres == 0
    assert want[movers[0], 0] == 3 and len(set(want[movers, 0].tolist())) == 6      # first served gets it, nobody else does


def test_exact_ties_from_duplicated_rows(hip, oracle):
    """Small integers (every product and sum exact in fp32): duplicated codebook rows tie exactly as free codes (lowest code
    wins), duplicated residual rows tie exactly as holders (lowest id keeps)."""
    K, e, n = 48, 32, 96
    r = gi.rs(23)
    cb = gi.f32(r.randint(-2, 3, size=(K, e)))
    cb[40] = cb[7]
    cb[41] = cb[7]
    cb[13] = cb[12]
    cb[47] = cb[0]
    rows = gi.f32(r.randint(-2, 3, size=(n // 4, e)))
    resid = gi.f32(rows[r.randint(0, n // 4, size=n)])              # every residual row occurs about four times
    resid[:6] = cb[[7, 7, 12, 12, 0, 0]]                            # exact hits on duplicated codes
    idx = np.stack([r.randint(0, 3, size=n), r.randint(0, 10, size=n)], axis=1).astype(np.int64)   # codes 0 .. 9 only: 38 free
    want, movers, unres = _check(hip, idx, resid, cb, [3, K])
    assert unres == 0 and len(movers) > 40
    d = oracle.distances(resid, cb)
    tied = sum(1 for i in movers if (d[i] == d[i, want[i, 1]]).sum() > 1)
    assert tied > 0                                                                  # the case does exercise exact ties


@pytest.mark.parametrize("ks,n", [([100], 60), ([100], 150), ([7, 48], 200), ([3, 3, 48], 400)])
def test_one_two_and_three_levels(hip, oracle, ks, n):
    """L = 1 is a single bucket of all items (150 items on 100 codes: 50 stay unresolved); L = 3 buckets on two columns."""
    idx, resid, cb = fc.random_case(n, ks, 32, seed=24 + n)
    want, movers, unres = _check(hip, idx, resid, cb, ks, (ks, n))
    if len(ks) == 1:
        assert unres == max(0, n - ks[-1])
    assert np.array_equal(want[:, :-1], idx[:, :-1])


def test_free_codes_run_out_in_a_later_chunk(hip, oracle):
    """One bucket of 600 items on codes 0 .. 39 of 320: 280 free codes for about 560 movers.  The walk takes 256 positions at a
    time, so the last free code goes in the second or third chunk, the movers behind it in that chunk are counted one by one, and
    at least one whole chunk starts with none left and is counted in parallel."""
    K, e, n = 320, 16, 600
    r = gi.rs(29)
    idx = r.randint(0, 40, size=(n, 1)).astype(np.int64)
    resid = gi.f32(r.standard_normal((n, e)))
    cb = gi.f32(r.standard_normal((K, e)))
    want, movers, unres = _check(hip, idx, resid, cb, [K])
    assert unres > 0 and len(movers) - unres == 280                                  # the case does run out of free codes


def test_300_touched_buckets_among_5000_items(hip, oracle):
    """400 prefixes, about 12 items each on 32 codes: more workgroups than the device has CUs, most of them touched, some not."""
    ks = [20, 20, 32]
    idx, resid, cb = fc.random_case(5000, ks, 32, seed=25)
    want, movers, unres = _check(hip, idx, resid, cb, ks)
    touched = {tuple(idx[i, :2]) for i in movers}
    prefixes = {tuple(row) for row in idx[:, :2]}
    assert len(touched) >= 300 and len(prefixes) > len(touched) and len(prefixes) > torch.cuda.get_device_properties(0).multi_processor_count
    still = np.ones(len(idx), dtype=bool)
    still[movers] = False
    got, _, _ = _run(hip, idx, resid, cb, ks)
    assert np.array_equal(got[still], idx[still]) and still.sum() > 3000             # untouched items stay bit for bit


def test_no_buckets_and_no_shared_codes(hip, oracle):
    K, e = 48, 16
    idx, resid, cb = fc.random_case(40, [5, K], e, seed=26)
    d_idx = torch.from_numpy(idx).to(DEV)
    empty = torch.zeros(0, dtype=torch.int64, device=DEV)
    zero = torch.zeros(1, dtype=torch.int64, device=DEV)
    assert hip.ops.finish_nearest_free(d_idx, torch.from_numpy(resid).to(DEV), torch.from_numpy(cb).to(DEV), [5, K], empty, zero) == (0, 0)
    assert hip.ops.finish_nearest_free(d_idx, torch.from_numpy(resid).to(DEV), torch.from_numpy(cb).to(DEV), [5, K], empty, empty) == (0, 0)
    assert np.array_equal(d_idx.cpu().numpy(), idx)
    # buckets listed, none of them with a shared code: nothing moves
    idx2 = np.stack([np.arange(40) % 2, np.arange(40) // 2], axis=1).astype(np.int64)
    got, moved, unresolved = _run(hip, idx2, resid, cb, [5, K])
    assert (moved, unresolved) == (0, 0) and np.array_equal(got, idx2)


def test_members_are_gathered_by_id_not_by_position(hip, oracle):
    """One listed bucket whose ids are far apart among 5000 items; the rows at positions 0 .. m-1 belong to other items."""
    K, e, n = 48, 32, 5000
    r = gi.rs(27)
    ids = np.sort(r.choice(n, size=30, replace=False))
    ids[0], ids[-1] = 3, n - 1
    ids = np.unique(ids)
    idx = np.stack([np.ones(n, int), r.randint(0, K, size=n)], axis=1).astype(np.int64)
    idx[ids, 0] = 0
    idx[ids, 1] = r.randint(0, 8, size=len(ids))
    resid = gi.f32(r.standard_normal((n, e)))
    cb = gi.f32(r.standard_normal((K, e)))
    sub, movers, unres = finish_ref(idx[ids], resid[ids], cb)
    want = idx.copy()
    want[ids] = sub
    d_idx = torch.from_numpy(idx).to(DEV)
    members = torch.from_numpy(ids.astype(np.int64)).to(DEV)
    offsets = torch.tensor([0, len(ids)], dtype=torch.int64, device=DEV)
    got = hip.ops.finish_nearest_free(d_idx, torch.from_numpy(resid).to(DEV), torch.from_numpy(cb).to(DEV), [2, K], members, offsets)
    assert got == (len(movers), 0) and len(movers) >= 10
    assert np.array_equal(d_idx.cpu().numpy(), want)


def test_finish_collisions_builds_the_single_bucket_itself(hip, oracle):
    from lcrec_amd import generate_indices as gen
    K, e = 100, 16
    idx, resid, cb = fc.random_case(90, [K], e, seed=28)
    want, movers, unres = finish_ref(idx, resid, cb)
    weight = torch.from_numpy(cb).to(DEV)
    model = types.SimpleNamespace(rq=types.SimpleNamespace(vq_layers=[types.SimpleNamespace(embedding=types.SimpleNamespace(weight=weight))]))
    d_idx = torch.from_numpy(idx).to(DEV)
    out = gen.finish_collisions(model, d_idx, torch.from_numpy(resid).to(DEV), [K])
    assert out == {"moved": len(movers), "unresolved": 0, "buckets": 1, "largest_bucket": 90}
    assert np.array_equal(d_idx.cpu().numpy(), want)


def test_generate_with_finish_separates_every_f6_item(hip, oracle, tmp_path):
    """The F6 checkpoint, built as test_gpu_e2e builds it: the rounds are the reference's, then the pass moves exactly the items
    the numpy rule moves on the reference's own final tuples, and the file differs from the fixture's in their last tokens only."""
    from lcrec_amd import generate_indices as gen
    idx, resid, cb, g = fc.f6_case()
    want, movers, unres = finish_ref(idx, resid, cb)
    meta = json.load(open(os.path.join(fc.GOLD, "manifest.json")))["fixtures"]["f6_generate.npz"]
    npy = str(tmp_path / "Toy.emb.npy")
    np.save(npy, gi.toy_items(meta["seed"]))
    kw = {k: v for k, v in meta["model"].items() if k != "in_dim"}
    args = argparse.Namespace(data_path=npy, num_workers=0, **kw)
    sd = {k[4:]: torch.from_numpy(g[k].copy()) for k in g.files if k.startswith("sd__")}
    ckpt = str(tmp_path / "toy.pth")
    torch.save({"args": args, "epoch": 0, "best_loss": 0.0, "best_collision_rate": 0.0, "state_dict": sd, "optimizer": {}}, ckpt,
               pickle_protocol=4)
    out = str(tmp_path / "Toy.index.json")
    stats = gen.generate(ckpt, out, device="cuda:0", verbose=False, finish="nearest_free")
    assert stats["groups_per_round"] == g["groups_per_round"].tolist()
    assert stats["finish"] == "nearest_free" and stats["finish_moved"] == len(movers) == fc.movers_by_count(idx)
    assert stats["finish_unresolved"] == 0 and stats["collision_rate"] == 0 and stats["max_conflicts"] == 1
    got = open(out, "rb").read()
    before, after = json.loads(bytes(g["json_text"]).decode()), json.loads(got.decode())
    assert list(after) == list(before)
    differing = [int(k) for k in before if before[k] != after[k]]
    assert differing == sorted(movers)
    for i in differing:
        assert after[str(i)][:-1] == before[str(i)][:-1] and after[str(i)][-1] == "<c_%d>" % want[i, -1]
    assert got == json.dumps({str(i): t for i, t in enumerate(gen.tokens_for(want.tolist()))}).encode()
    out2 = str(tmp_path / "Toy.again.index.json")
    stats2 = gen.generate(ckpt, out2, device="cuda:0", verbose=False, finish="nearest_free")
    assert open(out2, "rb").read() == got and stats2 == stats
    with pytest.raises(ValueError, match="finish"):
        gen.generate(ckpt, out2, device="cuda:0", verbose=False, finish="suffix")


def test_refusals_name_the_dimension_and_launch_nothing(hip):
    n, K = 64, 48
    idx = torch.zeros((n, 2), dtype=torch.int64, device=DEV)
    members = torch.arange(n, dtype=torch.int64, device=DEV)
    offsets = torch.tensor([0, n], dtype=torch.int64, device=DEV)
    f = hip.ops.finish_nearest_free
    hip.ops.trace_enable(True)
    try:
        for e in (8, 24, 128):
            with pytest.raises(hip.LcrecError, match=f"e_dim={e}"):
                f(idx, torch.zeros((n, e), device=DEV), torch.zeros((K, e), device=DEV), [4, K], members, offsets)
        with pytest.raises(hip.LcrecError, match=r"level 1 \(K=4096, e=64\) does not fit"):
            f(idx, torch.zeros((n, 64), device=DEV), torch.zeros((4096, 64), device=DEV), [4, 4096], members, offsets)
        flat = torch.zeros(n * 16 + 4, device=DEV)
        with pytest.raises(hip.LcrecError, match="resid_last and codebook_last must be 16-byte aligned"):
            f(idx, flat[1:1 + n * 16].view(n, 16), torch.zeros((K, 16), device=DEV), [4, K], members, offsets)
        with pytest.raises(hip.LcrecError, match="resid_last and codebook_last must be 16-byte aligned"):
            f(idx, torch.zeros((n, 16), device=DEV), flat[2:2 + K * 16].view(K, 16), [4, K], members, offsets)
        # what the binding itself refuses: shapes that do not go together, host tensors, a strided index matrix
        with pytest.raises(hip.LcrecError):
            f(idx, torch.zeros((n, 16), device=DEV), torch.zeros((K, 32), device=DEV), [4, K], members, offsets)
        with pytest.raises(hip.LcrecError):
            f(idx, torch.zeros((n, 16), device=DEV), torch.zeros((K, 16), device=DEV), [4, K + 1], members, offsets)
        with pytest.raises(hip.LcrecError):
            f(idx.cpu(), torch.zeros((n, 16), device=DEV), torch.zeros((K, 16), device=DEV), [4, K], members, offsets)
        with pytest.raises(hip.LcrecError):
            f(torch.zeros((n, 4), dtype=torch.int64, device=DEV)[:, :2], torch.zeros((n, 16), device=DEV),
              torch.zeros((K, 16), device=DEV), [4, K], members, offsets)
        torch.cuda.synchronize()
        assert hip.ops.trace_collect() == {}
    finally:
        hip.ops.trace_enable(False)
    assert int(idx.abs().sum()) == 0
