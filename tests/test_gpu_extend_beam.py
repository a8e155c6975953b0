"""MI355X: the frozen-aware beam finishing pass (lcrec_extend_finish_beam, ops.extend_finish_beam,
generate_indices.extend_beam_collisions, generate(extend=..., extend_finish="beam")).

As tests/test_gpu_beam_finish.py: the pass compares tuples and the errors it is given and computes nothing, so every comparison with
tests/extend_beam_ref.py is integer-exact: idx, choice_out and counters_out.  idx and choice_out sit between guard bands, choice_out
is pre-filled with garbage, the counters with a non-zero pattern, the workspace has exactly the queried size and is filled with 0xFF;
every call is made a second time on the then dirty workspace -- and that second call runs on the POISONED row, whose frozen members'
positions hold what would change the result if it were read."""
import argparse
import json
import os
import types

import numpy as np
import pytest
import torch

import beam_finish_cases as bfc
import extend_beam_cases as xbc
import extend_cases as ec
import finish_cases as fc
import golden_inputs as gi
from audit_ref import audit_ref
from beam_finish_ref import colliding_items

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAND = 256                                                  # bytes on either side of idx, choice_out and the workspace
BAND_BYTE = 0x5A
GARBAGE = 0x7FC12345
INPUTS = ("members", "offsets", "err_held", "cand", "cand_err")


class Banded:
    """`shape` elements of `dtype` as a view into a larger byte buffer: BAND bytes of BAND_BYTE, the elements, BAND bytes more."""

    def __init__(self, dtype, shape):
        self.nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full((BAND + self.nbytes + BAND,), BAND_BYTE, dtype=torch.uint8, device=DEV)
        self.bytes = self.raw[BAND:BAND + self.nbytes]
        self.view = self.bytes.view(dtype).view(shape)

    def bands_intact(self):
        return bool((self.raw[:BAND] == BAND_BYTE).all()) and bool((self.raw[BAND + self.nbytes:] == BAND_BYTE).all())


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)             # (a copy: the shared inputs are read-only arrays)


class Call:
    """One case's device buffers, allocated once, and the call in the form that reads nothing back.  frozen=False: ops.finish_beam
    on the same buffers."""

    def __init__(self, hip, c, frozen=True):
        self.hip, self.frozen = hip, frozen
        n, L = c["idx"].shape
        M, W = c["cand_err"].shape
        self.ks, self.n_frozen = list(c["ks"]), c.get("n_frozen", 0)
        self.idx = Banded(torch.int64, (n, L))
        self.choice = Banded(torch.int32, (M,))
        self.counters = torch.empty(4, dtype=torch.int64, device=DEV)
        self.inputs = {k: torch.empty(c[k].shape, dtype=torch.from_numpy(np.array(c[k])).dtype, device=DEV) for k in INPUTS}
        lib = hip._lib.load()
        need = (lib.lcrec_extend_finish_beam_workspace if frozen else lib.lcrec_finish_beam_workspace)(n, M, L, W)
        assert need > 0 and need == lib.lcrec_finish_beam_workspace(n, M, L, W)
        self.workspace = Banded(torch.uint8, (need,))

    def load(self, c, poison=True):
        self.idx.view.copy_(dev(c["idx"]))
        for k, t in self.inputs.items():
            t.copy_(dev(c[k]))
        self.choice.bytes.view(torch.int32).fill_(GARBAGE)
        self.counters.fill_(0x0123456789ABCDEF)
        if poison:
            self.workspace.bytes.fill_(0xFF)

    def __call__(self):
        i = self.inputs
        tail = (self.ks, i["members"], i["offsets"], i["err_held"], i["cand"], i["cand_err"])
        kw = dict(counters_out=self.counters, choice_out=self.choice.view, workspace=self.workspace.view)
        if self.frozen:
            choice, counters = self.hip.ops.extend_finish_beam(self.idx.view, self.n_frozen, *tail, **kw)
        else:
            choice, counters = self.hip.ops.finish_beam(self.idx.view, *tail, **kw)
        assert counters is None                                                       # nothing was read back

    def result(self, sync=torch.cuda.synchronize):
        sync()
        for name in ("idx", "choice", "workspace"):
            assert getattr(self, name).bands_intact(), f"{name}: written outside its buffer"
        return self.idx.view.cpu().numpy(), self.choice.view.cpu().numpy(), tuple(self.counters.tolist())


def check(got, want, what, no_launch=False):
    idx, choice, counters = got
    w_idx, w_choice, w_counters = want
    print(what, "counters", counters)
    assert counters == tuple(w_counters), (what, counters, w_counters)
    if no_launch:                                                                     # choice_out is not touched
        assert (choice.view(np.int32) == GARBAGE).all() or choice.size == 0
    else:
        bad = np.flatnonzero(choice != w_choice)
        assert bad.size == 0, (what, "choice", bad[:8], choice[bad[:8]], w_choice[bad[:8]])
    bad = np.flatnonzero((idx != w_idx).any(1))
    assert bad.size == 0, (what, "idx", bad[:8], idx[bad[:4]], w_idx[bad[:4]])


@pytest.mark.parametrize("row", xbc.rows())
def test_every_row_matches_the_rule_exactly(hip, oracle, row):
    c, want = xbc.case(row), xbc.reference(row)
    n, M, nf = len(c["idx"]), len(c["members"]), c["n_frozen"]
    if M == 0:                                                                        # no group: no launch, the counters are zeroed
        counters = torch.full((4,), 7, dtype=torch.int64, device=DEV)
        idx = dev(c["idx"])
        choice, none = hip.ops.extend_finish_beam(idx, nf, list(c["ks"]), torch.zeros(0, dtype=torch.int64, device=DEV), dev(c["offsets"]),
                                                  dev(c["err_held"]), dev(c["cand"]), dev(c["cand_err"]), counters_out=counters)
        torch.cuda.synchronize()
        assert none is None and choice.numel() == 0 and counters.tolist() == [0, 0, 0, 0]
        assert np.array_equal(idx.cpu().numpy(), c["idx"])
        return
    call = Call(hip, c)
    call.load(c)
    hip.ops.trace_enable(True)
    try:
        call()
        torch.cuda.synchronize()
        traced = hip.ops.trace_collect()
    finally:
        hip.ops.trace_enable(False)
    if nf == n:                                                                       # no new item: no launch either
        assert traced == {}
        check(call.result(), (c["idx"], None, (0, 0, 0, 0)), (row, "n_frozen == n"), no_launch=True)
        return
    assert set(traced) == {"extend_finish_beam"} and traced["extend_finish_beam"][0] == 1   # one bracket per call
    first = call.result()
    check(first, want, (row, "first call"))
    assert np.array_equal(first[0][:nf], c["idx"][:nf])
    call.load(xbc.poisoned(row), poison=False)                                        # again: a dirty workspace, poisoned frozen positions
    call()
    second = call.result()
    check(second, want, (row, "second call, dirty workspace, poisoned frozen positions"))
    if xbc.true_groups(row):
        assert colliding_items(second[0], c["ks"]) == colliding_items(c["idx"][:nf], c["ks"]) + want[2][2]


@pytest.mark.parametrize("row", ["q-48_100_7-W8", "s-wide-both", "s-nan", "s-foreign", "s-sync", "s-w1", "s-large"])
def test_without_frozen_items_it_is_finish_beam(hip, oracle, row):
    """n_frozen = 0: idx, choice_out and the counters are ops.finish_beam's on the same inputs (and the rule's)"""
    c = bfc.case(row)
    got = []
    for frozen in (True, False):
        call = Call(hip, c, frozen=frozen)
        call.load(c)
        call()
        got.append(call.result())
    check(got[0], got[1], (row, "extend_finish_beam(n_frozen=0) against finish_beam"))
    check(got[0], bfc.reference(row), (row, "against the rule"))


def test_a_group_table_without_groups_launches_nothing_and_leaves_choice_alone(hip, oracle):
    c = dict(xbc.case("s-dead-f1"))
    c["offsets"] = c["offsets"][:1]
    call = Call(hip, c)
    call.load(c)
    call()
    check(call.result(), (c["idx"], None, (0, 0, 0, 0)), "no group", no_launch=True)


def test_the_call_is_recorded_once_and_replayed_on_other_inputs(hip, oracle):
    """As tests/test_gpu_beam_finish.py does it: one stream, one chain, every buffer allocated before the capture, the second input set
    sharing every host-side argument, n_frozen included."""
    a, b = xbc.capture_pair()
    want_a, want_b = xbc.run_rule(a), xbc.run_rule(b)
    call = Call(hip, a)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(side):
            call.load(a)
            call()
            check(call.result(side.synchronize), want_a, "eager call on A, on a side stream")
            call.load(a)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                call()
            idx, choice, counters = call.result(side.synchronize)
            assert np.array_equal(idx, a["idx"]) and (choice == GARBAGE).all(), "the capture itself ran something"
            call.load(b)
            graph.replay()
            check(call.result(side.synchronize), want_b, "first replay, on B")
            call.load(a)
            graph.replay()
            check(call.result(side.synchronize), want_a, "second replay, on A")
            call.load(b, poison=False)
            graph.replay()
            check(call.result(side.synchronize), want_b, "third replay, on B, dirty workspace")
    finally:
        torch.cuda.synchronize()                                                      # a failed step leaves nothing in flight


def test_the_binding_refuses_what_does_not_go_together(hip, oracle):
    c = xbc.case("h-sync-f0")
    t = {k: dev(c[k]) for k in ("idx",) + INPUTS}
    f = hip.ops.extend_finish_beam
    args = lambda nf=1, **kw: [{**t, **kw}["idx"], nf, list(c["ks"])] + [{**t, **kw}[k] for k in INPUTS]
    for kw, text in (({"nf": -1}, "n_frozen=-1"), ({"nf": 7}, "n_frozen=7"),
                     ({"cand": t["cand"][:, :3].contiguous(), "cand_err": t["cand_err"][:, :3].contiguous()}, "width=3"),
                     ({"cand": t["cand"][:3].contiguous()}, "cand must be"), ({"err_held": t["err_held"][:3]}, "one error per member")):
        with pytest.raises(hip.LcrecError, match=text):
            ec.in_thread(f, *args(**kw))
    with pytest.raises(hip.LcrecError, match="counters_out must be"):
        f(*args(), counters_out=torch.zeros(2, dtype=torch.int64, device=DEV))
    need = hip._lib.load().lcrec_extend_finish_beam_workspace(6, 4, 2, 4)
    with pytest.raises(hip.LcrecError, match=f"workspace of {need - 1} bytes, {need} needed \\(lcrec_extend_finish_beam_workspace\\)"):
        f(*args(), workspace=torch.zeros(need - 1, dtype=torch.uint8, device=DEV))
    assert np.array_equal(t["idx"].cpu().numpy(), c["idx"])
    choice, counters = f(*args())                                                     # and the plain form returns the counts
    assert choice.tolist() == bfc.SYNC_WANT["choice"] and list(counters.values()) == bfc.SYNC_WANT["counters"]
    assert list(counters) == ["movers", "moved", "unresolved", "rounds"]
    assert [tuple(r) for r in t["idx"].tolist()] == bfc.SYNC_WANT["idx"]


# ---- end to end on the F6 split: 2 000 frozen items, 1 000 new ones ----------------------------------------------------------------
N0 = 2000


def _model(cbs):
    """what extend_beam_collisions reads of a model: the codebooks"""
    levels = [types.SimpleNamespace(embedding=types.SimpleNamespace(weight=dev(cb))) for cb in cbs]
    return types.SimpleNamespace(rq=types.SimpleNamespace(vq_layers=levels))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("base", ["finished", "reference"])
def test_extend_beam_collisions_is_the_numpy_pipeline_on_f6(hip, oracle, base):
    """beam_ref -> audit_ref -> the rule on the new members only, tuple for tuple; the rows of resid_new and resid_prev it rewrote
    are audit_ref's residuals of the new prefixes, bit for bit, and no other row changed; the frozen rows are the base's."""
    from lcrec_amd import generate_indices as gen
    z, cbs, _, _ = bfc.f6_model()
    L = len(cbs)
    flow = xbc.f6_flow(N0, base, 8)
    c, want_idx, want_choice = flow["case"], flow["idx_beam"], flow["choice"]
    union, z_new = flow["union"], np.ascontiguousarray(z[N0:])
    r_last0 = bfc.prefix_resid(z_new, cbs, np.ascontiguousarray(union[N0:]), L - 1)
    r_prev0 = bfc.prefix_resid(z_new, cbs, np.ascontiguousarray(union[N0:]), L - 2)
    idx, r_last, r_prev = dev(union), dev(r_last0), dev(r_prev0)
    hip.ops.trace_enable(True)
    try:
        done = gen.extend_beam_collisions(_model(cbs), idx, N0, [dev(z_new[:300]), dev(z_new[300:])], r_last, list(c["ks"]), 8, resid_prev=r_prev)
        torch.cuda.synchronize()
        traced = hip.ops.trace_collect()
    finally:
        hip.ops.trace_enable(False)
    print(base, done, "want", flow["counters"])
    assert traced["extend_finish_beam"][0] == 1 and "finish_beam" not in traced
    assert [done[k] for k in ("movers", "moved", "unresolved", "rounds")] == list(flow["counters"])
    got = idx.cpu().numpy()
    assert np.array_equal(got, want_idx) and np.array_equal(got[:N0], union[:N0])
    moved = c["members"][want_choice >= 0]
    assert (moved >= N0).all()
    want_sum = float(c["cand_err"][want_choice >= 0, want_choice[want_choice >= 0]].astype(np.float64).sum())
    assert done["err_moved_sum"] == pytest.approx(want_sum, rel=1e-12)              # (fp64 sums of the same fp32 values, in any order)
    want_last, want_prev = np.array(r_last0), np.array(r_prev0)
    want_last[moved - N0] = bfc.prefix_resid(z[moved], cbs, want_idx[moved], L - 1)
    want_prev[moved - N0] = bfc.prefix_resid(z[moved], cbs, want_idx[moved], L - 2)
    assert np.array_equal(_bits(r_last.cpu().numpy()), _bits(want_last)) and np.array_equal(_bits(r_prev.cpu().numpy()), _bits(want_prev))
    assert np.array_equal(_bits(want_last), _bits(flow["resid_new"]))
    assert (want_idx[moved, :L - 1] != union[moved, :L - 1]).any()                    # a move no last-code pass can make


def test_generate_extend_with_the_beam_step_on_f6(hip, oracle, tmp_path):
    from lcrec_amd import generate_indices as gen
    z, cbs, _, _ = bfc.f6_model()
    flow = xbc.f6_flow(N0, "finished", 8)
    ks = list(flow["case"]["ks"])
    g = fc.f6_case()[3]
    meta = json.load(open(os.path.join(fc.GOLD, "manifest.json")))["fixtures"]["f6_generate.npz"]
    npy = str(tmp_path / "Toy.emb.npy")
    np.save(npy, gi.toy_items(meta["seed"]))
    kw = {k: v for k, v in meta["model"].items() if k != "in_dim"}
    sd = {k[4:]: torch.from_numpy(g[k].copy()) for k in g.files if k.startswith("sd__")}
    ckpt = str(tmp_path / "toy.pth")
    torch.save({"args": argparse.Namespace(data_path=npy, num_workers=0, **kw), "epoch": 0, "best_loss": 0.0, "best_collision_rate": 0.0,
                "state_dict": sd, "optimizer": {}}, ckpt, pickle_protocol=4)
    base_file = str(tmp_path / "Base.index.json")
    gen.dump_index_json(flow["union"][:N0], base_file)
    base_bytes = open(base_file, "rb").read()

    out = str(tmp_path / "Toy.index.json")
    stats = gen.generate(ckpt, out, device=DEV, verbose=False, extend=base_file, extend_finish="beam")
    print({k: v for k, v in stats.items() if k != "audit"})
    got = open(out, "rb").read()
    assert got[:len(base_bytes) - 1] == base_bytes[:-1]                             # the base's bytes, without its closing brace
    held = gen.load_index_json(out, ks)
    assert np.array_equal(held, flow["idx_final"]) and np.array_equal(held[:N0], flow["union"][:N0])
    movers, moved, unresolved, rounds = flow["counters"]
    assert (stats["extend_beam_width"], stats["extend_beam_movers"], stats["extend_beam_moved"], stats["extend_beam_unresolved"],
            stats["extend_beam_rounds"]) == (8, movers, moved, unresolved, rounds)
    assert (stats["extend_moved"], stats["extend_unresolved"]) == flow["extend"]
    assert stats["collision_rate"] == 0.0 and stats["max_conflicts"] == 1 and "audit" not in stats and "spill_moved" not in stats
    # spill and audit behind it: nothing is left to spill, and the audit covers the new rows
    out2 = str(tmp_path / "Toy.spill.index.json")
    s2 = gen.generate(ckpt, out2, device=DEV, verbose=False, extend=base_file, extend_finish="beam", spill=True, audit=True)
    assert open(out2, "rb").read() == got and (s2["spill_moved"], s2["spill_unresolved"]) == (0, 0)
    err = audit_ref(np.ascontiguousarray(z[N0:]), cbs, np.ascontiguousarray(held[N0:]))["err"].astype(np.float64)
    assert s2["audit"]["items"] == 3000 - N0 and s2["audit"]["err_file_mean"] == pytest.approx(err.mean(), rel=1e-12)
    assert {k: v for k, v in s2.items() if k in stats} == stats
    # a narrower beam leaves more to the nearest-free pass
    s4 = gen.generate(ckpt, str(tmp_path / "W2.index.json"), device=DEV, verbose=False, extend=base_file, extend_finish="beam", finish_width=2)
    assert s4["extend_beam_width"] == 2 and s4["extend_beam_movers"] == movers and s4["extend_beam_moved"] < moved
    assert s4["extend_beam_unresolved"] == s4["extend_moved"] + s4["extend_unresolved"] and s4["collision_rate"] == 0.0
    # without the flag: today's --extend, bytes and statistics
    out3 = str(tmp_path / "Plain.index.json")
    plain = gen.generate(ckpt, out3, device=DEV, verbose=False, extend=base_file)
    assert not [k for k in plain if k.startswith("extend_beam")]
    assert np.array_equal(gen.load_index_json(out3, ks), flow["alone"]) and (plain["extend_moved"], plain["extend_unresolved"]) == flow["alone_extend"]
    expect = str(tmp_path / "Expect.index.json")
    gen.dump_index_json(flow["alone"], expect)
    assert open(out3, "rb").read() == open(expect, "rb").read()
    assert plain == gen.generate(ckpt, str(tmp_path / "Plain2.index.json"), device=DEV, verbose=False, extend=base_file, extend_finish="nearest_free")
