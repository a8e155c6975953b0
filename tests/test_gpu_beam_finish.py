"""MI355X: the beam finishing pass (lcrec_finish_beam, ops.finish_beam, generate_indices.beam_finish_collisions, generate(finish="beam")).

The pass compares tuples and the errors it is given and computes nothing, so every comparison with tests/beam_finish_ref.py is
integer-exact: idx, choice_out and counters_out.  idx and choice_out sit between guard bands, choice_out is pre-filled with garbage,
the counters with a non-zero pattern, the workspace has exactly the queried size and is filled with 0xFF; every call is made a
second time on the then dirty workspace.  The residual rows beam_finish_collisions rewrites are compared bit for bit with
tests/audit_ref.py's residual of the tuple's prefix: the same fp32 operations in the same order."""
import argparse
import json
import os
import types

import numpy as np
import pytest
import torch

import beam_finish_cases as bfc
import finish_cases as fc
import golden_inputs as gi
from audit_ref import audit_ref
from beam_finish_ref import colliding_items, finish_beam_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAND = 256                                                  # bytes on either side of idx, choice_out and the workspace
BAND_BYTE = 0x5A
GARBAGE = 0x7FC12345


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
    """One case's device buffers, allocated once, and the call in the form that reads nothing back."""

    def __init__(self, hip, c):
        self.hip, self.c = hip, c
        n, L = c["idx"].shape
        M, W = c["cand_err"].shape
        self.ks = list(c["ks"])
        self.idx = Banded(torch.int64, (n, L))
        self.choice = Banded(torch.int32, (M,))
        self.counters = torch.empty(4, dtype=torch.int64, device=DEV)
        self.inputs = {k: torch.empty(c[k].shape, dtype=torch.from_numpy(np.array(c[k])).dtype, device=DEV)
                       for k in ("members", "offsets", "err_held", "cand", "cand_err")}
        need = hip._lib.load().lcrec_finish_beam_workspace(n, M, L, W)
        assert need > 0
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
        choice, counters = self.hip.ops.finish_beam(self.idx.view, self.ks, i["members"], i["offsets"], i["err_held"], i["cand"],
                                                    i["cand_err"], counters_out=self.counters, choice_out=self.choice.view,
                                                    workspace=self.workspace.view)
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
    if no_launch:                                                                     # no group: choice_out is not touched
        assert (choice.view(np.int32) == GARBAGE).all() or choice.size == 0
    else:
        bad = np.flatnonzero(choice != w_choice)
        assert bad.size == 0, (what, "choice", bad[:8], choice[bad[:8]], w_choice[bad[:8]])
    bad = np.flatnonzero((idx != w_idx).any(1))
    assert bad.size == 0, (what, "idx", bad[:8], idx[bad[:4]], w_idx[bad[:4]])


@pytest.mark.parametrize("row", bfc.rows())
def test_every_row_matches_the_rule_exactly(hip, oracle, row):
    c, want = bfc.case(row), bfc.reference(row)
    M = len(c["members"])
    if M == 0:                                                                        # no group: no launch, the counters are zeroed
        counters = torch.full((4,), 7, dtype=torch.int64, device=DEV)
        idx = dev(c["idx"])
        empty = torch.zeros(0, dtype=torch.int64, device=DEV)
        hip.ops.trace_enable(True)
        try:
            choice, none = hip.ops.finish_beam(idx, list(c["ks"]), empty, dev(c["offsets"]), dev(c["err_held"]), dev(c["cand"]),
                                               dev(c["cand_err"]), counters_out=counters)
            torch.cuda.synchronize()
            assert hip.ops.trace_collect() == {}
        finally:
            hip.ops.trace_enable(False)
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
    assert set(traced) == {"finish_beam"} and traced["finish_beam"][0] == 1           # one bracket per call
    first = call.result()
    check(first, want, (row, "first call"))
    call.load(c, poison=False)                                                        # again, on the workspace as the first call left it
    call()
    second = call.result()
    check(second, want, (row, "second call, dirty workspace"))
    if bfc.true_groups(row):
        assert colliding_items(second[0], c["ks"]) == want[2][2]


def test_a_group_table_without_groups_launches_nothing_and_leaves_choice_alone(hip, oracle):
    """members are listed but n_tuple_groups is 0 (an offsets table of one entry): the counters are zeroed, choice_out keeps its bytes"""
    c = dict(bfc.case("s-dead"))
    c["offsets"] = c["offsets"][:1]
    call = Call(hip, c)
    call.load(c)
    call()
    check(call.result(), (c["idx"], None, (0, 0, 0, 0)), "no group", no_launch=True)


def test_the_call_is_recorded_once_and_replayed_on_other_inputs(hip, oracle):
    """As tests/test_gpu_capture_forms.py does it for the other index-side entries: one stream, one chain, every buffer allocated
    before the capture, the second input set sharing every host-side argument."""
    a, b = bfc.capture_pair()
    ref = lambda c: finish_beam_ref(c["idx"], c["ks"], c["members"], c["offsets"], c["err_held"], c["cand"], c["cand_err"])
    want_a, want_b = ref(a), ref(b)
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
            first_b = call.result(side.synchronize)
            check(first_b, want_b, "first replay, on B")
            call.load(a)
            graph.replay()
            check(call.result(side.synchronize), want_a, "second replay, on A")
            call.load(a)
            call.load(b, poison=False)
            graph.replay()
            third = call.result(side.synchronize)
            check(third, want_b, "third replay, on B")
    finally:
        torch.cuda.synchronize()                                                      # a failed step leaves nothing in flight


def test_the_binding_refuses_what_does_not_go_together(hip, oracle):
    c = bfc.case("s-sync")
    t = {k: dev(c[k]) for k in ("idx", "members", "offsets", "err_held", "cand", "cand_err")}
    args = lambda **kw: [{**t, **kw}[k] if k != "ks" else list(c["ks"]) for k in ("idx", "ks", "members", "offsets", "err_held", "cand", "cand_err")]
    for kw, text in (({"cand": t["cand"][:, :3].contiguous(), "cand_err": t["cand_err"][:, :3].contiguous()}, "width=3"),
                     ({"cand": t["cand"][:3].contiguous()}, "cand must be"), ({"err_held": t["err_held"][:3]}, "one error per member"),
                     ({"cand_err": t["cand_err"][:, :2].contiguous()}, "one error per member")):
        with pytest.raises(hip.LcrecError, match=text):
            hip.ops.finish_beam(*args(**kw))
    with pytest.raises(hip.LcrecError, match="counters_out must be"):
        hip.ops.finish_beam(*args(), counters_out=torch.zeros(2, dtype=torch.int64, device=DEV))
    with pytest.raises(hip.LcrecError, match="choice_out must be"):
        hip.ops.finish_beam(*args(), choice_out=torch.zeros(3, dtype=torch.int32, device=DEV))
    need = hip._lib.load().lcrec_finish_beam_workspace(6, 4, 2, 4)
    with pytest.raises(hip.LcrecError, match=f"workspace of {need - 1} bytes, {need} needed"):
        hip.ops.finish_beam(*args(), workspace=torch.zeros(need - 1, dtype=torch.uint8, device=DEV))
    assert np.array_equal(t["idx"].cpu().numpy(), c["idx"])
    choice, counters = hip.ops.finish_beam(*args())                                   # and the plain form returns the counts
    assert choice.tolist() == bfc.SYNC_WANT["choice"] and list(counters.values()) == bfc.SYNC_WANT["counters"]
    assert list(counters) == ["movers", "moved", "unresolved", "rounds"]
    assert [tuple(r) for r in t["idx"].tolist()] == bfc.SYNC_WANT["idx"]


# ---- end to end on F6 ------------------------------------------------------------------------------------------------------------
def _model(cbs):
    """what beam_finish_collisions reads of a model: the codebooks"""
    levels = [types.SimpleNamespace(embedding=types.SimpleNamespace(weight=dev(cb))) for cb in cbs]
    return types.SimpleNamespace(rq=types.SimpleNamespace(vq_layers=levels))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("start", ["greedy", "held"])
def test_beam_finish_collisions_is_the_numpy_pipeline_on_f6(hip, oracle, start):
    """beam_ref -> audit_ref -> the rule, tuple for tuple, from pass 1's tuples and behind the reference's own rounds; the rows of
    resid_last and resid_prev it rewrote are audit_ref's residuals of the new prefixes, bit for bit, and no other row changed."""
    from lcrec_amd import generate_indices as gen
    z, cbs, greedy, held = bfc.f6_model()
    L = len(cbs)
    idx0 = greedy if start == "greedy" else held
    c = bfc.from_quantiser(z, cbs, idx0, 8)
    want_idx, want_choice, want_counters = (bfc.f6_flow(8)[k] for k in ("idx_beam", "choice", "counters")) if start == "greedy" else \
        finish_beam_ref(c["idx"], c["ks"], c["members"], c["offsets"], c["err_held"], c["cand"], c["cand_err"])
    r_last0, r_prev0 = bfc.prefix_resid(z, cbs, idx0, L - 1), bfc.prefix_resid(z, cbs, idx0, L - 2)
    idx, r_last, r_prev = dev(idx0), dev(r_last0), dev(r_prev0)
    done = gen.beam_finish_collisions(_model(cbs), idx, [dev(z[:1700]), dev(z[1700:])], r_last, list(c["ks"]), 8, resid_prev=r_prev)
    print(start, done, "want", want_counters)
    assert [done[k] for k in ("movers", "moved", "unresolved", "rounds")] == list(want_counters)
    got = idx.cpu().numpy()
    assert np.array_equal(got, want_idx)
    moved = c["members"][want_choice >= 0]
    want_sum = float(c["cand_err"][want_choice >= 0, want_choice[want_choice >= 0]].astype(np.float64).sum())
    assert done["err_moved_sum"] == pytest.approx(want_sum, rel=1e-12)              # (fp64 sums of the same fp32 values, in any order)
    want_last, want_prev = np.array(r_last0), np.array(r_prev0)
    want_last[moved] = bfc.prefix_resid(z[moved], cbs, want_idx[moved], L - 1)
    want_prev[moved] = bfc.prefix_resid(z[moved], cbs, want_idx[moved], L - 2)
    assert np.array_equal(_bits(r_last.cpu().numpy()), _bits(want_last)) and np.array_equal(_bits(r_prev.cpu().numpy()), _bits(want_prev))
    assert (want_idx[moved, :L - 1] != idx0[moved, :L - 1]).any()                     # a move no last-code pass can make
    if start == "held":
        assert done["unresolved"] == 0 and colliding_items(got, c["ks"]) == 0


def _checkpoint(tmp_path, g, meta):
    npy = str(tmp_path / "Toy.emb.npy")
    np.save(npy, gi.toy_items(meta["seed"]))
    kw = {k: v for k, v in meta["model"].items() if k != "in_dim"}
    sd = {k[4:]: torch.from_numpy(g[k].copy()) for k in g.files if k.startswith("sd__")}
    args = argparse.Namespace(data_path=npy, num_workers=0, **kw)
    ckpt = str(tmp_path / "toy.pth")
    torch.save({"args": args, "epoch": 0, "best_loss": 0.0, "best_collision_rate": 0.0, "state_dict": sd, "optimizer": {}}, ckpt,
               pickle_protocol=4)
    return ckpt


def test_generate_without_rounds_and_finish_beam_separates_every_f6_item(hip, oracle, tmp_path):
    from lcrec_amd import generate_indices as gen
    z, cbs, greedy, _ = bfc.f6_model()
    flow = bfc.f6_flow(8)
    ks = list(flow["case"]["ks"])
    g = fc.f6_case()[3]
    meta = json.load(open(os.path.join(fc.GOLD, "manifest.json")))["fixtures"]["f6_generate.npz"]
    ckpt = _checkpoint(tmp_path, g, meta)
    out = str(tmp_path / "Toy.index.json")
    stats = gen.generate(ckpt, out, device=DEV, verbose=False, rounds=0, finish="beam", audit=True)
    print({k: v for k, v in stats.items() if k != "audit"})
    held = gen.load_index_json(out, ks)                                              # the file parses back
    assert np.array_equal(held, flow["idx_final"])
    assert stats["collision_rate"] == 0.0 and stats["max_conflicts"] == 1 and stats["rounds"] == 0 and stats["finish"] == "beam"
    movers, moved, unresolved, rounds = flow["counters"]
    assert (stats["finish_beam_width"], stats["finish_beam_movers"], stats["finish_beam_moved"], stats["finish_beam_unresolved"],
            stats["finish_beam_rounds"]) == (8, movers, moved, unresolved, rounds)
    assert (stats["finish_moved"], stats["finish_unresolved"]) == flow["finish"]
    err = audit_ref(z, cbs, held)["err"].astype(np.float64)
    assert stats["audit"]["colliding_items"] == 0 and stats["audit"]["err_file_mean"] == pytest.approx(err.mean(), rel=1e-12)
    # the narrower widths run too, and leave more to the nearest-free step
    s2 = gen.generate(ckpt, str(tmp_path / "W2.index.json"), device=DEV, verbose=False, rounds=0, finish="beam", finish_width=2)
    assert s2["finish_beam_width"] == 2 and s2["finish_beam_movers"] == movers and s2["finish_beam_moved"] < moved
    assert s2["finish_beam_unresolved"] == s2["finish_moved"] + s2["finish_unresolved"] and "audit" not in s2
    # without the new flags the statistics carry none of the new keys
    plain = gen.generate(ckpt, str(tmp_path / "Plain.index.json"), device=DEV, verbose=False)
    assert not [k for k in plain if k.startswith("finish_beam")] and plain["finish"] == "none" and plain["rounds"] > 0
    assert open(str(tmp_path / "Plain.index.json"), "rb").read() == bytes(g["json_text"])
