"""MI355X: the index-side entries that launch more than once per call, each recorded into a graph once and replayed on other inputs
(tests/capture_cases.py is the table; tests/test_capture_cases_host.py proves on the CPU that its two input sets share every
host-side argument and that this file's judge tells their results, and an unwritten buffer, apart).

include/lcrec.h says of lcrec_finish_nearest_free, lcrec_extend_nearest_free, lcrec_spill_nearest_free, lcrec_rq_audit and
lcrec_rq_beam: no allocation, no synchronisation, capturable.  Per row, every device buffer is allocated once: the inputs, the
outputs between guard bands, the counters, a workspace of exactly the queried size.  Then, on a stream that is not the default one:
  1. one eager call on input set A, compared with A's reference;
  2. one call recorded with torch.cuda.graph on that stream and nothing else inside -- a single chain;
  3. B copied into the input buffers (for the in/out idx: B's starting idx), every output refilled with garbage, the counters
     with a non-zero pattern and the workspace with 0xFF bytes; replay; everything compared with B's reference;
  4. the same back on A;
  5. A's and then B's inputs put back, a third replay: step 3's bits.
A host read of a counter, a launch on another stream, an allocation, or a host-side decision taken from device data at capture time
would each fail one of these.  Every comparison is exact: there is no tolerance in this file."""
import numpy as np
import pytest
import torch

import capture_cases as cc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAND = 256                                                  # bytes on either side of every buffer the calls write
BAND_BYTE = 0x5A
TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.int64): torch.int64, np.dtype(np.int32): torch.int32,
         np.dtype(np.uint32): torch.int32}


class Banded:
    """`count` elements of `dtype` as a view into a larger byte buffer: BAND bytes of BAND_BYTE, the elements, BAND bytes more."""

    def __init__(self, dtype, shape):
        self.nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full((BAND + self.nbytes + BAND,), BAND_BYTE, dtype=torch.uint8, device=DEV)
        self.bytes = self.raw[BAND:BAND + self.nbytes]
        self.view = self.bytes.view(dtype).view(shape)
        assert self.view.data_ptr() % 16 == 0

    def garbage(self):
        self.bytes.view(torch.int32).fill_(cc.GARBAGE)

    def bands_intact(self):
        return bool((self.raw[:BAND] == BAND_BYTE).all()) and bool((self.raw[BAND + self.nbytes:] == BAND_BYTE).all())


class Call:
    """One row's buffers and its call, in the form that touches nothing on the host."""

    def __init__(self, hip, row):
        self.hip, self.row = hip, row
        a = cc.variant(row, "A")
        host = self.host = a.host
        self.ks = [int(k) for k in host["ks"]]
        n, e, L = host["n"], host["e"], len(self.ks)
        self.inputs = {name: torch.empty(arr.shape, dtype=TORCH[arr.dtype], device=DEV) for name, arr in a.inputs.items()
                       if not (name == "idx" and "idx" in a.expected)}
        self.outputs = {name: Banded(TORCH[arr.dtype], arr.shape) for name, arr in a.expected.items()}
        self.in_out = [name for name in a.expected if name in a.inputs]                  # idx of the nearest-free passes
        lib, karr = hip._lib.load(), hip.ops._ints(self.ks)
        need = {"finish": 0, "extend": 0, "spill": lib.lcrec_spill_nearest_free_workspace(n),
                "rq_audit": lib.lcrec_rq_audit_workspace(n, e, karr, L),
                "rq_beam": lib.lcrec_rq_beam_workspace(n, e, karr, L, host.get("width", 1))}[row.entry]
        assert (need > 0) == (row.entry in ("spill", "rq_audit", "rq_beam"))
        self.workspace = Banded(torch.uint8, (need,)) if need else None

    def load(self, v):
        """a variant's inputs into the input buffers; the in/out idx starts from the variant's idx"""
        for name, t in self.inputs.items():
            t.copy_(torch.from_numpy(np.array(v.inputs[name])))
        for name in self.in_out:
            self.outputs[name].view.copy_(torch.from_numpy(np.array(v.inputs[name])))

    def dirty(self):
        """garbage in every output the call only writes, a non-zero pattern in the counters, 0xFF in the workspace"""
        for name, buf in self.outputs.items():
            if name not in self.in_out:
                buf.garbage()
        if self.workspace is not None:
            self.workspace.bytes.fill_(0xFF)

    def __call__(self, counters=None, workspace=None):
        """the row's call on its own buffers; `counters` / `workspace`: another tensor in that argument's place"""
        ops, i, o, ks, host = self.hip.ops, self.inputs, {k: b.view for k, b in self.outputs.items()}, self.ks, self.host
        entry = self.row.entry
        if counters is not None:
            o["counters"] = counters
        if workspace is None and self.workspace is not None:
            workspace = self.workspace.view
        if entry == "finish":
            got = ops.finish_nearest_free(o["idx"], i["resid"], i["cb"], ks, i["members"], i["offsets"], counters_out=o["counters"])
        elif entry == "extend":
            got = ops.extend_nearest_free(o["idx"], host["n_frozen"], i["resid"], i["cb"], ks, i["members"], i["offsets"],
                                          counters_out=o["counters"])
        elif entry == "spill":
            got = ops.spill_nearest_free(o["idx"], host["n_frozen"], i["r2"], i["r1"], i["cb_prev"], i["cb_last"], ks,
                                         (i["tuple_members"], i["tuple_offsets"]), (i["super_members"], i["super_offsets"]),
                                         counters_out=o["counters"], workspace=workspace)
        elif entry == "rq_audit":
            c0 = host["first_column"]
            got = ops.rq_audit_into(i["z"], i["codebooks"], ks, i["idx_wide"][:, c0:c0 + len(ks)], o, workspace=workspace)
        else:
            got = ops.rq_beam_into(i["z"], i["codebooks"], ks, host["width"], o, workspace=workspace)
        assert got is None                                                            # nothing was read back

    def result(self, stream):
        stream.synchronize()
        for name, buf in list(self.outputs.items()) + ([("workspace", self.workspace)] if self.workspace is not None else []):
            assert buf.bands_intact(), f"{name}: written outside its buffer"
        return {name: buf.view.cpu().numpy().copy() for name, buf in self.outputs.items()}


def check(got, want, what):
    for name in want:
        if not cc.same_bits(got[name], want[name]):
            g, w = np.asarray(got[name]), np.asarray(want[name])
            bad = np.flatnonzero((g.reshape(len(w), -1) != w.reshape(len(w), -1)).any(1))
            raise AssertionError((what, name, len(bad), bad[:8], g[bad[:4]], w[bad[:4]]))
    assert cc.judge(got, want), what


@pytest.mark.parametrize("row", cc.ROWS, ids=cc.row_id)
def test_the_call_is_recorded_once_and_replayed_on_other_inputs(hip, oracle, row):
    a, b = cc.variant(row, "A"), cc.variant(row, "B")
    call = Call(hip, row)                                                             # 1. every buffer, once, before the capture
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(side):
            call.load(a)
            call.dirty()
            call()                                                                    # 2. eagerly, off the default stream
            check(call.result(side), a.expected, (cc.row_id(row), "eager call on A, on a side stream"))
            call.load(a)
            call.dirty()
            untouched = call.result(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):                               # 3. one call, nothing else
                call()
            assert cc.judge(call.result(side), untouched), "the capture itself ran something"
            call.load(b)                                                              # 4. B through the graph
            call.dirty()
            graph.replay()
            first_b = call.result(side)
            check(first_b, b.expected, (cc.row_id(row), "first replay, on B"))
            call.load(a)                                                              # 5. back on A
            call.dirty()
            graph.replay()
            check(call.result(side), a.expected, (cc.row_id(row), "second replay, on A"))
            call.load(a)                                                              # 6. A's, then B's inputs put back: B again
            call.load(b)
            call.dirty()
            graph.replay()
            third = call.result(side)
            check(third, b.expected, (cc.row_id(row), "third replay, on B"))
            assert cc.judge(third, first_b)
    finally:
        torch.cuda.synchronize()                                                      # a failed row leaves nothing in flight


def test_the_new_arguments_are_refused_before_the_call(hip, oracle):
    """counters_out of the wrong dtype, shape or device and a workspace of the wrong dtype or device, or one byte too small: each is
    the binding's refusal -- the library is not called (its last-error text does not change, nothing is traced) and idx stays."""
    lib = hip._lib.load()
    before = lib.lcrec_last_error()
    good = torch.zeros(2, dtype=torch.int64, device=DEV)
    bad_counters = (torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(3, dtype=torch.int64, device=DEV),
                    torch.zeros(2, dtype=torch.int64), torch.zeros(4, dtype=torch.int64, device=DEV)[::2], [0, 0])
    hip.ops.trace_enable(True)
    try:
        for entry in ("finish", "extend", "spill"):
            call = Call(hip, cc.Row(entry, 16))
            a = cc.variant(call.row, "A")
            call.load(a)
            for bad in bad_counters:
                with pytest.raises(hip.LcrecError, match="counters_out must be"):
                    call(counters=bad)
        spill = Call(hip, cc.Row("spill", 16))
        spill.load(cc.variant(spill.row, "A"))
        audit = Call(hip, cc.Row("rq_audit", 16))
        audit.load(cc.variant(audit.row, "A"))
        for call in (spill, audit):
            need = call.workspace.nbytes
            for bad, text in ((torch.zeros(need // 4, dtype=torch.float32, device=DEV), "workspace must be"),
                              (torch.zeros(need, dtype=torch.uint8), "workspace must be"),
                              (torch.zeros(need - 1, dtype=torch.uint8, device=DEV), f"workspace of {need - 1} bytes, {need} needed")):
                with pytest.raises(hip.LcrecError, match=text):
                    call(workspace=bad)
        torch.cuda.synchronize()
        assert hip.ops.trace_collect() == {} and lib.lcrec_last_error() == before
        assert np.array_equal(spill.outputs["idx"].view.cpu().numpy(), cc.variant(spill.row, "A").inputs["idx"])
        # ... and with a counters_out that is right the same call goes through, and says what the reference says
        call = Call(hip, cc.Row("finish", 16))
        call.load(cc.variant(call.row, "A"))
        call(counters=good)
        torch.cuda.synchronize()
        assert good.tolist() == cc.variant(call.row, "A").expected["counters"].tolist()
    finally:
        hip.ops.trace_enable(False)
        hip.ops.trace_collect()
