"""GPU: every row of tests/optim_cases.py through its optimiser entry point of the C ABI -- optim_step_kernel<RULE> of
csrc/train_ops.hip -- with a ticket and without one, every buffer and device scalar carved out of a sentinel-filled buffer at the
row's offset.  Per row and form, against the oracle's step (oracle/lcrec_oracle.c, written from the op tables of include/lcrec.h and
itself held to torch and to float64 by tests/test_optim_host.py), bit for bit: params, grads (the clipped values; untouched without a
clip pair and at coefficient 1), every state buffer, *step, momentum_ready and lr_out.  Where the oracle yields NaN (the planted
NaN lanes) the NaN masks are compared and the bits elsewhere, so a NaN lane's three neighbours in its float4 must be exact.  The two
forms agree bit for bit, the ticket word and its two neighbours are zero afterwards, no sentinel has changed.  With skip_flag set
nothing changes, and the next call equals the oracle's first step."""
import numpy as np
import pytest

import optim_cases as oc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev():
    import torch
    return torch.device(DEV)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bits_or_nan(got, want, what):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN at {np.flatnonzero(np.isnan(got) != nan)[:8]}, the oracle's at {np.flatnonzero(nan)[:8]}"
    bad = np.flatnonzero((bits(got) != bits(want)) & ~nan)
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} elements differ, first at {bad[0]}: {got[bad[0]]!r} vs {want[bad[0]]!r}"


def assert_state(got, want, r, what):
    """got: what optim_cases.run read back; want: optim_cases.expected."""
    assert sorted(got) == sorted(want)
    for k in ("p", "g") + oc.state_names(r):
        assert_bits_or_nan(got[k], want[k], f"{what}: {k}")
    assert got["step"] == want["step"], f"{what}: *step"
    assert got["ready"] == want["ready"], f"{what}: momentum_ready"
    assert got["lr"] == bits(want["lr"]), f"{what}: lr_out {got['lr']:#x}, the oracle's {float(want['lr'])!r}"


def assert_same(a, b, what):
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].tobytes() == b[k].tobytes(), f"{what}: {k}"
        else:
            assert a[k] == b[k], f"{what}: {k}"


@pytest.mark.parametrize("r", oc.ROWS, ids=oc.row_id)
def test_row_has_the_oracles_bits_in_both_forms(hip, r):
    assert hip.ops.optim_plan(r.count, r.off == "none", True) == oc.want_plan(r, True), r.why
    want = oc.expected(r)
    _, with_ticket = oc.run(hip, r, dev(), ticket=True)
    assert_state(with_ticket, want, r, "with a ticket")
    _, two_launches = oc.run(hip, r, dev(), ticket=False)
    assert_state(two_launches, want, r, "without a ticket")
    assert_same(with_ticket, two_launches, "ticket form vs two launches")
    if r.clip is None or r.clip == 1.0:
        assert with_ticket["g"].tobytes() == oc.inputs(r)["g"].tobytes(), "grads untouched"
    assert want["step"] == r.s0 + r.steps and (want["ready"] is None or want["ready"] == 1)


@pytest.mark.parametrize("ticket", (True, False), ids=("ticket", "two_launches"))
@pytest.mark.parametrize("r", oc.SKIP_ROWS, ids=oc.row_id)
def test_a_skipped_call_changes_nothing_and_the_next_is_the_first_step(hip, r, ticket):
    skipped, after = oc.run(hip, r, dev(), ticket=ticket, skip_first=True)
    for k, v in oc.inputs(r).items():
        assert skipped[k].tobytes() == v.tobytes(), f"skipped: {k} changed"
    assert skipped["step"] == r.s0, "skipped: *step moved"
    assert skipped["lr"] == oc.SENT32, "skipped: lr_out written"
    assert skipped["ready"] == (0 if r.rule == "sgd" else None), "skipped: momentum_ready set"
    assert_state(after, oc.expected(r), r, "the call after the skipped one")
