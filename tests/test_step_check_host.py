"""tests/step_check.py and the case recipe of tests/test_gpu_support_matrix.py on the host: what the GPU test relies on holds
for the CPU evaluations alone, and the judge does refuse a wrong gradient."""
import numpy as np
import pytest
import torch

import golden_inputs as gi
import philox_ref as ph
import step_check
from oracle import torch_ref

SEED = 20240917          # tests/test_gpu_dropout.py's first seed: the one the GPU test hands the engine


def host_masks(c, step, seed=SEED):
    """torch_ref's `masks` for step counter `step` from tests/philox_ref.py (the device masks equal it bit for bit,
    tests/test_gpu_dropout.py): positions encoder 0 .. k-1, decoder k .. 2k-1; a kept element carries s = (float)(1 / (1 - p))."""
    if not c["dropout"]:
        return None
    dims = [c["in_dim"]] + list(c["layers"]) + [c["e_dim"]]
    k = len(dims) - 1
    s = np.float32(ph.threshold(c["dropout"])[1])
    return {part: [torch.from_numpy(ph.keep_mask((c["batch"], d[l]), c["dropout"], seed, step, pos0 + l).astype(np.float32) * s)
                   for l in range(k)] for part, d, pos0 in (("encoder", dims, 0), ("decoder", dims[::-1], k))}


@pytest.mark.parametrize("letter", sorted(gi.SUPPORT_MATRIX) + sorted(gi.SUPPORT_EDGE))
def test_the_reference_alone_satisfies_what_the_gpu_test_asks(letter):
    """Per case (and, with dropout, per step counter 0 and 1): the fp32 and the fp64 evaluation choose the same codes on every
    row, so the cap on differently assigned rows leaves the device path its whole allowance; the fp32 evaluation passes its
    own judgement; and every case of 16 rows or more uses more than one code per level."""
    c, sd, x = gi.support_matrix_case(letter)
    spec = step_check.spec_of(c, gi.SUPPORT_MATRIX_SK_ITERS)
    judge = step_check.Judge(spec, sd, x, exact_codes=True)
    for step in ((0, 1) if c["dropout"] else (0,)):
        masks = host_masks(c, step)
        idx32 = step_check.free_codes(spec, sd, x, torch.float32, masks)
        idx64 = step_check.free_codes(spec, sd, x, torch.float64, masks)
        assert np.array_equal(idx32, idx64), (letter, step)
        assert all(0 <= idx32[:, l].min() and idx32[:, l].max() < K for l, K in enumerate(c["codes"]))
        if c["batch"] >= 16:
            assert all(len(set(idx32[:, l])) > 1 for l in range(idx32.shape[1]))
        scalars, g32 = step_check.evaluate(spec, sd, x, idx32, torch.float32, masks)
        rows = judge(g32, scalars, idx32, f"case {letter}, fp32 evaluation, step counter {step}", masks, step)
        assert max(r[3] for r in rows if r[1] == "rel") < 2e-5               # the reference's own fp32 distances stay small


def test_the_judge_refuses_wrong_gradients_scalars_and_codes():
    c, sd, x = gi.support_matrix_case("B")
    spec = step_check.spec_of(c, gi.SUPPORT_MATRIX_SK_ITERS)
    judge = step_check.Judge(spec, sd, x, exact_codes=False)
    idx = step_check.free_codes(spec, sd, x)
    scalars, grads = step_check.evaluate(spec, sd, x, idx, torch.float32)
    judge(grads, scalars, idx, "as evaluated")
    name = "encoder.mlp_layers.5.weight"
    for what, wrong in (("one tensor 1e-4 too large", {**grads, name: grads[name] * (1.0 + 1e-4)}),
                        ("one element of 2 880 off by its own size", {**grads, name: _bump(grads[name])}),
                        ("noise tensor that is not noise", {**grads, "encoder.mlp_layers.1.bias": grads["encoder.mlp_layers.2.bias"][:72] * 1e-3})):
        with pytest.raises(AssertionError, match="path"):
            judge(wrong, scalars, idx, what)
    with pytest.raises(AssertionError):
        judge(grads, [scalars[0] * (1 + 5e-5)] + scalars[1:], idx, "loss 5e-5 off")
    with pytest.raises(AssertionError):
        judge(grads, scalars[:3] + [scalars[3] * (1 + 5e-4)], idx, "gradient norm 5e-4 off")
    # two rows sent to another code: their own problem is evaluated exactly, but the cap on such rows holds
    moved = idx.copy()
    moved[:2, 1] = (moved[:2, 1] + 1) % c["codes"][1]
    s2, g2 = step_check.evaluate(spec, sd, x, moved, torch.float32)
    with pytest.raises(AssertionError, match="2"):
        judge(g2, s2, moved, "two rows moved")


def _bump(a):
    b = a.copy()
    i = np.unravel_index(np.abs(b).argmax(), b.shape)
    b[i] *= 2.0
    return b


def test_masks_in_the_oracle():
    """masks=None is the old call; masks of ones change nothing, bit for bit; a mask is the multiplication nn.Dropout makes."""
    c, sd, x = gi.support_matrix_case("G")
    spec = step_check.spec_of(c, gi.SUPPORT_MATRIX_SK_ITERS)
    leaf = lambda: {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
    xt = torch.from_numpy(x)
    with torch.no_grad():
        plain = torch_ref.forward(spec, leaf(), xt, training=True)
        masks = host_masks(c, 0)
        ones = {part: [torch.ones_like(m) for m in ms] for part, ms in masks.items()}
        same = torch_ref.forward(spec, leaf(), xt, training=True, masks=ones)
        assert all(torch.equal(a, b) for a, b in zip(plain, same))
        dropped = torch_ref.forward(spec, leaf(), xt, training=True, masks=masks)
        assert not torch.equal(plain[0], dropped[0])
        # layer 0 of the encoder by hand
        w, b = leaf()["encoder.mlp_layers.1.weight"], leaf()["encoder.mlp_layers.1.bias"]
        first = torch.nn.functional.linear(xt * masks["encoder"][0], w, b)
        one = torch_ref.mlp(leaf(), "encoder", xt, 1, False, True, {"encoder": masks["encoder"][:1]})
        assert torch.equal(first, one)
    kept = np.mean([float((m > 0).float().mean()) for ms in masks.values() for m in ms])
    assert abs(kept - (1 - c["dropout"])) < 0.02
