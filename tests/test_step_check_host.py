"""tests/step_check.py and the case recipe of tests/test_gpu_support_matrix.py on the host: what the GPU test relies on holds
for the CPU evaluations alone, and the judge does refuse a wrong gradient -- and a wrong code: one row sent to another code
than its only acceptable one is refused by its fp64 regret (step_check.CodeRule), where the count cap, the gradients and
the scalars all let it through; a row with two acceptable codes may take either."""
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
    own judgement; and every case of 16 rows or more uses more than one code per level.  The rule on the codes
    (step_check.CodeRule) holds for the reference alone: every cost of both evaluations is finite, the fp32 evaluation's own
    codes are acceptable on every row (the judge asserts it) and are the fp64 minimum, and the rule is not vacuous -- per
    level at most max(3, rows // 100) rows have more than one acceptable code."""
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
        rule = judge.yardsticks(idx32, masks, step)[4]
        for l, v in enumerate(rule.levels):
            several = rule.undecidable(l)
            print(f"case {letter}, step counter {step}, level {l}: rows with more than one acceptable code {several.tolist()} of "
                  f"{c['batch']}, acceptable codes on them {v['ok'][several].sum(1).tolist()}")
            assert v["finite"], (letter, step, l)
            assert np.array_equal(idx32[:, l], v["best"]), (letter, step, l)
            assert len(several) <= max(3, c["batch"] // 100), (letter, step, l, several)


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
    # ONE row with a single acceptable code sent to its fp64 runner-up: within the cap, gradients and scalars those of its own
    # problem -- refused by its fp64 regret alone
    row, code = _to_the_runner_up(judge.yardsticks(idx)[4], 1)
    moved = idx.copy()
    moved[row, 1] = code
    s1, g1 = step_check.evaluate(spec, sd, x, moved, torch.float32)
    with pytest.raises(AssertionError, match=rf"row {row} level 1:"):
        judge(g1, s1, moved, "one decidable row moved")


def _bump(a):
    b = a.copy()
    i = np.unravel_index(np.abs(b).argmax(), b.shape)
    b[i] *= 2.0
    return b


def _to_the_runner_up(rule, level):
    """(the first row of `level` with exactly one acceptable code, its fp64 runner-up)."""
    v = rule.levels[level]
    row = int(np.flatnonzero(v["ok"].sum(1) == 1)[0])
    return row, int(np.argsort(v["regret"][row], kind="stable")[1])


def _to_the_other_acceptable_code(rule, level):
    """(the first row of `level` with more than one acceptable code, the best of its acceptable codes but the fp64 minimum)."""
    v = rule.levels[level]
    row = int(rule.undecidable(level)[0])
    order = np.argsort(v["regret"][row], kind="stable")
    assert order[0] == v["best"][row] and v["ok"][row, order[1]]
    return row, int(order[1])


@pytest.fixture(scope="module")
def case_f():
    """Case F (131 rows: three 64-row tiles, the last one ragged; an argmin level, then a Sinkhorn level), its judge with the
    device paths' allowance of one row, the fp32 evaluation's own codes and the rule on them."""
    c, sd, x = gi.support_matrix_case("F")
    spec = step_check.spec_of(c, gi.SUPPORT_MATRIX_SK_ITERS)
    judge = step_check.Judge(spec, sd, x, exact_codes=False)
    idx = step_check.free_codes(spec, sd, x)
    return c, spec, sd, x, judge, idx, judge.yardsticks(idx)[4]


def _judge_moved(case, row, level, code, monkeypatch=None):
    """The fp32 evaluation of the problem with `row` sent to `code` on `level`, judged: its gradients and scalars are that
    problem's own and one row is within the cap, so only the rule on the codes can refuse it."""
    c, spec, sd, x, judge, idx, _ = case
    moved = idx.copy()
    moved[row, level] = code
    scalars, grads = step_check.evaluate(spec, sd, x, moved, torch.float32)
    if monkeypatch is not None:
        monkeypatch.setattr(step_check.CodeRule, "check", lambda self, idx, what: [])
    judge(grads, scalars, moved, f"case F, row {row} level {level} sent to code {code}")


@pytest.mark.parametrize("level", [0, 1])
def test_a_decidable_row_sent_to_its_runner_up_is_refused(case_f, level, monkeypatch):
    """Once on the argmin level and once on the Sinkhorn level of case F: the nearest wrong code there is.  Without the rule
    the same step passes -- gradients, scalars and the count cap do not see it."""
    row, code = _to_the_runner_up(case_f[6], level)
    with pytest.raises(AssertionError, match=rf"row {row} level {level}:"):
        _judge_moved(case_f, row, level, code)
    _judge_moved(case_f, row, level, code, monkeypatch)


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("row", [0, 128, 130])
def test_a_wrong_code_on_an_edge_row_is_refused(case_f, row, level):
    """Row 0, the first row of the ragged last 64-row tile and the last row, each sent to the next code: the rows an
    assignment kernel gets wrong at its edges, one at a time, which the count cap lets through."""
    c, idx = case_f[0], case_f[5]
    assert c["batch"] == 131 and row < c["batch"]
    with pytest.raises(AssertionError, match=rf"row {row} level {level}:"):
        _judge_moved(case_f, row, level, (idx[row, level] + 1) % c["codes"][level])


def test_an_undecidable_row_sent_to_its_other_acceptable_code_passes(case_f):
    """The allowance is still there for what it was made for: a near-tie of the fp64 evaluation (case F, last level)."""
    rule = case_f[6]
    row, code = _to_the_other_acceptable_code(rule, 1)
    print(f"case F level 1: row {row} to code {code}, regret {rule.levels[1]['regret'][row, code]:.3e}, threshold "
          f"{rule.levels[1]['threshold'][row, code]:.3e}")
    _judge_moved(case_f, row, 1, code)


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
