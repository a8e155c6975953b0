"""Dropout in the captured training step (csrc/train_ops.hip dropout_kernel, lcrec_amd/engine.py).

The mask is a function defined in include/lcrec.h -- Philox4x32-10 of (seed, step, position, element) -- so every check here
is against tests/philox_ref.py, a numpy restatement pinned to the generator's known answers by tests/test_dropout_host.py:
the kernels element for element, the engine against the autograd path running the SAME masks."""
import os

import numpy as np
import pytest
import torch
from torch import nn

import golden_inputs as gi
import philox_ref as ph

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
SEEDS = (20240917, (0x9E37 << 32) | 0x1234567)          # the second one above 2^32; both checked on the host (see the statistics test)
SHAPES = [(1024, 768), (1024, 2048), (475, 96), (2, 32), (1024, 32)]


@pytest.mark.parametrize("shape", SHAPES)
def test_mask_matches_the_host_recomputation(hip, shape):
    ops = hip.ops
    for p in (0.1, 0.5, 0.9):
        for seed in SEEDS:
            for step in (0, 1, 2 ** 31):
                for position, row_offset in ((0, 0), (9, 1531)):
                    got = ops.dropout_mask(shape, p, seed, step, position, row_offset=row_offset, device=DEV)
                    assert got.dtype == torch.uint8 and tuple(got.shape) == shape
                    want = ph.keep_mask(shape, p, seed, step, position, row_offset)
                    assert np.array_equal(got.cpu().numpy().astype(bool), want), (p, seed, step, position, row_offset)
    # seed and step as the device scalars the engine passes, a negative seed included (its 64 bits are the key)
    seed = torch.tensor(-SEEDS[1], dtype=torch.int64, device=DEV)
    step = torch.tensor(7, dtype=torch.int64, device=DEV)
    got = ops.dropout_mask(shape, 0.5, seed, step, 3)
    assert np.array_equal(got.cpu().numpy().astype(bool), ph.keep_mask(shape, 0.5, -SEEDS[1], 7, 3))


@pytest.mark.parametrize("shape", SHAPES)
def test_apply_matches_the_definition(hip, shape):
    ops = hip.ops
    rs = np.random.RandomState(shape[0] + shape[1])
    x_np = gi.f32(rs.standard_normal(shape) * 3.0)
    x_np[0, :4] = [np.inf, -np.inf, np.nan, -0.0]
    x = torch.from_numpy(x_np).to(DEV)
    for p in (0.1, 0.5, 0.9):
        for seed, step, position, row_offset in ((SEEDS[0], 0, 0, 0), (SEEDS[1], 2 ** 31, 13, 77)):
            keep = ph.keep_mask(shape, p, seed, step, position, row_offset)
            with np.errstate(invalid="ignore"):
                want = np.where(keep, x_np * ph.threshold(p)[1], np.float32(0.0))
            assert want.dtype == np.float32
            out = ops.dropout_apply(x, p, seed, step, position, row_offset=row_offset)
            assert out.data_ptr() != x.data_ptr() and np.array_equal(x.cpu().numpy(), x_np, equal_nan=True)
            assert np.array_equal(out.cpu().numpy(), want, equal_nan=True), (p, seed, step)
            assert not np.signbit(out.cpu().numpy()[~keep]).any()            # a dropped value is +0.0, whatever it was
            same = ops.dropout_mask(shape, p, seed, step, position, row_offset=row_offset, device=DEV)
            assert np.array_equal(same.cpu().numpy().astype(bool), keep)
            buf = x.clone()
            res = ops.dropout_apply(buf, p, seed, step, position, row_offset=row_offset, out=buf)      # in place
            assert res.data_ptr() == buf.data_ptr() and np.array_equal(buf.cpu().numpy(), want, equal_nan=True)
    # p = 0: x, unchanged
    out = ops.dropout_apply(x, 0.0, SEEDS[0], 5, 1)
    assert np.array_equal(out.cpu().numpy().view(np.uint32)[:, 4:], x_np.view(np.uint32)[:, 4:])
    assert np.array_equal(out.cpu().numpy(), x_np, equal_nan=True)
    for bad in (1.0, -0.25, 1.5):
        with pytest.raises(hip.LcrecError):
            ops.dropout_apply(x, bad, SEEDS[0], 0, 0)
        with pytest.raises(hip.LcrecError):
            ops.dropout_mask(shape, bad, SEEDS[0], 0, 0, device=DEV)
    with pytest.raises(hip.LcrecError):
        ops.dropout_apply(x[:, :shape[1] - 2].contiguous(), 0.1, SEEDS[0], 0, 0)          # features % 4 != 0


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("seed", SEEDS)
def test_mask_statistics(hip, p, seed):
    """Conditions, not measurements: the kept share of 1024 x 2048 elements within 5 binomial standard deviations of 1 - p;
    the agreement between two masks that differ only in step, only in position or only in seed (low word, high word) within 5
    standard deviations of p^2 + (1 - p)^2, what independent masks give.  SEEDS were chosen so that tests/philox_ref.py alone
    satisfies both (largest deviation over all cases: 2.8 standard deviations); the device masks equal those bit for bit."""
    ops = hip.ops
    shape = (1024, 2048)
    count = shape[0] * shape[1]
    mask = lambda seed_, step, position: ops.dropout_mask(shape, p, seed_, step, position, device=DEV).cpu().numpy().astype(bool)
    base = mask(seed, 5, 3)
    assert np.array_equal(base, ph.keep_mask(shape, p, seed, 5, 3))
    assert abs(base.mean() - (1.0 - p)) <= 5.0 * np.sqrt(p * (1.0 - p) / count)
    agree = p * p + (1.0 - p) ** 2
    for what, other in (("step", mask(seed, 6, 3)), ("position", mask(seed, 5, 4)), ("seed, low word", mask(seed ^ 1, 5, 3)),
                        ("seed, high word", mask(seed + (1 << 32), 5, 3))):
        assert abs((base == other).mean() - agree) <= 5.0 * np.sqrt(agree * (1.0 - agree) / count), what


# ------------------------------------------------------------------ the engine
def _tiny(hip, bn, dropout_prob, sk_last=0.0):
    """tests/test_gpu_train.py's _tiny with a dropout probability; sk_last: the last level's Sinkhorn epsilon (0 = argmin)."""
    g = np.load(os.path.join(GOLD, f"f4_step_bn{bn}.npz"))
    model = hip.RQVAE(in_dim=128, num_emb_list=[256] * 4, e_dim=16, layers=[64, 32], dropout_prob=dropout_prob, bn=bool(bn),
                      loss_type="mse", quant_loss_weight=1.0, beta=0.25, kmeans_init=False, kmeans_iters=100,
                      sk_epsilons=[0.0, 0.0, 0.0, sk_last], sk_iters=50)
    sd = {k[4:]: torch.from_numpy(g[k].copy()) for k in g.files if k.startswith("sd__")}
    model.load_state_dict(sd, strict=True)
    x = torch.from_numpy(gi.f32(gi.rs(400 + bn).standard_normal((256, 128)))).to(DEV)
    return model.to(DEV).train(), x


class _MaskedDropout(nn.Dropout):
    """nn.Dropout with the engine's mask: multiplies by lcrec_dropout_mask(seed, step, position) * s; `clock` is a one-element
    list holding the step, advanced by the test after every optimiser step."""

    def __init__(self, ops, p, seed, position, clock):
        super().__init__(p=p)
        self.ops, self.seed, self.position, self.clock = ops, seed, position, clock

    def forward(self, x):
        keep = self.ops.dropout_mask(x.shape, self.p, self.seed, self.clock[0], self.position, device=x.device)
        return x * (keep.to(x.dtype) * float(ph.threshold(self.p)[1]))


def _plant_masks(hip, model, seed, clock):
    k = len(model.encoder._groups)
    for mlp, pos0 in ((model.encoder, 0), (model.decoder, k)):
        for l, g in enumerate(mlp._groups):
            assert type(mlp.mlp_layers[g["drop"]]) is nn.Dropout
            mlp.mlp_layers[g["drop"]] = _MaskedDropout(hip.ops, mlp.dropout, seed, pos0 + l, clock)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("bn", [0, 1])
def test_engine_equals_the_autograd_path_with_the_same_masks(hip, bn, seed):
    """Copy A: the autograd path (torch AdamW, clip_grad_norm_) with every nn.Dropout replaced by one that multiplies by the
    mask of (seed, step, position).  Copy B: TrainEngine(dropout_seed=seed).  Three steps -- eager, captured, replayed.  Both
    run the same forward kernels, so the tolerances are those of test_engine_equals_autograd_path_on_the_run_sh_architecture
    (loss) and test_engine_reproduces_reference_trajectory (gradients) in tests/test_gpu_train.py.  Argmin levels only."""
    from lcrec_amd.engine import TrainEngine
    (a, x), (b, _) = _tiny(hip, bn, 0.1), _tiny(hip, bn, 0.1)
    clock = [0]
    _plant_masks(hip, a, seed, clock)
    opt_a = torch.optim.AdamW(a.parameters(), lr=1e-3, weight_decay=1e-4, fused=True)
    opt_b = torch.optim.AdamW(b.parameters(), lr=1e-3, weight_decay=1e-4, fused=True)
    assert TrainEngine.unsupported_reason(b, opt_b) is None
    eng = TrainEngine(b, opt_b, None, 0, 0, use_graph=True, dropout_seed=seed)
    assert int(eng.dropout_seed) == seed
    x_before = x.clone()
    for step in range(3):
        opt_a.zero_grad()
        out, rq_loss, _ = a(x)
        loss, _ = a.compute_loss(out, rq_loss, xs=x)
        loss.backward()
        grads = {k: p.grad.detach().cpu().numpy().copy() for k, p in a.named_parameters()}
        torch.nn.utils.clip_grad_norm_(a.parameters(), 1.0)
        opt_a.step()
        clock[0] += 1
        eng.step(x)
        torch.cuda.synchronize()
        assert torch.equal(x, x_before), f"step {step}: the batch was written"
        assert int(eng.step_count) == clock[0]
        print(f"bn {bn} seed {seed:#x} step {step}: autograd loss {loss.item():.9g} engine loss {eng.last[0].item():.9g}")
        np.testing.assert_allclose(eng.last[0].item(), loss.item(), rtol=1e-5 if step == 0 else 3e-4, err_msg=f"step {step}")
        if step == 0:
            gmax = max(np.abs(v).max() for v in grads.values())
            coef = eng.clip[1].item()
            worst = max(np.abs(p.grad.cpu().numpy() / coef - grads[k]).max() for k, p in b.named_parameters())
            print(f"  gradients: max |grad| {gmax:.6g}, clip coefficient {coef:.6g}, largest difference {worst:.3g}")
            for k, p in b.named_parameters():
                np.testing.assert_allclose(p.grad.cpu().numpy() / coef, grads[k], rtol=1e-4, atol=1e-6 * gmax, err_msg=k)
    assert eng.graph_replays == 2


@pytest.mark.parametrize("bn", [0, 1])
def test_a_replayed_step_draws_a_new_mask(hip, bn):
    from lcrec_amd.engine import TrainEngine
    # learning rate 0: the parameters stay as they are, so on one batch only the masks can move the loss from step to step
    model, x = _tiny(hip, bn, 0.1, sk_last=0.003)
    eng = TrainEngine(model, torch.optim.AdamW(model.parameters(), lr=0.0, weight_decay=1e-4, fused=True), None, 0, 0,
                      dropout_seed=SEEDS[0])
    before = eng.flat_p.clone()
    losses = []
    for _ in range(5):
        eng.step(x)
        losses.append(eng.last[0].item())
    assert eng.graph_replays == 4 and torch.equal(eng.flat_p, before) and int(eng.step_count) == 5
    assert all(np.isfinite(losses)) and len(set(losses)) == 5, losses
    eng.end_epoch()

    # the same seed: the same trajectory, bit for bit; another seed: another one
    def run(seed):
        m, xb = _tiny(hip, bn, 0.1, sk_last=0.003)
        e = TrainEngine(m, torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-4, fused=True), None, 0, 0, dropout_seed=seed)
        got = []
        for _ in range(3):
            e.step(xb)
            got.append(e.last.cpu().numpy().copy())
        assert e.graph_replays == 2
        return np.stack(got), e.flat_p.clone()

    (la, pa), (lb, pb), (lc, _) = run(SEEDS[1]), run(SEEDS[1]), run(SEEDS[0])
    assert np.array_equal(la, lb) and torch.equal(pa, pb)
    assert not np.array_equal(la[:, 0], lc[:, 0])


def test_seed_comes_from_torchs_generator_when_none_is_given(hip):
    from lcrec_amd.engine import TrainEngine

    def seed_of(dropout_prob):
        model, _ = _tiny(hip, 0, dropout_prob)
        torch.manual_seed(99)
        before = torch.get_rng_state()
        eng = TrainEngine(model, torch.optim.AdamW(model.parameters(), lr=1e-3, fused=True), None, 0, 0)
        return eng.dropout_seed, torch.equal(before, torch.get_rng_state())

    (s1, same1), (s2, _) = seed_of(0.1), seed_of(0.1)
    assert s1.is_cuda and s1.dtype == torch.int64 and int(s1) == int(s2) and not same1      # torch.manual_seed governs it
    none, same = seed_of(0.0)
    assert none is None and same                                             # p = 0: nothing drawn, nothing allocated


@pytest.mark.parametrize("bn", [0, 1])
def test_without_dropout_the_step_is_the_old_line(hip, bn, monkeypatch):
    from lcrec_amd.engine import TrainEngine
    calls = []
    real = hip.ops.dropout_apply
    monkeypatch.setattr(hip.ops, "dropout_apply", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def run(**extra):
        model, x = _tiny(hip, bn, 0.0, sk_last=0.003)
        eng = TrainEngine(model, torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4, fused=True), None, 0, 0, **extra)
        got = []
        for _ in range(3):
            eng.step(x)
            got.append(eng.last.cpu().numpy().copy())
        assert eng.graph_replays == 2 and eng.dropout_seed is None
        return np.stack(got)

    with_seed, plain = run(dropout_seed=SEEDS[0]), run()
    assert not calls
    assert np.array_equal(with_seed, plain)
    # (and the spy does see the calls of a model that has dropout)
    model, x = _tiny(hip, bn, 0.1)
    eng = TrainEngine(model, torch.optim.AdamW(model.parameters(), lr=1e-3, fused=True), None, 0, 0, dropout_seed=1)
    eng.step(x)
    k = len(model.encoder._groups)
    assert len(calls) == 2 * k + (2 * k - 1)          # every position going forward; all but the encoder's first going back


def test_trainer_runs_dropout_on_the_engine(hip, tmp_path):
    from lcrec_amd import main as cli
    from lcrec_amd import generate_indices as gen
    from lcrec_amd.datasets import DeviceLoader
    from lcrec_amd.trainer import Trainer
    data = torch.from_numpy(gi.toy_items(3, n=3000, d=128)).to(DEV)
    argv = ["--data_path", "unused", "--ckpt_dir", str(tmp_path / "drop"), "--device", DEV, "--batch_size", "768",
            "--epochs", "2", "--eval_step", "2", "--no_kmeans_init", "--num_emb_list", "32", "32", "32", "--e_dim", "32",
            "--layers", "64", "--sk_epsilons", "0.0", "0.0", "0.003", "--train_engine", "auto", "--bn", "True",
            "--lr_scheduler_type", "linear", "--warmup_epochs", "1", "--dropout_prob", "0.1"]
    args = cli.parse_args(argv)
    cli.seed_everything(2024)
    model = cli.build_model(args, 128)
    loader = DeviceLoader(data, 768, True, DEV)
    tr = Trainer(args, model, len(loader))
    per_epoch = [tr._train_epoch(loader, e) for e in range(2)]
    assert tr.engine is not None and tr.engine.dropout_seed is not None
    assert tr.engine.graph_replays == 2 * 4 - 2                  # as without dropout: one eager step at each of the two batch sizes
    assert all(np.isfinite(v) for pair in per_epoch for v in pair), per_epoch
    path = tr._save_checkpoint(epoch=1, ckpt_file="e.pth")
    ck = gen.load_checkpoint(path)
    fresh = cli.build_model(ck["args"], 128)
    fresh.load_state_dict(ck["state_dict"], strict=True)
    for k, v in tr.model.state_dict().items():
        assert torch.equal(v.cpu(), fresh.state_dict()[k]), k
