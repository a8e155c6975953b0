"""The reference's other learners (index/trainer.py:49-81: SGD, Adagrad, RMSprop) on the captured training step.

Kernels (lcrec_{sgd,adagrad,rmsprop}_step, csrc/train_ops.hip) against torch's single-tensor CPU optimisers; the engine
(lcrec_amd/engine.py) against the same model trained by torch's optimiser through autograd; the Trainer end to end, its
checkpoints, the take-over of state the autograd path left, the data-parallel step and the improve fork's EMA runs."""
import os
import socket

import numpy as np
import pytest
import torch

import golden_inputs as gi

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
CLS = {"sgd": torch.optim.SGD, "adagrad": torch.optim.Adagrad, "rmsprop": torch.optim.RMSprop}
# every state tensor of each rule (the options that allocate them)
FULL = {"sgd": {"momentum": 0.9, "nesterov": True}, "adagrad": {"lr_decay": 0.01, "initial_accumulator_value": 0.1},
        "rmsprop": {"momentum": 0.9, "centered": True}}
SCHED = {"linear": 1, "constant": 0, None: -1}

KERNEL_CASES = [(rule, wd, sched, {}, 0) for rule in CLS for wd in (0.0, 1e-4) for sched in ("linear", "constant", None)] + [
    ("sgd", 1e-4, "linear", {"momentum": 0.9}, 0),
    ("sgd", 1e-4, "linear", {"momentum": 0.9, "nesterov": True}, 0),
    ("sgd", 0.0, "constant", {"momentum": 0.9, "dampening": 0.1}, 0),
    ("adagrad", 1e-4, "linear", {"lr_decay": 0.01, "initial_accumulator_value": 0.1}, 0),
    ("rmsprop", 1e-4, "linear", {"centered": True}, 0),
    ("rmsprop", 1e-4, "linear", {"momentum": 0.9}, 0),
    ("rmsprop", 1e-4, "constant", {"momentum": 0.9, "centered": True, "alpha": 0.9}, 0),
    ("rmsprop", 1e-4, "linear", {"centered": True, "alpha": 0.3}, 0),           # lerp's large-weight form
] + [(rule, 1e-4, "linear", FULL[rule], 1) for rule in CLS]          # buffers one float off 16-byte alignment: the scalar path


class _Flat:
    """Flat device buffers for one rule and its options, and one call of its update."""

    def __init__(self, rule, kw, p0, offset=0):
        self.rule, self.kw = rule, kw
        n = p0.size
        dev = torch.device(DEV)
        buf = lambda fill=0.0: torch.full((n + offset,), fill, dtype=torch.float32, device=dev)[offset:]
        self.p = buf()
        self.p.copy_(torch.from_numpy(p0))
        self.state = {}
        if rule == "sgd" and kw.get("momentum", 0):
            self.state["momentum_buffer"] = buf()
        if rule == "adagrad":
            self.state["sum"] = buf(kw.get("initial_accumulator_value", 0.0))
        if rule == "rmsprop":
            self.state["square_avg"] = buf()
            if kw.get("momentum", 0):
                self.state["momentum_buffer"] = buf()
            if kw.get("centered"):
                self.state["grad_avg"] = buf()
        self.ready = torch.zeros((), dtype=torch.bool, device=dev) if "momentum_buffer" in self.state and rule == "sgd" else None
        self.step = torch.zeros((), dtype=torch.int64, device=dev)
        self.lr_used = torch.zeros((), dtype=torch.float32, device=dev)
        self.n, self.offset = n, offset

    def grad(self, g):
        t = torch.zeros(self.n + self.offset, dtype=torch.float32, device=DEV)[self.offset:]
        t.copy_(torch.from_numpy(g))
        return t

    def update(self, ops, g, lr, wd, clip=None, schedule=-1, warmup=2, total=10, skip=None):
        kw, st = self.kw, self.state
        common = dict(clip=clip, schedule=schedule, warmup_steps=warmup, total_steps=total, lr_out=self.lr_used, skip_flag=skip)
        if self.rule == "sgd":
            ops.sgd_step(self.p, g, self.step, lr, kw.get("momentum", 0.0), kw.get("dampening", 0.0), kw.get("nesterov", False), wd,
                         momentum_buffer=st.get("momentum_buffer"), momentum_ready=self.ready, **common)
        elif self.rule == "adagrad":
            ops.adagrad_step(self.p, g, st["sum"], self.step, lr, kw.get("lr_decay", 0.0), kw.get("eps", 1e-10), wd, **common)
        else:
            ops.rmsprop_step(self.p, g, st["square_avg"], self.step, lr, kw.get("alpha", 0.99), kw.get("eps", 1e-8), wd,
                             kw.get("momentum", 0.0), kw.get("centered", False), momentum_buffer=st.get("momentum_buffer"),
                             grad_avg=st.get("grad_avg"), **common)


def _state_close(got, ref, what):
    # state tensors: relative, with an absolute floor of 1e-6 of the tensor's own scale (a momentum buffer crosses zero)
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-6 * max(float(np.abs(ref).max()), 1e-30), err_msg=what)


@pytest.mark.gpu
@pytest.mark.parametrize("rule,wd,schedule,kw,offset", KERNEL_CASES)
def test_clip_and_update_match_torch(hip, rule, wd, schedule, kw, offset):
    """Five steps of clip_grad_norm_(1.0) + the rule + the warm-up schedule on a flat buffer of 100 003 elements (a ragged
    tail) against torch's own single-tensor CPU implementation and transformers' multipliers (lcrec_amd.trainer)."""
    from lcrec_amd.trainer import constant_schedule_with_warmup, linear_schedule_with_warmup
    rs = np.random.RandomState(5)
    n = 100_003
    p0 = gi.f32(rs.standard_normal(n) * 0.1)
    grads = [gi.f32(rs.standard_normal(n) * s) for s in (0.001, 0.01, 0.02, 1e-4, 0.003)]
    lr = 1e-2
    pr = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = CLS[rule]([pr], lr=lr, weight_decay=wd, foreach=False, **kw)
    sched = {"linear": lambda: linear_schedule_with_warmup(opt, 2, 10), "constant": lambda: constant_schedule_with_warmup(opt, 2),
             None: lambda: None}[schedule]()
    fl = _Flat(rule, kw, p0, offset)
    identical = []
    for i, g in enumerate(grads):
        pr.grad = torch.from_numpy(g.copy())
        lr_ref = opt.param_groups[0]["lr"]
        norm_ref = torch.nn.utils.clip_grad_norm_([pr], 1.0)
        opt.step()
        if sched is not None:
            sched.step()
        gd = fl.grad(g)
        clip = hip.ops.grad_norm_clip(gd, 1.0)
        fl.update(hip.ops, gd, lr, wd, clip=clip, schedule=SCHED[schedule])
        np.testing.assert_allclose(clip[0].item(), float(norm_ref), rtol=1e-6)
        np.testing.assert_allclose(fl.lr_used.item(), lr_ref, rtol=1e-6, atol=1e-12)
        np.testing.assert_allclose(gd.cpu().numpy(), pr.grad.numpy(), rtol=1e-6, atol=1e-12)        # clipped in place
        got = fl.p.cpu().numpy()
        # centered RMSprop with a small alpha divides by sqrt(square_avg - grad_avg^2) of two near-equal terms: a last-bit
        # difference (torch's CPU sqrt is not IEEE-rounded, the clip coefficient comes from an fp64 norm) grows to ~1.6e-7
        # on a handful of the 100 003 elements; its state (grad_avg: the lerp's large-weight form) is held as tightly as any
        atol = 1e-6 if kw.get("centered") and kw.get("alpha", 0.99) < 0.5 else 1e-7
        np.testing.assert_allclose(got, pr.detach().numpy(), rtol=2e-5, atol=atol, err_msg=f"step {i}")
        identical.append(int((got == pr.detach().numpy()).sum()))
    assert int(fl.step.item()) == len(grads)
    st = opt.state[pr]
    assert sorted(k for k in st if k != "step") == sorted(fl.state)
    for k, t in fl.state.items():
        _state_close(t.cpu().numpy(), st[k].numpy(), k)
    if fl.ready is not None:
        assert bool(fl.ready)
    print(f"\n[{rule} wd={wd} schedule={schedule} {kw} offset={offset}] parameters bit-identical to torch after each step: "
          f"{identical} of {n}")


@pytest.mark.gpu
@pytest.mark.parametrize("rule", list(CLS))
def test_a_nan_loss_freezes_parameters_state_and_step(hip, rule):
    """skip_flag (the sticky NaN flag of lcrec_step_losses): nothing is updated and *step stays -- also on the very first
    step, where SGD's buffer must stay marked empty."""
    ops = hip.ops
    rs = np.random.RandomState(32)
    p0 = gi.f32(rs.standard_normal(10_000))
    fl = _Flat(rule, FULL[rule], p0)
    g = fl.grad(gi.f32(rs.standard_normal(10_000)))
    flag = torch.ones((), dtype=torch.bool, device=DEV)
    snap = lambda: [t.clone() for t in [fl.p, fl.step, fl.lr_used] + list(fl.state.values()) + ([fl.ready] if fl.ready is not None else [])]
    before = snap()
    fl.update(ops, g, 1e-2, 1e-4, skip=flag)
    assert all(torch.equal(a, b) for a, b in zip(before, snap())) and int(fl.step) == 0
    flag.zero_()
    fl.update(ops, g, 1e-2, 1e-4, skip=flag)
    good = snap()
    assert int(fl.step) == 1 and not torch.equal(good[0], before[0])
    flag.fill_(True)
    fl.update(ops, g, 1e-2, 1e-4, skip=flag)
    assert all(torch.equal(a, b) for a, b in zip(good, snap())) and int(fl.step) == 1


def _state_layout(opt):
    sd = opt.state_dict()["state"]
    return {i: {k: (tuple(v.shape), v.dtype) if torch.is_tensor(v) else type(v) for k, v in s.items()} for i, s in sd.items()}


def _tiny_model(hip, bn):
    g = np.load(os.path.join(GOLD, f"f4_step_bn{bn}.npz"))
    model = hip.RQVAE(in_dim=128, num_emb_list=[256] * 4, e_dim=16, layers=[64, 32], dropout_prob=0.0, bn=bool(bn),
                      loss_type="mse", quant_loss_weight=1.0, beta=0.25, kmeans_init=False, kmeans_iters=100,
                      sk_epsilons=[0.0, 0.0, 0.0, 0.003], sk_iters=50)
    model.load_state_dict({k[4:]: torch.from_numpy(g[k].copy()) for k in g.files if k.startswith("sd__")}, strict=True)
    return model.to(DEV).train()


def _run_sh_model(hip, bn):
    torch.manual_seed(7)
    x_init = torch.randn(512, 768, device=DEV)
    m = hip.RQVAE(in_dim=768, num_emb_list=[256] * 4, e_dim=32, layers=gi.RUN_SH_LAYERS, bn=bool(bn), kmeans_init=False,
                  sk_epsilons=[0.0, 0.0, 0.0, 0.003], sk_iters=50).to(DEV)
    with torch.no_grad():
        z = m.eval().encoder(x_init)
        for l, q in enumerate(m.rq.vq_layers):
            q.embedding.weight.copy_(z[torch.arange(256, device=DEV) * 2 + (l % 2)] * (0.6 ** l))
    return m.train()


LR = {"sgd": 1e-2, "adagrad": 1e-3, "rmsprop": 1e-4}


def _autograd_step(model, opt, sched, x):
    opt.zero_grad()
    out, rq_loss, _ = model(x)
    loss, _ = model.compute_loss(out, rq_loss, xs=x)
    loss.backward()
    norm = torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
    lr = opt.param_groups[0]["lr"]
    opt.step()
    sched.step()
    return loss.item(), float(norm), lr


def _compare_runs(rule, a, opt_a, b, opt_b, noise):
    """Parameters and optimiser state of the autograd run (a) and the engine run (b).  `noise`: names of parameters whose
    gradient is rounding noise in any evaluation (the bias of a Linear in front of a BatchNorm) -- Adagrad and RMSprop
    normalise it into steps of +-lr * O(1), so those are only bounded."""
    assert _state_layout(opt_b) == _state_layout(opt_a)
    step_bound = {"sgd": 1e-3, "adagrad": 8 * LR["adagrad"], "rmsprop": 80 * LR["rmsprop"]}[rule]
    names = dict(a.named_parameters())
    for k, pb in b.named_parameters():
        va, vb = names[k].detach().cpu().numpy(), pb.detach().cpu().numpy()
        assert np.abs(vb - va).max() < step_bound, (k, np.abs(vb - va).max())
        if k in noise:
            continue
        off = ~np.isclose(vb, va, rtol=1e-3, atol=1e-5)
        assert off.sum() <= max(8, 0.02 * off.size), (k, int(off.sum()), float(np.abs(vb - va).max()))
    sa, sb = opt_a.state_dict()["state"], opt_b.state_dict()["state"]
    order = [k for k, _ in a.named_parameters()]
    for i in sa:
        if order[i] in noise:
            continue
        for key, ta in sa[i].items():
            tb = sb[i][key]
            if key == "step":
                assert float(ta) == float(tb)
            elif key in ("sum", "square_avg"):
                # sums of squared gradients: noisy entries are tiny, the others agree closely
                ta, tb = ta.cpu().numpy(), tb.cpu().numpy()
                off = ~np.isclose(tb, ta, rtol=2e-2, atol=1e-3 * max(float(np.abs(ta).max()), 1e-30))
                assert off.sum() <= max(8, 0.02 * off.size), (i, key, int(off.sum()))


def _noise_params(model):
    out = set()
    for part in ("encoder", "decoder"):
        layers = getattr(model, part).mlp_layers
        for j, mod in enumerate(layers):
            if isinstance(mod, torch.nn.Linear) and j + 1 < len(layers) and isinstance(layers[j + 1], torch.nn.BatchNorm1d):
                out.add(f"{part}.mlp_layers.{j}.bias")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("bn", [0, 1])
@pytest.mark.parametrize("rule", list(CLS))
def test_engine_equals_autograd_path(hip, rule, bn, use_graph):
    """F4's model (tests/golden/f4_step_bn{0,1}.npz), four steps with a warm-up schedule: the engine (eager, or captured and
    replayed) against the same model trained by torch's optimiser through autograd -- losses, clip norm, learning rate,
    parameters, and the optimiser's state entries (torch's keys, shapes and dtypes)."""
    from lcrec_amd.engine import TrainEngine
    from lcrec_amd.trainer import linear_schedule_with_warmup
    x = [torch.from_numpy(gi.f32(gi.rs(400 + bn + s).standard_normal((256, 128)))).to(DEV) for s in range(2)]
    a, b = _tiny_model(hip, bn), _tiny_model(hip, bn)
    kw = FULL[rule] if use_graph else {}
    opt_a = CLS[rule](a.parameters(), lr=LR[rule], weight_decay=1e-4, **kw)
    opt_b = CLS[rule](b.parameters(), lr=LR[rule], weight_decay=1e-4, **kw)
    sched_a, sched_b = linear_schedule_with_warmup(opt_a, 1, 10), linear_schedule_with_warmup(opt_b, 1, 10)
    assert TrainEngine.unsupported_reason(b, opt_b) is None
    eng = TrainEngine(b, opt_b, "linear", 1, 10, use_graph=use_graph, scheduler=sched_b)
    for step in range(4):
        loss, norm, lr = _autograd_step(a, opt_a, sched_a, x[step % 2])
        eng.step(x[step % 2])
        np.testing.assert_allclose(eng.last[0].item(), loss, rtol=1e-5 if step == 0 else 3e-4, err_msg=f"loss, step {step}")
        np.testing.assert_allclose(eng.clip[0].item(), norm, rtol=1e-5 if step == 0 else 1e-3, err_msg=f"norm, step {step}")
        np.testing.assert_allclose(eng.lr_used.item(), lr, rtol=1e-6, atol=1e-12)
    eng.end_epoch(sched_b)
    assert eng.graph_replays == (3 if use_graph else 0)
    assert sched_b.last_epoch == sched_a.last_epoch == 4
    _compare_runs(rule, a, opt_a, b, opt_b, _noise_params(a) if bn else set())


@pytest.mark.gpu
@pytest.mark.parametrize("rule", list(CLS))
def test_engine_equals_autograd_path_on_the_run_sh_architecture(hip, rule):
    """index/run.sh's 768 -> 2048 ... 64 -> 32 with BatchNorm at batch 256, every state tensor of the rule, captured step."""
    from lcrec_amd.engine import TrainEngine
    from lcrec_amd.trainer import linear_schedule_with_warmup
    torch.manual_seed(5)
    xs = [torch.randn(256, 768, device=DEV) for _ in range(2)]
    a, b = _run_sh_model(hip, True), _run_sh_model(hip, True)
    opt_a = CLS[rule](a.parameters(), lr=LR[rule], weight_decay=1e-4, **FULL[rule])
    opt_b = CLS[rule](b.parameters(), lr=LR[rule], weight_decay=1e-4, **FULL[rule])
    sched_a, sched_b = linear_schedule_with_warmup(opt_a, 1, 10), linear_schedule_with_warmup(opt_b, 1, 10)
    assert TrainEngine.unsupported_reason(b, opt_b) is None
    eng = TrainEngine(b, opt_b, "linear", 1, 10, scheduler=sched_b)
    for step in range(4):
        loss, norm, lr = _autograd_step(a, opt_a, sched_a, xs[step % 2])
        eng.step(xs[step % 2])
        np.testing.assert_allclose(eng.last[0].item(), loss, rtol=1e-5 if step == 0 else 3e-4, err_msg=f"loss, step {step}")
        np.testing.assert_allclose(eng.lr_used.item(), lr, rtol=1e-6, atol=1e-12)
    eng.end_epoch(sched_b)
    assert eng.graph_replays == 3
    assert _state_layout(opt_b) == _state_layout(opt_a)


@pytest.mark.gpu
@pytest.mark.parametrize("rule,kw", [("adagrad", {}), ("sgd", {"momentum": 0.9}), ("rmsprop", {"momentum": 0.9, "centered": True})])
def test_engine_takes_over_the_autograd_state(hip, rule, kw):
    """Two autograd steps, then the engine: it picks up the optimiser's state (Adagrad's initial sum and step, SGD's momentum
    buffer -- whose existence it keeps in a device flag -- and, SGD keeping no step, the scheduler's count) and the run
    matches four autograd steps."""
    from lcrec_amd.engine import TrainEngine
    from lcrec_amd.trainer import linear_schedule_with_warmup
    x = [torch.from_numpy(gi.f32(gi.rs(410 + s).standard_normal((256, 128)))).to(DEV) for s in range(2)]
    a, b = _tiny_model(hip, 0), _tiny_model(hip, 0)
    opt_a = CLS[rule](a.parameters(), lr=LR[rule], weight_decay=1e-4, **kw)
    opt_b = CLS[rule](b.parameters(), lr=LR[rule], weight_decay=1e-4, **kw)
    sched_a, sched_b = linear_schedule_with_warmup(opt_a, 1, 10), linear_schedule_with_warmup(opt_b, 1, 10)
    for step in range(2):
        _autograd_step(a, opt_a, sched_a, x[step % 2])
        _autograd_step(b, opt_b, sched_b, x[step % 2])
    eng = TrainEngine(b, opt_b, "linear", 1, 10, scheduler=sched_b)
    assert eng.host_steps == 2
    for step in range(2, 4):
        loss, _, lr = _autograd_step(a, opt_a, sched_a, x[step % 2])
        eng.step(x[step % 2])
        np.testing.assert_allclose(eng.last[0].item(), loss, rtol=3e-4, err_msg=f"loss, step {step}")
        np.testing.assert_allclose(eng.lr_used.item(), lr, rtol=1e-6, atol=1e-12)
    eng.end_epoch(sched_b)
    assert eng.graph_replays == 1
    _compare_runs(rule, a, opt_a, b, opt_b, set())


def _trainer_run(cli, tmp_path, learner, mode, data, extra=(), epochs=3, batch=768):
    from lcrec_amd.datasets import DeviceLoader
    from lcrec_amd.trainer import Trainer
    argv = ["--data_path", "unused", "--ckpt_dir", str(tmp_path / f"{learner}{mode}"), "--device", DEV, "--batch_size", str(batch),
            "--epochs", str(epochs), "--eval_step", str(epochs), "--no_kmeans_init", "--num_emb_list", "32", "32", "32", "--e_dim",
            "32", "--layers", "64", "--sk_epsilons", "0.0", "0.0", "0.003", "--train_engine", mode, "--learner", learner,
            "--lr", "1e-3", "--lr_scheduler_type", "linear", "--warmup_epochs", "1"] + list(extra)
    args = cli.parse_args(argv)
    cli.seed_everything(2024)
    model = cli.build_model(args, 128)
    loader = DeviceLoader(data, batch, True, DEV)
    tr = Trainer(args, model, len(loader))
    losses = [tr._train_epoch(loader, e) for e in range(epochs)]
    return tr, losses, tr._valid_epoch(loader)


@pytest.mark.gpu
@pytest.mark.parametrize("learner", ["SGD", "Adagrad", "RMSprop"])
def test_trainer_runs_the_learner_on_the_engine(hip, tmp_path, learner):
    """--learner SGD / Adagrad / RMSprop: the Trainer takes the engine; epochs and collision rate as with --train_engine off;
    a checkpoint written under the engine has the autograd run's optimiser layout, reloads into a fresh torch optimiser
    and continues on the autograd path."""
    from lcrec_amd import generate_indices as gen
    from lcrec_amd import main as cli
    data = torch.from_numpy(gi.toy_items(3, n=3000, d=128)).to(DEV)
    on, lo, rate_on = _trainer_run(cli, tmp_path, learner, "auto", data, ["--bn", "True"])
    off, lf, rate_off = _trainer_run(cli, tmp_path, learner, "off", data, ["--bn", "True"])
    assert on.engine is not None and off.engine is None
    assert on.engine.graph_replays == 3 * 4 - 2
    np.testing.assert_allclose(np.array(lo), np.array(lf), rtol=1e-3)
    assert abs(rate_on - rate_off) < 0.02
    ck_on = gen.load_checkpoint(on._save_checkpoint(epoch=2, ckpt_file="e.pth"))
    ck_off = gen.load_checkpoint(off._save_checkpoint(epoch=2, ckpt_file="e.pth"))
    lay = lambda ck: {i: {k: (tuple(v.shape), v.dtype) for k, v in s.items()} for i, s in ck["optimizer"]["state"].items()}
    assert lay(ck_on) == lay(ck_off)
    assert ck_on["optimizer"]["param_groups"][0].keys() == ck_off["optimizer"]["param_groups"][0].keys()
    for s in ck_on["optimizer"]["state"].values():
        if "step" in s:
            assert float(s["step"]) == 12.0
    # the checkpoint continues on the autograd path
    fresh = cli.build_model(ck_on["args"], 128).to(DEV).train()
    fresh.load_state_dict(ck_on["state_dict"])
    opt = getattr(torch.optim, learner)(fresh.parameters(), lr=1e-3, weight_decay=ck_on["args"].weight_decay)
    opt.load_state_dict(ck_on["optimizer"])
    x = data[:768]
    for _ in range(2):
        opt.zero_grad()
        out, rq_loss, _ = fresh(x)
        loss, _ = fresh.compute_loss(out, rq_loss, xs=x)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(fresh.parameters(), 1.0)
        opt.step()
        assert bool(torch.isfinite(loss))
    for s in opt.state.values():
        if "step" in s:
            assert float(s["step"]) == 14.0


@pytest.mark.gpu
def test_improve_fork_ema_run_with_sgd_on_the_engine(hip, tmp_path):
    """index_improve's EMA codebook update (--ema_decay) with --learner SGD: engine and autograd path, same epochs."""
    from lcrec_amd import main as cli
    data = torch.from_numpy(gi.toy_items(4, n=3000, d=128)).to(DEV)
    extra = ["--no_bn", "--ema_decay", "0.9", "--reset_interval", "10000", "--reset_threshold", "0.01", "--reset_seed", "5"]
    on, lo, _ = _trainer_run(cli, tmp_path, "SGD", "auto", data, extra, epochs=2, batch=1000)
    off, lf, _ = _trainer_run(cli, tmp_path, "SGD", "off", data, extra, epochs=2, batch=1000)
    assert on.engine is not None and on.engine.graph_replays == 6 - 1 and off.engine is None
    np.testing.assert_allclose(np.array(lo), np.array(lf), rtol=5e-4)
    for qa, qb in zip(on.model.rq.vq_layers, off.model.rq.vq_layers):
        assert qa.step_count == qb.step_count == 6
        np.testing.assert_allclose(qa._ema_cluster_size.cpu().numpy(), qb._ema_cluster_size.cpu().numpy(), rtol=2e-3, atol=1e-3)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_run(rank, port, tmp, engine):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from lcrec_amd import dist as ldist, main as cli
    from lcrec_amd.datasets import DeviceLoader
    from lcrec_amd.trainer import Trainer
    argv = ["--data_path", "unused", "--ckpt_dir", os.path.join(tmp, f"ck{engine}"), "--device", DEV, "--batch_size", "96",
            "--epochs", "1", "--layers", "64", "32", "--e_dim", "16", "--num_emb_list", "32", "32", "32",
            "--sk_epsilons", "0.0", "0.0", "0.003", "--no_kmeans_init", "--bn", "True", "--learner", "RMSprop", "--lr", "1e-4",
            "--train_engine", engine]
    args = cli.parse_args(argv)
    ctx = ldist.init_from_env(args, backend="nccl", force=True)
    cli.seed_everything(2024)
    model = cli.build_model(args, 48)
    data = torch.randn((300, 48), generator=torch.Generator().manual_seed(7)).to(DEV)
    loader = DeviceLoader(data, 96, True, DEV, rank=ctx.rank, world_size=ctx.world_size)
    trainer = Trainer(args, model, len(loader))
    ldist.attach(trainer, ctx)
    torch.manual_seed(11)
    losses = [trainer._train_epoch(loader, 0)]
    eng = trainer.engine
    np.savez(os.path.join(tmp, f"{engine}.npz"), losses=np.array(losses), engine=np.int64(eng is not None),
             collectives=np.int64(getattr(eng, "collectives", 0)), replays=np.int64(getattr(eng, "graph_replays", 0)))
    ldist.shutdown(ctx)


@pytest.mark.gpu
def test_rmsprop_data_parallel_step_on_a_one_rank_rccl_group(hip, tmp_path):
    """One RMSprop epoch of the data-parallel step on a one-rank RCCL group: engine (exchanges captured) against the
    autograd path over the same group."""
    import torch.multiprocessing as mp
    tmp = str(tmp_path)
    for engine in ("auto", "off"):
        mp.spawn(_dp_run, args=(_free_port(), tmp, engine), nprocs=1, join=True)
    on, off = np.load(os.path.join(tmp, "auto.npz")), np.load(os.path.join(tmp, "off.npz"))
    assert int(on["engine"]) == 1 and int(off["engine"]) == 0
    assert int(on["collectives"]) > 0 and int(on["replays"]) > 0
    np.testing.assert_allclose(on["losses"], off["losses"], rtol=2e-4)


# ------------------------------------------------------------------ support matrix (host only)
def _cpu_model():
    import lcrec_amd
    return lcrec_amd.RQVAE(in_dim=32, num_emb_list=[16, 16], e_dim=16, layers=[32], bn=True, kmeans_init=False,
                           sk_epsilons=[0.0, 0.0])


@pytest.mark.parametrize("rule", list(CLS))
def test_the_learners_pass_the_optimizer_checks(rule):
    """SGD / Adagrad / RMSprop with the CLI's settings and with every option the kernels cover get past the optimiser checks
    (the CPU model then stops the engine, for its own reason)."""
    from lcrec_amd.engine import TrainEngine
    m = _cpu_model()
    for kw in ({}, FULL[rule]):
        opt = CLS[rule](m.parameters(), lr=1e-3, weight_decay=1e-4, **kw)
        assert TrainEngine.unsupported_reason(m, opt) == "model is not on a HIP device"


@pytest.mark.parametrize("rule", list(CLS))
def test_uncovered_optimizer_options_are_still_refused(rule):
    from lcrec_amd.engine import TrainEngine
    m = _cpu_model()
    reason = TrainEngine.unsupported_reason(m, CLS[rule](m.parameters(), lr=1e-3, maximize=True))
    assert reason is not None and "maximize" in reason
    enc, rest = list(m.encoder.parameters()), [p for n, p in m.named_parameters() if not n.startswith("encoder.")]
    reason = TrainEngine.unsupported_reason(m, CLS[rule]([{"params": enc}, {"params": rest, "lr": 1e-4}], lr=1e-3))
    assert reason is not None and "param group" in reason
