"""The training engine's support matrix (lcrec_amd/engine.py, TrainEngine.unsupported_reason), one step per configuration
against an fp64 evaluation of the same step: oracle/torch_ref.py on the CPU, judged by tests/step_check.py -- not the
autograd path, which runs the same kernels.  The cases (tests/golden_inputs.py SUPPORT_MATRIX) are the smallest shapes that
reach what the two architectures of tests/test_gpu_train.py never do:

    A, H  72 -> 40 -> 24 -> 16: no width is a multiple of 32, so every forward Linear takes the generic kernel with guarded
          loads (linear_fwd_64x64 / linear_fwd_128x32 in the trace, never linear_fwd_32x64), every dX product the zero-padded
          branch (out % 32 != 0; it then runs as linear_fwd_32x64), the grouped dW has out % 32 != 0, and no parameter but
          the 100- and 32-code books is a multiple of the flat buffers' 64-float alignment; l1 loss; codebooks of 100, 7 and 32
          codes; Sinkhorn on the last level.  H: the same with mse and dropout 0.5.
    B, G  128 -> 72 -> 40 -> 64 with BatchNorm at F = 72 and 40 (float4 strips plus a scalar rest), e_dim 64 (the one-workgroup
          input-gradient kernel), 64 and 48 codes, Sinkhorn on the FIRST level, beta 0.5, quant_loss_weight 0.3.  G: l1 and
          dropout 0.3.
    C     one Linear per MLP (layers = []), batch 2.
    D     Sinkhorn on all three levels, l1, BatchNorm, quant_loss_weight 2.
    E     batch 1 without BatchNorm, codebooks of 7 and 5 codes.
    F     136 -> 264 -> 72 -> 40 -> 32, BatchNorm at F = 264, 72, 40, batch 131 (three row tiles, the last one ragged), 256 and
          100 codes, l1.
    I     (not in the issue's table) two Sinkhorn levels of 600 x 32 entries each, above the 16 384 from which a level hands
          the engine a give-up probe: the second probe is OR-ed into the engine's flag by a launch of its own (probes[1:]).

test_step_check_host.py checks on the CPU that in every case the fp32 and fp64 evaluations choose the same codes on every
row (default seeds, dropout masks of step counters 0 and 1 included), so the cap on differently assigned rows is the device
path's alone.

The codes the device assigned are judged on every row and level, not only counted (step_check.CodeRule).  With C64 and C32 a
level's cost matrix -- torch_ref.distances on an argmin level, -ln Q of torch_ref.sinkhorn on a Sinkhorn level -- of the CPU
evaluation in fp64 and in fp32, both with the device's codes forced, b_i the fp64 minimum of row i and D = |C32 - C64|, the
code k of row i has to satisfy

    C64[i, k] - C64[i, b_i]  <=  f11_check.SLACK * (D[i, k] + D[i, b_i]) + floor(i, k)

floor = 2^-22 * (||R64_i||^2 + ||c_k||^2) on an argmin level, 1e-9 on a Sinkhorn level.  The one row a case may assign
differently from the fp32 evaluation is therefore a near-tie of the fp64 evaluation; a wrong code on the last row of a ragged
tile, on row 0 or on the first row of a workgroup's share is refused (test_step_check_host.py does exactly that to case F)."""
import numpy as np
import pytest
import torch
from torch import nn

import golden_inputs as gi
import step_check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 20240917                  # of the dropout masks (tests/test_gpu_dropout.py's first seed; test_step_check_host.py uses it too)
GENERIC = ("linear_fwd_64x64", "linear_fwd_128x32", "linear_fwd_128x64", "linear_fwd_128x128", "linear_fwd_pp_256x128")
_JUDGES = {}


def _dims(c):
    return [c["in_dim"]] + list(c["layers"]) + [c["e_dim"]]


def _case(hip, letter):
    """(configuration, judge, model on the device in training mode, batch on the device)."""
    c, sd, x = gi.support_matrix_case(letter)
    if letter not in _JUDGES:
        _JUDGES[letter] = step_check.Judge(step_check.spec_of(c, gi.SUPPORT_MATRIX_SK_ITERS), sd, x, exact_codes=c["batch"] <= 2)
    model = hip.RQVAE(in_dim=c["in_dim"], num_emb_list=list(c["codes"]), e_dim=c["e_dim"], layers=list(c["layers"]),
                      dropout_prob=c["dropout"], bn=c["bn"], loss_type=c["loss"], quant_loss_weight=c["qlw"], beta=c["beta"],
                      kmeans_init=False, sk_epsilons=list(c["sk"]), sk_iters=gi.SUPPORT_MATRIX_SK_ITERS)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, strict=True)
    return c, _JUDGES[letter], model.to(DEV).train(), torch.from_numpy(x).to(DEV)


def _device_masks(ops, c, step):
    """oracle/torch_ref.py's `masks` as the engine draws them: ops.dropout_mask (pinned to the host Philox recomputation by
    tests/test_gpu_dropout.py) of (seed, step counter, position) -- encoder 0 .. k-1, decoder k .. 2k-1 -- times s."""
    if not c["dropout"]:
        return None
    dims = _dims(c)
    k = len(dims) - 1
    s = float(np.float32(ops.dropout_threshold(c["dropout"])[1]))
    return {part: [ops.dropout_mask((c["batch"], d[l]), c["dropout"], SEED, step, pos0 + l, device=DEV).cpu().float() * s
                   for l in range(k)] for part, d, pos0 in (("encoder", dims, 0), ("decoder", dims[::-1], k))}


def _two_steps(hip, letter, make_optimizer, fuse_bn=False, trace=False):
    """The eager first step and the captured-and-replayed second one on the same batch, each judged by step_check.  The
    warm-up schedule's first learning rate is 0: both differentiate the same parameters (with dropout: under the masks of
    step counters 0 and 1)."""
    from lcrec_amd.engine import TrainEngine
    ops = hip.ops
    c, judge, model, x = _case(hip, letter)
    opt = make_optimizer(model.parameters())
    assert TrainEngine.unsupported_reason(model, opt) is None
    eng = TrainEngine(model, opt, "linear", 2, 10, fuse_bn=fuse_bn, dropout_seed=SEED if c["dropout"] else None)
    before = eng.flat_p.clone()
    launches = None
    for step, what in enumerate(("eager step", "captured step")):
        if trace and step == 0:
            ops.trace_enable(True)
        try:
            eng.step(x)
        finally:
            if trace and step == 0:
                launches = {k: v[0] for k, v in ops.trace_collect().items()}
                ops.trace_enable(False)
        coef = eng.clip[1].item()
        grads = {k: (p.grad / coef).cpu().numpy() for k, p in model.named_parameters()}
        loss, recon, rq_loss = eng.last.tolist()
        label = f"case {letter}, {type(opt).__name__}{', BatchNorm folded' if fuse_bn else ''}, {what}"
        judge(grads, [loss, recon, rq_loss, eng.clip[0].item()], eng.last_idx.cpu().numpy(), label,
              _device_masks(ops, c, step), step if c["dropout"] else None)
        assert int(eng.step_count) == step + 1
        if step == 0:
            assert torch.equal(eng.flat_p, before)           # learning rate 0 on the first step: same parameters again
    assert eng.graph_replays == 1
    eng.end_epoch()                                          # neither a NaN loss nor a Sinkhorn level that gave up
    eng.release()
    return c, model, launches


def _adamw(params):
    return torch.optim.AdamW(params, lr=1e-3, weight_decay=1e-4, fused=True)


@pytest.mark.parametrize("letter", sorted(gi.SUPPORT_MATRIX))
def test_one_step_per_configuration_against_fp64(hip, letter):
    c, model, launches = _two_steps(hip, letter, _adamw, trace=True)
    # which kernels the eager step's products took (the unfused line): a forward Linear runs on 32 x 64 tiles only when its
    # in_features is a multiple of 32, else on the generic kernel; every dX product (all layers but the encoder's first) runs
    # on 32 x 64 tiles -- one whose out_features is no multiple of 32 can only get there through the zero-padded branch, the
    # kernel refuses it otherwise; all weight gradients are one grouped launch (counted as linear_fwd_64x64)
    dims = _dims(c)
    k = len(dims) - 1
    fan_in = dims[:-1] + dims[::-1][:-1]
    print(f"case {letter}: launches of the eager step {launches}")
    aligned = sum(1 for w in fan_in if w % 32 == 0)
    assert launches.get("linear_fwd_32x64", 0) == aligned + (2 * k - 1), launches
    assert sum(launches.get(name, 0) for name in GENERIC) == (2 * k - aligned) + 1, launches
    assert launches.get("dropout", 0) == ((2 * k) + (2 * k - 1) if c["dropout"] else 0), launches
    if letter in "ABFGH":
        assert aligned < 2 * k                               # these cases are here for the generic kernel
    if c["bn"]:
        assert launches["bn_relu_forward"] == launches["bn_relu_backward"] == 2 * (k - 1)


@pytest.mark.parametrize("letter", sorted(gi.SUPPORT_MATRIX))
def test_one_step_per_configuration_with_batchnorm_folded(hip, letter, monkeypatch):
    """fuse_bn=True: BatchNorm folded into the GEMMs on either side where lcrec_linear_bn_forward takes every layer of an MLP
    (every in_features a multiple of 32 -- the encoders of D and I; with dropout never); everywhere else the engine takes the
    unfused line without a word, and must still pass.  The engine decides per MLP; a spy counts the folded launches."""
    ops = hip.ops
    c = gi.SUPPORT_MATRIX[letter]
    dims = _dims(c)
    foldable = {part: not c["dropout"] and all(ops.linear_bn_supported(c["batch"], d[l], d[l + 1]) for l in range(len(d) - 1))
                for part, d in (("encoder", dims), ("decoder", dims[::-1]))}
    calls = []
    real = ops.linear_bn_forward
    monkeypatch.setattr(ops, "linear_bn_forward", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    _two_steps(hip, letter, _adamw, fuse_bn=True)
    bn_layers = (len(dims) - 2) if c["bn"] else 0
    # per step (eager + captured = 2): a folded MLP with BatchNorm calls it for every layer, one without never needs it
    want = 2 * sum((len(dims) - 1) if (fold and bn_layers) else 0 for fold in foldable.values())
    assert len(calls) == want, (letter, foldable, len(calls), want)
    assert (want > 0) == (letter in "DI"), (letter, foldable)


@pytest.mark.parametrize("rule", ["sgd", "adagrad", "rmsprop"])
def test_case_a_under_the_other_learners(hip, rule):
    """Gradients and scalars only (the update rules have tests/test_gpu_learners.py)."""
    make = {"sgd": lambda p: torch.optim.SGD(p, lr=1e-3, weight_decay=1e-4, momentum=0.9),
            "adagrad": lambda p: torch.optim.Adagrad(p, lr=1e-3, weight_decay=1e-4),
            "rmsprop": lambda p: torch.optim.RMSprop(p, lr=1e-3, weight_decay=1e-4, centered=True)}[rule]
    _two_steps(hip, "A", make)


# ------------------------------------------------------------------ the edge of the matrix
_near = gi.near_miss


# name -> (configuration, activation, what must happen): "engine" = accepted, runs and passes step_check; "autograd" = a
# reason, and the Trainer's autograd path trains; ("error", text) = a reason, and nothing can run it: LcrecError naming the
# dimension before any launch; ("reference error", text): the reference's own ValueError
EDGE = {
    "hidden 36": (_near(layers=[36]), "relu", ("error", "in_features=36")),
    "hidden 100": (_near(layers=[100]), "relu", ("error", "in_features=100")),
    "in_dim 36": (_near(in_dim=36), "relu", ("error", "in_features=36")),
    "in_dim 100": (_near(in_dim=100), "relu", ("error", "in_features=100")),
    "hidden 6": (_near(layers=[6]), "relu", ("error", "in_features=6")),
    "e_dim 8": (_near(e_dim=8), "relu", ("error", "e_dim=8")),
    "e_dim 128": (_near(e_dim=128), "relu", ("error", "e_dim=128")),
    "leakyrelu": (_near(), "leakyrelu", "autograd"),
    "dropout 1.0": (_near(dropout=1.0), "relu", "autograd"),
    "loss huber": (_near(loss="huber"), "relu", ("reference error", "incompatible loss type")),
    # the accepted side of the same edges (tests/golden_inputs.py SUPPORT_EDGE, checked on the CPU like the cases above)
    "hidden 40": ("a", "relu", "engine"), "hidden 104": ("b", "relu", "engine"), "in_dim 40": ("c", "relu", "engine"),
    "in_dim 104": ("d", "relu", "engine"), "e_dim 64": ("e", "relu", "engine"), "dropout 0.9": ("f", "relu", "engine"),
}


@pytest.mark.parametrize("name", list(EDGE))
def test_the_edge_of_the_support_matrix(hip, name, tmp_path):
    """No configuration is accepted by unsupported_reason and then refused by a kernel: what it accepts runs (and is right);
    what it refuses either trains on the autograd path under --train_engine auto, or cannot run anywhere and says which
    dimension is at fault before the first launch."""
    from lcrec_amd import main as cli
    from lcrec_amd.datasets import DeviceLoader
    from lcrec_amd.engine import TrainEngine
    from lcrec_amd.layers import MLPLayers
    from lcrec_amd.trainer import Trainer
    ops = hip.ops
    c, activation, outcome = EDGE[name]
    if outcome == "engine":
        _two_steps(hip, c, _adamw)
        return
    argv = ["--data_path", "unused", "--ckpt_dir", str(tmp_path), "--device", DEV, "--batch_size", str(c["batch"]), "--epochs", "2",
            "--no_kmeans_init", "--num_emb_list", *map(str, c["codes"]), "--e_dim", str(c["e_dim"]), "--layers",
            *map(str, c["layers"]), "--sk_epsilons", *map(str, c["sk"]), "--train_engine", "auto", "--no_bn", "--loss_type",
            c["loss"], "--dropout_prob", str(c["dropout"]), "--lr_scheduler_type", "linear", "--warmup_epochs", "1"]
    args = cli.parse_args(argv)
    cli.seed_everything(2024)
    model = cli.build_model(args, c["in_dim"])
    if activation != "relu":
        model.encoder = MLPLayers(model.encode_layer_dims, dropout=c["dropout"], activation=activation, bn=False)
        model.decoder = MLPLayers(model.decode_layer_dims, dropout=c["dropout"], activation=activation, bn=False)
        assert any(isinstance(m, nn.LeakyReLU) for m in model.encoder.mlp_layers)
    data = torch.from_numpy(gi.f32(gi.rs(7).standard_normal((3 * c["batch"], c["in_dim"])))).to(DEV)
    loader = DeviceLoader(data, c["batch"], True, DEV)
    tr = Trainer(args, model, len(loader))
    reason = TrainEngine.unsupported_reason(tr.model, tr.optimizer, args)
    print(f"{name}: unsupported_reason = {reason!r}")
    assert reason is not None
    if outcome == "autograd":
        losses = [tr._train_epoch(loader, e) for e in range(2)]
        assert tr.engine is None and tr._engine_decided
        assert all(np.isfinite(v) for pair in losses for v in pair), losses
        return
    kind, text = outcome
    ops.trace_enable(True)
    try:
        with pytest.raises(ValueError if kind == "reference error" else hip.LcrecError, match=text):
            tr._train_epoch(loader, 0)
    finally:
        launched = ops.trace_collect()
        ops.trace_enable(False)
    assert tr.engine is None
    if kind == "error":
        assert launched == {}, launched                      # refused whole, before the first launch
        with pytest.raises(hip.LcrecError, match=text):      # and so do the module's own entry points
            tr.model(data[:4])
        with pytest.raises(hip.LcrecError, match=text):
            tr.model.eval().get_indices(data[:4])
