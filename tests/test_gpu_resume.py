"""--save_state / --resume / --stop_after_epoch / --init_from on the MI355X: a run that is stopped and resumed must
leave THE SAME BITS as the run that was never interrupted -- weights, optimizer state, EMA and BatchNorm buffers,
generator states, checkpoints, directory listing and per-epoch losses.  No tolerance anywhere: where one would be
needed, some state has not been restored.  The cases and the comparison are in resume_cases.py."""
import math
import os

import pytest
import torch

import resume_cases as rc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _argv(case, root, data, extra=(), schedule=rc.LINEAR):
    return ["--data_path", data, "--ckpt_dir", str(root), "--device", DEV] + rc.BASE + list(schedule) + rc.CASES[case] + list(extra)


def _cli(argv):
    """cli.main(argv) -> the (loss, recon) pairs Trainer._train_epoch returned, in order."""
    from lcrec_amd import main as cli
    from lcrec_amd.trainer import Trainer
    plain, seen = Trainer._train_epoch, []

    def recording(self, data, epoch_idx):
        seen.append(plain(self, data, epoch_idx))
        return seen[-1]
    Trainer._train_epoch = recording
    try:
        cli.main(argv)
    finally:
        Trainer._train_epoch = plain
    return seen


def _state(run_dir):
    from lcrec_amd import train_state
    return train_state.load(os.path.join(run_dir, train_state.FILE_NAME))


def _assert_same_run(s_dir, r_dir, s_losses, r_losses):
    """The whole comparison of the issue: final state file, every checkpoint, the listing, the epoch losses."""
    from lcrec_amd.checkpoint import load_checkpoint
    assert r_losses == s_losses and all(math.isfinite(v) for pair in s_losses for v in pair)
    files = sorted(os.listdir(s_dir))
    assert sorted(os.listdir(r_dir)) == files
    assert "train_state.pth" in files and "best_loss_model.pth" in files and "best_collision_model.pth" in files
    assert any(f.startswith(f"epoch_{rc.EPOCHS - 1}_") for f in files)
    a, b = _state(s_dir), _state(r_dir)
    assert a["epoch"] == rc.EPOCHS - 1 and rc.tensors_in(a) > 10
    assert rc.differences(a, b, "train_state") == []
    for f in files:
        if f == "train_state.pth":
            continue
        ca, cb = load_checkpoint(os.path.join(s_dir, f)), load_checkpoint(os.path.join(r_dir, f))
        assert sorted(ca) == rc.CHECKPOINT_KEYS
        assert isinstance(ca["best_loss"], float) and isinstance(ca["best_collision_rate"], float)
        assert rc.differences(ca, cb, f) == []


class _Runs:
    """Every run is made once and shared; nothing changes a finished run's directory afterwards."""

    def __init__(self, root):
        self.root, self.data, self.made = root, rc.write_toy(str(root / "Toy.emb-test-td.npy")), {}

    def straight(self, case, schedule=rc.LINEAR):
        key = ("S", case, tuple(schedule))
        if key not in self.made:
            root = self.root / ("S_%s_%d" % (case, len(self.made)))
            losses = _cli(_argv(case, root, self.data, ["--save_state"], schedule))
            self.made[key] = (rc.only_run_dir(root), losses)
        return self.made[key]

    def first_part(self, case, tag):
        """The same command with --stop_after_epoch: -> (argv, run directory, losses)."""
        root = self.root / ("R_%s_%s" % (case, tag))
        argv = _argv(case, root, self.data, ["--save_state"])
        losses = _cli(argv + ["--stop_after_epoch", str(rc.SPLIT)])
        return argv, rc.only_run_dir(root), losses

    def resumed(self, case):
        key = ("R", case)
        if key not in self.made:
            argv, run_dir, losses = self.first_part(case, "resumed")
            assert len(losses) == rc.SPLIT and _state(run_dir)["epoch"] == rc.SPLIT - 1
            losses = losses + _cli(argv + ["--resume", run_dir])
            assert rc.only_run_dir(os.path.dirname(run_dir)) == run_dir          # no second time-stamped folder
            self.made[key] = (run_dir, losses)
        return self.made[key]


@pytest.fixture(scope="module")
def runs(hip, tmp_path_factory):
    return _Runs(tmp_path_factory.mktemp("resume"))


# ------------------------------------------------------------------ 1. eager equals replayed
@pytest.mark.parametrize("case", rc.ENGINE_CASES)
def test_eager_step_and_replayed_step_leave_the_same_bits(hip, tmp_path, case):
    """A resumed process takes an eager step at each batch size where the straight run replays its graph: exact resume
    needs the two forms of a step to leave the same bits.  Two engines from identical state, the same two batches:
    one steps eagerly twice, the other eagerly once and then replays the graph it captures."""
    from lcrec_amd import main as cli
    from lcrec_amd.engine import TrainEngine
    from lcrec_amd.trainer import Trainer
    x = torch.from_numpy(rc.toy_matrix()).to(DEV)
    batches = [x[:128].contiguous(), x[128:256].contiguous()]

    def two_steps(use_graph):
        args = cli.parse_args(_argv(case, tmp_path / str(use_graph), "unused"))
        cli.seed_everything(2024)
        model = cli.build_model(args, rc.WIDTH)
        if args.reset_seed is not None:
            for l, q in enumerate(model.rq.vq_layers):
                q.reset_generator = torch.Generator(device=DEV).manual_seed(int(args.reset_seed) + l)
        tr = Trainer(args, model, 3)
        assert TrainEngine.unsupported_reason(tr.model, tr.optimizer, args, None, tr.use_ema) is None
        eng = TrainEngine(tr.model, tr.optimizer, "linear", tr.warmup_steps, tr.max_steps, use_graph=use_graph,
                          use_ema=tr.use_ema, scheduler=tr.scheduler, dropout_seed=1234)
        eng.begin_epoch()
        for b in batches:
            eng.step(b)
        sums = eng.end_epoch(tr.scheduler)
        got = {"flat_p": eng.flat_p.clone(), "last_idx": eng.last_idx.clone(), "step_count": eng.step_count.clone(),
               "last": eng.last.clone(), "clip": eng.clip.clone(), "lr_used": eng.lr_used.clone()}
        got.update({"state." + k: v.clone() for k, v in eng.flat_state.items()})
        got.update({"model." + k: v.clone() for k, v in tr.model.state_dict().items()})
        if eng._buf_ready is not None:
            got["buf_ready"] = eng._buf_ready.clone()
        replays = eng.graph_replays
        eng.release()
        return got, sums, replays

    eager, sums_e, replays_e = two_steps(False)
    mixed, sums_m, replays_m = two_steps(True)
    assert (replays_e, replays_m) == (0, 1)
    assert float(eager["lr_used"]) > 0 and int(eager["step_count"]) == 2             # the second step moved the parameters
    assert list(eager) == list(mixed)
    differing = [k for k in eager if not torch.equal(eager[k], mixed[k])]
    assert differing == [], differing
    assert sums_e == sums_m


# ------------------------------------------------------------------ 2. resume equals the straight run
@pytest.mark.parametrize("case", list(rc.CASES))
def test_resumed_run_equals_the_straight_run(runs, case):
    """Six epochs straight against three epochs, a new start from the state file, three more: split after epoch index 2,
    which is no evaluation epoch, lies inside the linear decay and follows a warm-up that ended with epoch 1."""
    s_dir, s_losses = runs.straight(case)
    r_dir, r_losses = runs.resumed(case)
    assert len(s_losses) == rc.EPOCHS
    state = _state(s_dir)
    assert state["engine"] is (not case.startswith("g_"))
    assert (state["dropout_seed"] is not None) == (case == "e_dropout")
    if case == "f_ema_resets":
        assert [lvl["step_count"] for lvl in state["levels"]] == [18, 18, 18]           # resets at steps 3, 6, 9 | 12, 15, 18
        assert all(lvl["reset_generator"] is not None for lvl in state["levels"])
    _assert_same_run(s_dir, r_dir, s_losses, r_losses)


# ------------------------------------------------------------------ 3. growing --epochs
def test_finished_run_resumed_with_more_epochs_equals_the_longer_run(runs):
    """constant schedule: nothing in a step depends on --epochs, so four finished epochs plus two equal six."""
    case = "a_adamw_bn_sinkhorn"
    s_dir, s_losses = runs.straight(case, schedule=[])
    root = runs.root / "grown"
    argv = _argv(case, root, runs.data, ["--save_state"], schedule=[])
    losses = _cli(argv + ["--epochs", "4"])
    run_dir = rc.only_run_dir(root)
    assert len(losses) == 4 and _state(run_dir)["epoch"] == 3
    losses += _cli(["--resume", os.path.join(run_dir, "train_state.pth"), "--epochs", "6"])     # (the file itself, no other flag)
    assert _state(run_dir)["args"].epochs == 6
    _assert_same_run(s_dir, run_dir, s_losses, losses)


# ------------------------------------------------------------------ 4. the mistakes this feature exists to avoid
def _final_weights_differ(s_dir, r_dir):
    a, b = _state(s_dir)["state_dict"], _state(r_dir)["state_dict"]
    return any(not torch.equal(a[k], b[k]) for k in a)


def test_comparison_sees_a_dropout_seed_drawn_afresh(runs, monkeypatch):
    from lcrec_amd.engine import TrainEngine
    s_dir, _ = runs.straight("e_dropout")
    argv, run_dir, _ = runs.first_part("e_dropout", "fresh_seed")
    plain = TrainEngine.__init__

    def forgetful(self, *a, **kw):
        kw["dropout_seed"] = None
        plain(self, *a, **kw)
    monkeypatch.setattr(TrainEngine, "__init__", forgetful)
    _cli(argv + ["--resume", run_dir])
    assert _state(run_dir)["epoch"] == rc.EPOCHS - 1
    assert _final_weights_differ(s_dir, run_dir)


def test_comparison_sees_an_unrestored_cpu_generator(runs, monkeypatch):
    from lcrec_amd import train_state
    s_dir, _ = runs.straight("a_adamw_bn_sinkhorn")
    argv, run_dir, _ = runs.first_part("a_adamw_bn_sinkhorn", "no_cpu_generator")
    plain = train_state.restore
    monkeypatch.setattr(train_state, "restore", lambda trainer, state: plain(trainer, state, skip_generators=("torch_cpu",)))
    _cli(argv + ["--resume", run_dir])
    assert _state(run_dir)["epoch"] == rc.EPOCHS - 1
    assert _final_weights_differ(s_dir, run_dir)                 # another permutation of the rows from epoch 3 on


# ------------------------------------------------------------------ 5. --init_from
@pytest.mark.parametrize("source", ["best_collision_model.pth", "train_state.pth"])
def test_init_from_starts_at_the_files_weights(runs, monkeypatch, source):
    """Before the first step the new run's model, in eval mode, gives the source file's model's forward bit for bit --
    both taken at the same moment, inside the run.  (An earlier form took the source model's forward before cli.main:
    twice, and only when the whole file ran in order, that one differed from both later ones in the last bit -- 1.2e-7
    on `out`, indices equal -- while the two later ones agreed.  Not reproduced in isolation and not explained; it
    concerns two forwards of one unchanged model, not --init_from.)"""
    from lcrec_amd import generate_indices as gen
    from lcrec_amd import layers
    from lcrec_amd import main as cli
    from lcrec_amd.trainer import Trainer
    case = "a_adamw_bn_sinkhorn"
    s_dir, _ = runs.straight(case)
    ckpt_path = os.path.join(s_dir, source)
    ckpt = gen.load_checkpoint(ckpt_path)
    grown = rc.write_toy(str(runs.root / "Grown.npy"), rows=350, seed=rc.SEED + 1)
    x = torch.from_numpy(rc.toy_matrix()).to(DEV)
    ref = gen.build_model_from_args(ckpt["args"], rc.WIDTH)
    ref.load_state_dict(ckpt["state_dict"])
    ref = ref.to(DEV).eval()
    monkeypatch.setattr(layers, "kmeans", lambda *a, **k: pytest.fail("--init_from ran k-means"))
    plain, seen = Trainer.fit, {}

    def checking(self, data):
        seen["initted"] = [q.initted for q in self.model.rq.vq_layers]
        seen["optimizer_state"] = len(self.optimizer.state)
        seen["start"], seen["rows"], seen["dir"] = self.start_epoch, data.data.shape[0], self.ckpt_dir
        self.model.eval()
        with torch.no_grad():
            seen["out"] = self.model(x)
            seen["want"] = ref(x)                     # the source model, on the same rows at the same moment
        return plain(self, data)
    monkeypatch.setattr(Trainer, "fit", checking)
    root = runs.root / ("init_" + source.split(".")[0])
    # k-means initialisation left ON (the default): --init_from marks every level initialised, so none runs
    argv = [a for a in _argv(case, root, grown) if a != "--no_kmeans_init"] + ["--init_from", ckpt_path, "--epochs", "2"]
    losses = _cli(argv)
    assert seen["initted"] == [True, True, True] and seen["optimizer_state"] == 0 and seen["start"] == 0 and seen["rows"] == 350
    assert os.path.dirname(seen["dir"]) == str(root) and seen["dir"] != s_dir              # a run directory of its own
    assert len(seen["want"]) == len(seen["out"]) == 3
    for name, a, b in zip(("out", "rq_loss", "indices"), seen["want"], seen["out"]):
        assert a.dtype == b.dtype and torch.equal(a, b), name
    assert len(losses) == 2 and all(math.isfinite(v) for pair in losses for v in pair)
    assert "train_state.pth" not in os.listdir(seen["dir"])


# ------------------------------------------------------------------ 6. flags absent on a real run
def test_run_without_the_new_flags_leaves_what_it_always_left(runs):
    from lcrec_amd.checkpoint import load_checkpoint
    case = "a_adamw_bn_sinkhorn"
    s_dir, s_losses = runs.straight(case)
    root = runs.root / "plain"
    losses = _cli(_argv(case, root, runs.data))
    run_dir = rc.only_run_dir(root)
    files = sorted(os.listdir(run_dir))
    assert "train_state.pth" not in files and not any(f.endswith(".tmp") for f in files)
    assert files == sorted(f for f in os.listdir(s_dir) if f != "train_state.pth")           # --save_state changes no other file
    for f in files:
        ck = load_checkpoint(os.path.join(run_dir, f))
        assert sorted(ck) == rc.CHECKPOINT_KEYS, f
        assert rc.differences(ck, load_checkpoint(os.path.join(s_dir, f)), f) == []
    assert losses == s_losses
