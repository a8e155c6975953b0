"""--save_state / --resume / --init_from, the parts that need no GPU: the state file's round trip through the restricted
unpickler, the refusals, the checkpoint keeper across a restart, an interrupted write, and that nothing changes in a run
directory when the new flags are absent."""
import logging
import os
import pickle
import random

import numpy as np
import pytest
import torch

import resume_cases as rc


def _scripted_run(root, extra=(), rates=(0.5, 0.3, 0.4, 0.2, 0.6, 0.1), save_limit=2, reset_gen=False):
    """Trainer.fit on the CPU with scripted epochs (no kernel runs), one evaluation per epoch: -> (trainer, args)."""
    from lcrec_amd import main as cli
    from lcrec_amd import trainer as tr_mod
    args = cli.parse_args(rc.BASE + ["--ckpt_dir", str(root), "--device", "cpu", "--epochs", str(len(rates)), "--eval_step", "1",
                                     "--save_limit", str(save_limit), "--bn", "True", "--learner", "Adagrad",
                                     "--ema_decay", "0.99"] + list(extra))
    cli.seed_everything(2024)
    model = cli.build_model(args, rc.WIDTH)
    if reset_gen:
        for l, q in enumerate(model.rq.vq_layers):
            q.reset_generator = torch.Generator().manual_seed(7 + l)

    class Scripted(tr_mod.Trainer):
        def _train_epoch(self, data, epoch_idx):
            self.scheduler.last_epoch += 3          # three batches an epoch
            return 10.0 - epoch_idx, 5.0 - epoch_idx

        def _valid_epoch(self, data):
            self._evals = getattr(self, "_evals", 0) + 1
            return rates[self.start_epoch + self._evals - 1]

    t = Scripted(args, model, data_num=3, data_shape=(rc.ROWS, rc.WIDTH))
    logging.disable(logging.CRITICAL)
    try:
        t.fit(None)
    finally:
        logging.disable(logging.NOTSET)
    return t, args


# ------------------------------------------------------------------ round trip
def test_state_file_round_trips_through_the_restricted_unpickler(tmp_path):
    from lcrec_amd import _lib, train_state
    t, args = _scripted_run(tmp_path, ["--save_state"], reset_gen=True)
    random.random(), np.random.rand(), torch.rand(1)        # the generators are somewhere specific, not at their seeds
    t.model.rq.vq_layers[1].step_count = 17
    state = train_state.capture(t, 5)
    path = train_state.write(t.ckpt_dir, state)
    want = (random.random(), float(np.random.rand()), torch.rand(3), torch.rand(2, generator=t.model.rq.vq_layers[2].reset_generator))
    back = train_state.load(path)                           # load_checkpoint: a foreign global would have raised
    assert list(back) == list(state)
    assert rc.differences(state, back, "state") == []
    assert back["format"] == train_state.FORMAT_VERSION and back["abi"] == int(_lib.ABI_VERSION)
    assert vars(back["args"]) == vars(args)
    assert type(back["epoch"]) is int and back["epoch"] == 5 and type(back["scheduler_last_epoch"]) is int
    assert type(back["best_loss"]) is float and type(back["best_collision_rate"]) is float and back["cur_eval_step"] == 0
    for k, v in t.model.state_dict().items():
        assert back["state_dict"][k].dtype == v.dtype and torch.equal(back["state_dict"][k], v), k
    assert back["state_dict"]["encoder.mlp_layers.2.num_batches_tracked"].dtype == torch.int64
    assert back["optimizer"]["state"][0]["sum"].dtype == torch.float32
    gens = back["generators"]
    assert gens["torch_cpu"].dtype == torch.uint8 and gens["torch_device"] is None
    assert gens["numpy"]["keys"].dtype == torch.int64 and gens["numpy"]["keys"].shape == (624,) and gens["numpy"]["name"] == "MT19937"
    assert len(gens["python"]["words"]) == 625 and all(type(w) is int for w in gens["python"]["words"])
    for l, lvl in enumerate(back["levels"]):
        assert lvl["initted"] is True and lvl["step_count"] == (17 if l == 1 else 0)
        assert lvl["reset_generator"].dtype == torch.uint8
    assert back["keeper"]["newest"] == [[-0.6, "epoch_4_collision_0.6000_model.pth"], [-0.1, "epoch_5_collision_0.1000_model.pth"]]
    assert (back["dropout_seed"], back["engine"], back["world_size"]) == (None, None, 1)
    assert (back["data_rows"], back["data_width"]) == (rc.ROWS, rc.WIDTH)

    # into a fresh trainer: every generator goes on where the saved one was
    from lcrec_amd import main as cli
    from lcrec_amd.trainer import Trainer
    model = cli.build_model(args, rc.WIDTH)
    for l, q in enumerate(model.rq.vq_layers):
        q.reset_generator = torch.Generator().manual_seed(99)
    fresh = Trainer(args, model, 3, run_dir=t.ckpt_dir)
    train_state.restore(fresh, back)
    got = (random.random(), float(np.random.rand()), torch.rand(3), torch.rand(2, generator=model.rq.vq_layers[2].reset_generator))
    assert got[:2] == want[:2] and torch.equal(got[2], want[2]) and torch.equal(got[3], want[3])
    assert fresh.start_epoch == 6 and fresh.scheduler.last_epoch == 18 and model.rq.vq_layers[1].step_count == 17
    assert fresh.ckpt_dir == t.ckpt_dir and (fresh.best_loss, fresh.best_collision_rate) == (t.best_loss, t.best_collision_rate)
    assert rc.differences(t.optimizer.state_dict()["state"], fresh.optimizer.state_dict()["state"], "optimizer") == []
    assert fresh.optimizer.param_groups[0]["lr"] == fresh.scheduler.get_last_lr()[0] == args.lr     # constant, past its warm-up


def test_hostile_state_file_is_refused_and_nothing_runs(tmp_path):
    from lcrec_amd import train_state
    marker = tmp_path / "pwned"

    class Evil:
        def __reduce__(self):
            return (os.system, ("echo pwned > %s" % marker,))
    torch.save({"format": train_state.FORMAT_VERSION, "args": Evil()}, tmp_path / train_state.FILE_NAME, pickle_protocol=4)
    with pytest.raises(pickle.UnpicklingError, match="system"):
        train_state.load(train_state.locate(str(tmp_path)))
    assert not marker.exists()


# ------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def saved_run(tmp_path_factory):
    root = tmp_path_factory.mktemp("saved")
    t, args = _scripted_run(root, ["--save_state"])
    data = rc.write_toy(str(root / "Toy.npy"))
    return t.ckpt_dir, args, data


def test_resume_refuses_a_missing_file(tmp_path):
    from lcrec_amd import main as cli
    with pytest.raises(FileNotFoundError, match="no state file at .*train_state.pth"):
        cli.main(["--resume", str(tmp_path)])
    with pytest.raises(FileNotFoundError, match="nowhere.pth"):
        cli.main(["--resume", str(tmp_path / "nowhere.pth")])


def test_resume_refuses_an_unknown_format_version(tmp_path, saved_run):
    from lcrec_amd import main as cli
    from lcrec_amd import train_state
    state = train_state.load(os.path.join(saved_run[0], train_state.FILE_NAME))
    state["format"] = 99
    train_state.write(str(tmp_path), state)
    with pytest.raises(ValueError, match="format version 99"):
        cli.main(["--resume", str(tmp_path)])
    # a checkpoint is not a state file
    with pytest.raises(ValueError, match="format version None"):
        cli.main(["--resume", os.path.join(saved_run[0], "best_loss_model.pth")])


def test_resume_refuses_a_conflicting_flag_before_it_reads_data(saved_run, monkeypatch):
    from lcrec_amd import main as cli
    monkeypatch.setattr(cli, "EmbDataset", lambda *a, **k: pytest.fail("the data was loaded before the flags were checked"))
    with pytest.raises(ValueError, match=r"--lr is 0\.5 on the command line and 0\.001 in the saved run"):
        cli.main(["--resume", saved_run[0], "--lr", "0.5"])
    with pytest.raises(ValueError, match=r"--num_emb_list is \[16, 16\] on the command line and \[16, 16, 16\]"):
        cli.main(["--resume", saved_run[0], "--num_emb_list", "16", "16"])
    with pytest.raises(ValueError, match=r"--learner is 'SGD' on the command line and 'Adagrad'"):
        cli.main(["--resume", saved_run[0], "--learner", "SGD"])


def test_resume_accepts_the_flags_that_may_differ_and_repeated_ones(saved_run):
    from lcrec_amd import main as cli
    from lcrec_amd import train_state
    run_dir, saved, _ = saved_run
    argv = ["--resume", run_dir, "--epochs", "9", "--save_limit", "4", "--stop_after_epoch", "8", "--data_path", "elsewhere.npy",
            "--device", "cpu", "--lr", "0.001", "--learner", "Adagrad", "--bn", "True", "--no_kmeans_init"]
    args = train_state.resume_args(saved, cli.parse_args(argv), cli.given_flags(argv))
    assert (args.epochs, args.save_limit, args.stop_after_epoch, args.data_path) == (9, 4, 8, "elsewhere.npy")
    assert args.resume == run_dir and args.save_state is True and args.ema_decay == saved.ema_decay
    assert train_state.resume_args(saved, cli.parse_args(argv[:2]), cli.given_flags(argv[:2])).stop_after_epoch is None


@pytest.mark.parametrize("rows,width", [(rc.ROWS + 50, rc.WIDTH), (rc.ROWS, rc.WIDTH // 2)])
def test_resume_refuses_another_row_count_or_width(tmp_path, saved_run, rows, width):
    from lcrec_amd import main as cli
    other = str(tmp_path / "Other.npy")
    np.save(other, np.zeros((rows, width), dtype=np.float32))
    with pytest.raises(ValueError, match=f"{rows} rows x {width} columns, the saved run had {rc.ROWS} x {rc.WIDTH}"):
        cli.main(["--resume", saved_run[0], "--data_path", other])


def test_resume_refuses_another_world_size_and_more_than_one_rank(saved_run):
    import argparse
    from lcrec_amd import train_state
    state = train_state.load(os.path.join(saved_run[0], train_state.FILE_NAME))
    train_state.check_world(state, 1)
    with pytest.raises(ValueError, match="world size 2, the saved run had 1"):
        train_state.check_world(state, 2)
    train_state.refuse_ranks(argparse.Namespace(resume="x", save_state=True), 1)          # a one-rank group is a single process
    with pytest.raises(ValueError, match="--resume under torchrun"):
        train_state.refuse_ranks(argparse.Namespace(resume="x", save_state=False), 2)
    with pytest.raises(ValueError, match="--save_state under torchrun"):
        train_state.refuse_ranks(argparse.Namespace(resume=None, save_state=True), 2)
    train_state.refuse_ranks(argparse.Namespace(resume=None, save_state=False), 2)


def test_resume_and_init_from_exclude_each_other(saved_run):
    from lcrec_amd import main as cli
    with pytest.raises(ValueError, match="--resume and --init_from exclude each other"):
        cli.main(["--resume", saved_run[0], "--init_from", os.path.join(saved_run[0], "best_loss_model.pth")])


_SAVED_ARCH = ["--bn", "True", "--ema_decay", "0.99"]       # what _scripted_run's model was built with, beyond rc.BASE


@pytest.mark.parametrize("field,flags,width,message", [
    ("num_emb_list", _SAVED_ARCH + ["--num_emb_list", "16", "16", "32"], rc.WIDTH,
     r"num_emb_list is \[16, 16, 32\] here and \[16, 16, 16\] in"),
    ("e_dim", _SAVED_ARCH + ["--e_dim", "32"], rc.WIDTH, "e_dim is 32 here and 16 in"),
    ("layers", _SAVED_ARCH + ["--layers", "32", "24"], rc.WIDTH, r"layers is \[32, 24\] here and \[32\] in"),
    ("bn", _SAVED_ARCH + ["--no_bn"], rc.WIDTH, "bn is False here and True in"),
    ("input width", _SAVED_ARCH, rc.WIDTH + 8, f"input width is {rc.WIDTH + 8} here .* and {rc.WIDTH} in"),
    ("ema_decay", ["--bn", "True"], rc.WIDTH, "ema_decay is not set here and set in"),
])
@pytest.mark.parametrize("source", ["best_loss_model.pth", "train_state.pth"])
def test_init_from_refuses_another_architecture(saved_run, field, flags, width, message, source):
    from lcrec_amd import main as cli
    from lcrec_amd import train_state
    args = cli.parse_args(rc.BASE + flags)
    path = os.path.join(saved_run[0], source)
    with pytest.raises(ValueError, match="--init_from: " + message):
        train_state.init_weights(path, args, width)
    same = cli.parse_args(rc.BASE + ["--bn", "True", "--ema_decay", "0.5", "--lr", "0.1", "--learner", "SGD"])
    sd = train_state.init_weights(path, same, rc.WIDTH)                 # what is no architecture may differ
    cli.build_model(same, rc.WIDTH).load_state_dict(sd)


def test_init_from_refuses_a_missing_file(tmp_path):
    from lcrec_amd import main as cli
    from lcrec_amd import train_state
    with pytest.raises(FileNotFoundError, match="--init_from: no file at"):
        train_state.init_weights(str(tmp_path / "none.pth"), cli.parse_args(rc.BASE), rc.WIDTH)


# ------------------------------------------------------------------ keeper
def test_restored_keeper_removes_what_the_uninterrupted_one_removes(tmp_path):
    from lcrec_amd import train_state
    from lcrec_amd.checkpoint import load_checkpoint
    from lcrec_amd.trainer import CheckpointKeeper
    rates = [0.5, 0.2, 0.4, 0.3, 0.1, 0.6, 0.25]
    name = lambda run, e: os.path.join(run, "epoch_%d_collision_%.4f_model.pth" % (e, rates[e]))
    straight, gone_s = [], []
    keeper = CheckpointKeeper(2, remove=gone_s.append)
    for e in range(len(rates)):
        keeper.add(rates[e], name("run", e))
        straight.append(list(gone_s))
    gone_a = []
    first = CheckpointKeeper(2, remove=gone_a.append)
    for e in range(4):
        first.add(rates[e], name("run", e))
    torch.save({"keeper": train_state.keeper_entries(first)}, tmp_path / "k.pth", pickle_protocol=4)
    entries = load_checkpoint(str(tmp_path / "k.pth"))["keeper"]
    assert all(os.sep not in f for _, f in entries["best"] + entries["newest"])       # relative to the run directory
    gone_b = []
    second = CheckpointKeeper(2, remove=gone_b.append)
    train_state.restore_keeper(second, entries, "run")
    assert second.best == first.best and second.newest == first.newest
    for e in range(4, 7):
        second.add(rates[e], name("run", e))
        assert gone_a + gone_b == straight[e], e
    assert len(gone_b) >= 2 and second.best == keeper.best and second.newest == keeper.newest


# ------------------------------------------------------------------ interrupted write
def test_interrupted_write_leaves_the_previous_state_file(tmp_path, monkeypatch):
    from lcrec_amd import train_state
    t, _ = _scripted_run(tmp_path, ["--save_state"], rates=(0.5, 0.3))
    path = os.path.join(t.ckpt_dir, train_state.FILE_NAME)
    before = open(path, "rb").read()
    later = train_state.capture(t, 7)

    def dies(src, dst):
        raise KeyboardInterrupt("between the temporary file and the rename")
    monkeypatch.setattr(train_state.os, "replace", dies)
    with pytest.raises(KeyboardInterrupt):
        train_state.write(t.ckpt_dir, later)
    monkeypatch.undo()
    assert open(path, "rb").read() == before
    assert train_state.load(path)["epoch"] == 1
    train_state.write(t.ckpt_dir, later)                   # the next write goes through, over the leftover temporary
    assert train_state.load(path)["epoch"] == 7
    assert sorted(f for f in os.listdir(t.ckpt_dir) if "train_state" in f) == [train_state.FILE_NAME]


# ------------------------------------------------------------------ flags absent
def test_without_the_new_flags_a_run_directory_is_what_it_was(tmp_path):
    from lcrec_amd.checkpoint import load_checkpoint
    rates = (0.5, 0.3, 0.4, 0.2, 0.6, 0.1)
    want = rc.parent_listing(range(len(rates)), rates, 2)
    t, _ = _scripted_run(tmp_path / "plain", rates=rates)
    assert sorted(os.listdir(t.ckpt_dir)) == want
    for f in want:
        assert sorted(load_checkpoint(os.path.join(t.ckpt_dir, f))) == rc.CHECKPOINT_KEYS, f
    # --save_state adds the one file and changes no other; --stop_after_epoch ends the run after that many epochs
    s, _ = _scripted_run(tmp_path / "state", ["--save_state"], rates=rates)
    assert sorted(os.listdir(s.ckpt_dir)) == sorted(want + ["train_state.pth"])
    for f in want:
        assert sorted(load_checkpoint(os.path.join(s.ckpt_dir, f))) == rc.CHECKPOINT_KEYS, f
    k, _ = _scripted_run(tmp_path / "stop", ["--stop_after_epoch", "4"], rates=rates)
    assert sorted(os.listdir(k.ckpt_dir)) == rc.parent_listing(range(4), rates[:4], 2)


def test_scripted_resume_walks_the_same_directory_as_the_straight_run(tmp_path):
    """Trainer.fit stopped after four scripted epochs and continued from the state file: listing, best values and the
    returned pair are those of the run that went straight through."""
    from lcrec_amd import main as cli
    from lcrec_amd import train_state
    from lcrec_amd import trainer as tr_mod
    rates = (0.5, 0.3, 0.4, 0.2, 0.6, 0.1)
    s, _ = _scripted_run(tmp_path / "s", ["--save_state"], rates=rates)
    r1, args = _scripted_run(tmp_path / "r", ["--save_state", "--stop_after_epoch", "4"], rates=rates)
    state = train_state.load(os.path.join(r1.ckpt_dir, train_state.FILE_NAME))
    assert state["epoch"] == 3

    class Scripted(tr_mod.Trainer):
        def _train_epoch(self, data, epoch_idx):
            return 10.0 - epoch_idx, 5.0 - epoch_idx

        def _valid_epoch(self, data):
            self._evals = getattr(self, "_evals", 0) + 1
            return rates[self.start_epoch + self._evals - 1]
    args.stop_after_epoch = None
    r2 = Scripted(args, cli.build_model(args, rc.WIDTH), 3, run_dir=r1.ckpt_dir, data_shape=(rc.ROWS, rc.WIDTH))
    train_state.restore(r2, state)
    logging.disable(logging.CRITICAL)
    try:
        best = r2.fit(None)
    finally:
        logging.disable(logging.NOTSET)
    assert best == (s.best_loss, s.best_collision_rate)
    assert sorted(os.listdir(r2.ckpt_dir)) == sorted(os.listdir(s.ckpt_dir))
    assert os.listdir(tmp_path / "r") == [os.path.basename(r1.ckpt_dir)]              # no second time-stamped folder
    final = train_state.load(os.path.join(r2.ckpt_dir, train_state.FILE_NAME))
    assert final["epoch"] == 5 and final["keeper"] == train_state.load(os.path.join(s.ckpt_dir, train_state.FILE_NAME))["keeper"]
