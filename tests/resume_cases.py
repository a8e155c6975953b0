"""The shared table of the resume tests (test_resume_host.py, test_gpu_resume.py): one toy problem that reaches every
form of the training step in about a second per run, and the comparison that "the same bits" means.

300 rows x 64 columns in batches of 128: three batches an epoch of 128, 128 and 44 rows -- two graph sizes, one ragged.
Six epochs, evaluated every second one, two of warm-up: a split after epoch index 2 is no evaluation epoch, lies inside
the linear schedule's decay and comes after the warm-up has ended.
"""
import argparse
import os

import numpy as np
import torch

ROWS, WIDTH, SEED = 300, 64, 20240613
EPOCHS, SPLIT = 6, 3
BASE = ["--batch_size", "128", "--layers", "32", "--e_dim", "16", "--num_emb_list", "16", "16", "16", "--no_kmeans_init",
        "--epochs", str(EPOCHS), "--eval_step", "2", "--warmup_epochs", "2"]
LINEAR = ["--lr_scheduler_type", "linear"]

# name -> the flags of the case beyond BASE; every one but (g) trains on the engine, captured
CASES = {
    "a_adamw_bn_sinkhorn": ["--bn", "True", "--sk_epsilons", "0.0", "0.0", "0.003"],
    "b_sgd": ["--learner", "SGD"],
    "c_adagrad": ["--learner", "Adagrad"],
    "d_rmsprop": ["--learner", "RMSprop"],
    "e_dropout": ["--dropout_prob", "0.3"],
    "f_ema_resets": ["--ema_decay", "0.99", "--reset_interval", "3", "--reset_threshold", "0.02", "--reset_seed", "7"],
    "g_autograd_dropout": ["--train_engine", "off", "--dropout_prob", "0.3"],
}
ENGINE_CASES = [c for c in CASES if not c.startswith("g_")]

CHECKPOINT_KEYS = ["args", "best_collision_rate", "best_loss", "epoch", "optimizer", "state_dict"]


def toy_matrix(rows=ROWS, seed=SEED):
    rs = np.random.RandomState(seed)
    centres = rs.standard_normal((24, WIDTH)).astype(np.float32)
    return (centres[rs.randint(0, 24, size=rows)] + 0.1 * rs.standard_normal((rows, WIDTH))).astype(np.float32)


def write_toy(path, rows=ROWS, seed=SEED):
    np.save(path, toy_matrix(rows, seed))
    return path


def parent_listing(eval_epochs, rates, limit):
    """The names a run directory holds after evaluations at `eval_epochs` with collision rates `rates`, by the rule of
    the trainer before the state file existed (reference trainer.py:231-247, written out here, not imported): the two
    best_* files, and the epoch checkpoints that are among the `limit` newest or the `limit` lowest collision rates
    (an earlier file wins a tie: a later one must be strictly better to displace it)."""
    name = lambda e, r: "epoch_%d_collision_%.4f_model.pth" % (e, r)
    newest, best, alive = [], [], set()
    for e, r in zip(eval_epochs, rates):
        f = name(e, r)
        alive.add(f)
        if len(newest) < limit:
            newest.append((r, f))
            best.append((r, f))
            continue
        oldest = newest.pop(0)
        newest.append((r, f))
        worst = max(best, key=lambda t: t[0])
        if r < worst[0]:
            best.remove(worst)
            best.append((r, f))
            if worst not in newest:
                alive.discard(worst[1])
        if oldest not in best:
            alive.discard(oldest[1])
    return sorted(alive | {"best_loss_model.pth", "best_collision_model.pth"})


def differences(a, b, where=""):
    """Where two loaded files differ: tensors by torch.equal (dtype and shape included), everything else by ==; an
    argparse.Namespace (`args`: the runs' command lines differ by design) is not compared."""
    if isinstance(a, argparse.Namespace) and isinstance(b, argparse.Namespace):
        return []
    if type(a) is not type(b):
        return [f"{where}: {type(a).__name__} vs {type(b).__name__}"]
    if torch.is_tensor(a):
        same = a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
        return [] if same else [f"{where}: tensors differ ({a.dtype}{tuple(a.shape)} vs {b.dtype}{tuple(b.shape)})"]
    if isinstance(a, dict):
        if list(a) != list(b):
            return [f"{where}: keys {list(a)} vs {list(b)}"]
        return [d for k in a for d in differences(a[k], b[k], f"{where}.{k}")]
    if isinstance(a, (list, tuple)):
        if len(a) != len(b):
            return [f"{where}: length {len(a)} vs {len(b)}"]
        return [d for i, (x, y) in enumerate(zip(a, b)) for d in differences(x, y, f"{where}[{i}]")]
    return [] if a == b else [f"{where}: {a!r} vs {b!r}"]


def tensors_in(obj):
    if torch.is_tensor(obj):
        return 1
    if isinstance(obj, dict):
        return sum(tensors_in(v) for v in obj.values())
    if isinstance(obj, (list, tuple)):
        return sum(tensors_in(v) for v in obj)
    return 0


def only_run_dir(root):
    runs = os.listdir(root)
    assert len(runs) == 1, runs
    return os.path.join(root, runs[0])
