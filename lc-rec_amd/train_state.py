"""`<run dir>/train_state.pth`: everything a training run needs, beyond a checkpoint's six keys, to go on after an
epoch exactly as if it had never stopped (main.py --save_state / --resume), and the checks of --init_from.

The checkpoints keep the reference's layout; this file is ours.  It is read with the restricted unpickler of
checkpoint.py, so it holds tensors, plain containers, numbers, strings and the `args` Namespace only: generator
states are uint8 tensors, numpy's Mersenne-Twister keys an int64 tensor, Python's a list of ints.

What a training step reads and where it is kept:
  parameters, buffers (EMA statistics, BatchNorm running statistics)   state_dict
  moments, `step` entries                                               optimizer -- the engine's device step counter, which
                                                                        drives the schedule and the dropout masks, is rebuilt
                                                                        from `step` (SGD: from the scheduler's last_epoch)
  the dropout masks' seed                                               dropout_seed (engine) / torch's device generator (autograd)
  per level: initted, step_count (times the dead-code reset), reset draws   levels
  the epoch's permutation                                               torch's CPU generator
"""
import argparse
import copy
import logging
import os
import random

import numpy as np
import torch

from . import _lib
from .checkpoint import load_checkpoint

FORMAT_VERSION = 1
FILE_NAME = "train_state.pth"
log = logging.getLogger(__name__)

# what --resume may say differently from the run it continues; everything else must agree with the saved args
RESUME_MAY_DIFFER = ("epochs", "device", "data_path", "save_limit", "stop_after_epoch")
_NOT_CONFIGURATION = ("resume", "init_from", "save_state")
# --init_from: the fields of the file's args that shape the state dict (the input width is read off the weights)
ARCHITECTURE_FIELDS = ("num_emb_list", "e_dim", "layers", "bn")


# ------------------------------------------------------------------ generators
def _numpy_state():
    name, keys, pos, has_gauss, cached = np.random.get_state()
    return {"name": str(name), "keys": torch.from_numpy(keys.astype(np.int64)), "pos": int(pos),
            "has_gauss": int(has_gauss), "cached_gaussian": float(cached)}


def _set_numpy_state(s):
    np.random.set_state((s["name"], s["keys"].numpy().astype(np.uint32), int(s["pos"]), int(s["has_gauss"]),
                         float(s["cached_gaussian"])))


def _python_state():
    version, words, gauss_next = random.getstate()
    return {"version": int(version), "words": [int(w) for w in words], "gauss_next": gauss_next}


def _set_python_state(s):
    random.setstate((int(s["version"]), tuple(int(w) for w in s["words"]), s["gauss_next"]))


def generator_states(device):
    device = torch.device(device)
    return {"torch_cpu": torch.get_rng_state().clone(),
            "torch_device": torch.cuda.get_rng_state(device).clone() if device.type == "cuda" else None,
            "numpy": _numpy_state(), "python": _python_state()}


def restore_generators(states, device, skip=()):
    """`skip`: names left as they are (tests show what each one is needed for)."""
    device = torch.device(device)
    if "python" not in skip:
        _set_python_state(states["python"])
    if "numpy" not in skip:
        _set_numpy_state(states["numpy"])
    if "torch_device" not in skip and states["torch_device"] is not None and device.type == "cuda":
        torch.cuda.set_rng_state(states["torch_device"], device)
    if "torch_cpu" not in skip:
        torch.set_rng_state(states["torch_cpu"])


# ------------------------------------------------------------------ the file
def keeper_entries(keeper):
    """The CheckpointKeeper's two lists as [-collision rate, file name relative to the run directory] pairs, in the
    lists' own order (`best` is a heap: its order is part of it)."""
    keep = lambda entries: [[float(neg), os.path.basename(path)] for neg, path in entries]
    return {"best": keep(keeper.best), "newest": keep(keeper.newest)}


def restore_keeper(keeper, entries, run_dir):
    at = lambda pairs: [(float(neg), os.path.join(run_dir, name)) for neg, name in pairs]
    keeper.best, keeper.newest = at(entries["best"]), at(entries["newest"])


def capture(trainer, epoch):
    """The state after epoch index `epoch` has finished (with its evaluation, if it had one)."""
    levels = []
    for q in trainer.model.rq.vq_layers:
        gen = getattr(q, "reset_generator", None)
        levels.append({"initted": bool(q.initted), "step_count": int(q.step_count),
                       "reset_generator": None if gen is None else gen.get_state().clone()})
    engine = trainer.engine
    seed, on_engine = trainer.dropout_seed, trainer.resumed_engine       # (a resumed run that has not stepped yet)
    if trainer._engine_decided:
        on_engine = engine is not None
        seed = int(engine.dropout_seed.item()) if engine is not None and engine.dropout_seed is not None else None
    rows, width = trainer.data_shape if trainer.data_shape is not None else (None, None)
    return {
        "format": FORMAT_VERSION,
        "abi": int(_lib.ABI_VERSION),
        "args": trainer.args,
        "epoch": int(epoch),
        "state_dict": trainer.model.state_dict(),                 # (the engine's hooks bring the host's view up to date)
        "optimizer": trainer.optimizer.state_dict(),
        "scheduler_last_epoch": int(trainer.scheduler.last_epoch),
        "best_loss": float(trainer.best_loss),
        "best_collision_rate": float(trainer.best_collision_rate),
        "cur_eval_step": int(trainer.cur_eval_step),
        "keeper": keeper_entries(trainer.keeper),
        "levels": levels,
        "generators": generator_states(trainer.device),
        "dropout_seed": seed,
        "engine": on_engine,
        "world_size": 1 if trainer.dist is None else int(trainer.dist.world_size),
        "data_rows": rows,
        "data_width": width,
    }


def write(run_dir, state):
    """Atomically: a temporary name in the same directory, then os.replace -- a write that dies half way leaves the
    previous file as it was."""
    path = os.path.join(run_dir, FILE_NAME)
    tmp = path + ".tmp"
    torch.save(state, tmp, pickle_protocol=4)
    os.replace(tmp, path)
    return path


def locate(where):
    """--resume's argument: a run directory or the path of its train_state.pth."""
    path = os.path.join(where, FILE_NAME) if os.path.isdir(where) else where
    if not os.path.isfile(path):
        raise FileNotFoundError(f"--resume: no state file at {path} (was the run started with --save_state?)")
    return path


def load(path):
    state = load_checkpoint(path)
    version = state.get("format") if isinstance(state, dict) else None
    if version != FORMAT_VERSION:
        raise ValueError(f"{path}: state file format version {version!r} is unknown to this build (it reads version "
                         f"{FORMAT_VERSION}); a checkpoint is not a state file")
    if state["abi"] != int(_lib.ABI_VERSION):
        log.warning("%s was written with library ABI %s, this build has %s: the continuation may not reproduce the "
                    "uninterrupted run bit for bit", path, state["abi"], _lib.ABI_VERSION)
    return state


# ------------------------------------------------------------------ --resume: configuration
def resume_args(saved, cli, given):
    """The configuration of a resumed run: the saved args, with what RESUME_MAY_DIFFER allows taken from the command line.
    `cli`: the parsed command line; `given`: the dests the command line set itself.  A flag given with another value than
    the saved one is an error naming the flag and both values."""
    args = copy.deepcopy(saved)
    for key in sorted(given):
        if key in _NOT_CONFIGURATION:
            continue
        now = getattr(cli, key)
        if key in RESUME_MAY_DIFFER:
            setattr(args, key, now)
            continue
        was = getattr(saved, key, None)
        if now != was:
            raise ValueError(f"--resume: --{key} is {now!r} on the command line and {was!r} in the saved run; only "
                             + ", ".join("--" + k for k in RESUME_MAY_DIFFER) + " may change")
    if "stop_after_epoch" not in given:
        args.stop_after_epoch = None                       # (the stop that ended the run before is not this run's)
    args.resume, args.init_from, args.save_state = cli.resume, None, True
    return args


def check_data(state, rows, width):
    if (state["data_rows"], state["data_width"]) != (rows, width):
        raise ValueError(f"--resume: the data file has {rows} rows x {width} columns, the saved run had "
                         f"{state['data_rows']} x {state['data_width']} (for a grown file use --init_from)")


def check_world(state, world_size):
    if int(state["world_size"]) != int(world_size):
        raise ValueError(f"--resume: world size {world_size}, the saved run had {state['world_size']}")


def refuse_ranks(args, world_size):
    if world_size > 1:
        for flag in ("resume", "save_state"):
            if getattr(args, flag, None):
                raise ValueError(f"--{flag} under torchrun is not supported: run it in a single process")


# ------------------------------------------------------------------ --resume: state
def restore(trainer, state, skip_generators=()):
    """Put `state` into a freshly built Trainer, in an order that lets nothing draw from a generator between here and
    the first step: model, level flags, reset generators, optimizer, scheduler, keeper, best values, generators."""
    trainer.model.load_state_dict(state["state_dict"])
    levels = list(trainer.model.rq.vq_layers)
    if len(levels) != len(state["levels"]):
        raise ValueError(f"--resume: {len(levels)} quantiser levels, the saved run had {len(state['levels'])}")
    for q, s in zip(levels, state["levels"]):
        q.initted, q.step_count = bool(s["initted"]), int(s["step_count"])
    for l, (q, s) in enumerate(zip(levels, state["levels"])):
        gen = getattr(q, "reset_generator", None)
        if (gen is None) != (s["reset_generator"] is None):
            raise ValueError(f"--resume: level {l} has {'a' if gen is not None else 'no'} reset generator, the saved run "
                             f"had {'one' if s['reset_generator'] is not None else 'none'}")
        if gen is not None:
            gen.set_state(s["reset_generator"])
    opt = trainer.optimizer
    # (Adagrad's `step` entries live where Trainer._build_optimizer put them; load_state_dict leaves a `step` where the file's was)
    homes = {p: st["step"].device for p, st in opt.state.items() if torch.is_tensor(st.get("step"))}
    opt.load_state_dict(state["optimizer"])
    for p, dev in homes.items():
        if torch.is_tensor(opt.state[p].get("step")):
            opt.state[p]["step"] = opt.state[p]["step"].to(dev)
    sch = trainer.scheduler
    sch.last_epoch = int(state["scheduler_last_epoch"])
    sch._step_count = sch.last_epoch + 1
    # the learning rate of the step counter under THIS run's schedule (a larger --epochs moves a linear decay's end)
    lrs = [base * lmbda(sch.last_epoch) for base, lmbda in zip(sch.base_lrs, sch.lr_lambdas)]
    for group, lr in zip(opt.param_groups, lrs):
        group["lr"] = lr
    sch._last_lr = lrs
    restore_keeper(trainer.keeper, state["keeper"], trainer.ckpt_dir)
    trainer.best_loss = float(state["best_loss"])
    trainer.best_collision_rate = float(state["best_collision_rate"])
    trainer.cur_eval_step = int(state["cur_eval_step"])
    trainer.start_epoch = int(state["epoch"]) + 1
    trainer.dropout_seed = state["dropout_seed"]
    trainer.resumed_engine = state["engine"]
    restore_generators(state["generators"], trainer.device, skip=skip_generators)


# ------------------------------------------------------------------ --init_from
def input_width(state_dict):
    """in_features of the encoder's first Linear."""
    first = None
    for key, v in state_dict.items():
        parts = key.split(".")
        if key.startswith("encoder.mlp_layers.") and parts[-1] == "weight" and v.dim() == 2:
            if first is None or int(parts[2]) < first[0]:
                first = (int(parts[2]), int(v.shape[1]))
    if first is None:
        raise ValueError("--init_from: the file's state_dict has no encoder weights")
    return first[1]


def init_weights(path, args, in_dim):
    """The state_dict of a checkpoint or state file for a model built from `args` on `in_dim` columns; any architecture
    field on which the file's args and `args` differ is an error naming it."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"--init_from: no file at {path}")
    ckpt = load_checkpoint(path)
    if not isinstance(ckpt, dict) or "state_dict" not in ckpt or not isinstance(ckpt.get("args"), argparse.Namespace):
        raise ValueError(f"--init_from: {path} is neither a trainer checkpoint nor a state file")
    theirs = ckpt["args"]
    for field in ARCHITECTURE_FIELDS:
        was, now = getattr(theirs, field, None), getattr(args, field, None)
        if isinstance(was, (list, tuple)):
            was, now = list(was), list(now) if isinstance(now, (list, tuple)) else now
        if was != now:
            raise ValueError(f"--init_from: {field} is {now!r} here and {was!r} in {path}")
    width = input_width(ckpt["state_dict"])
    if width != int(in_dim):
        raise ValueError(f"--init_from: input width is {int(in_dim)} here (the data file's columns) and {width} in {path}")
    was, now = getattr(theirs, "ema_decay", None) is not None, getattr(args, "ema_decay", None) is not None
    if was != now:
        raise ValueError(f"--init_from: ema_decay is {'set' if now else 'not set'} here and {'set' if was else 'not set'} "
                         f"in {path} (the EMA buffers are part of the state dict)")
    return ckpt["state_dict"]
