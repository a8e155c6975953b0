"""Index audit -- what every tuple of an `.index.json` costs, code by code.  Beyond the reference, whose
index/generate_indices.py:131-136 prints a collision rate and nothing else.

    python -m lcrec_amd.audit_indices --ckpt_path CKPT.pth --index_file X.index.json [--data_path ...] [--report OUT.json]

The conflict rounds (Sinkhorn) and the opt-in passes of generate_indices (--finish nearest_free, --extend, --spill) deliberately
give some items a code that is not their nearest one.  This command walks the file's tuples through the checkpoint's quantiser
(ops.rq_audit; include/lcrec.h, lcrec_rq_audit, states the rule) and reports how many items sit on a non-nearest code and at
which level, how far down the distance ranking their code is, and how much quantisation error that added over the greedy tuples
of pass 1.  It also tells a file that was not written from the checkpoint at all: no pass of this project moves a code above the
last two levels, so an item that leaves the model's own path earlier, and is no near-tie there, cannot have come from it.

What runs where: per chunk of 2^20 rows one ops.encode_assign (the greedy tuples, the latents, pass 1's near-tie flags) and two
ops.rq_audit calls on those latents (the file's tuples; the greedy tuples, for their error).  The per-item arrays come to the host
and every aggregate is formed there in numpy float64, so the report is a plain function of exact arrays.
generate_indices --audit builds the same report from the latents and the greedy tuples its pass 1 already has (report_for).
"""
import argparse
import json
import logging
import os

import numpy as np
import torch

from . import ops
from .generate_indices import load_index_json, open_run

CHUNK_ROWS = 1 << 20
WORST = 10
log = logging.getLogger(__name__)


def _refuse_torchrun():
    from . import dist as ldist
    if ldist.current().enabled or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise ValueError("the index audit under torchrun is not supported: run it in a single process")


@torch.no_grad()
def audit_chunk(flat, ks, latent, greedy, held):
    """Both ops.rq_audit calls of one chunk, brought to the host: dict of numpy arrays rank int32 [n, L], d_held / d_best
    float32 [n, L], flags int32 [n], err_file / err_greedy float32 [n].  latent float32 [n, e], greedy / held int64 [n, L], all
    on the device."""
    mine = ops.rq_audit(latent, flat, ks, held)
    theirs = ops.rq_audit(latent, flat, ks, greedy)
    out = {k: mine[k].cpu().numpy() for k in ("rank", "d_held", "d_best", "flags")}
    out["err_file"] = mine["err"].cpu().numpy()
    out["err_greedy"] = theirs["err"].cpu().numpy()
    return out


def _joined(parts, L):
    """audit_chunk's dicts of consecutive chunks as one (no chunk: the empty arrays)"""
    if parts:
        return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    return {"rank": np.zeros((0, L), np.int32), "d_held": np.zeros((0, L), np.float32), "d_best": np.zeros((0, L), np.float32),
            "flags": np.zeros(0, np.int32), "err_file": np.zeros(0, np.float32), "err_greedy": np.zeros(0, np.float32)}


def build_report(per, ks, held, greedy, neartie, unique, max_count, first_item=0):
    """The report dict from the exact per-item arrays (host, numpy): `per` as audit_chunk returns it for all items, held / greedy
    int64 [n, L], neartie int [n] (pass 1's near-tie flags, bit l = level l), unique / max_count from ops.collision_groups on the
    held tuples; first_item: the item id of row 0 (generate --extend audits the new rows only), added to the ids in `worst`.
    Every float is a float64 aggregate; every count an int."""
    rank = per["rank"].astype(np.int64)
    n, L = held.shape
    ks = [int(k) for k in ks]
    rep = {"items": int(n), "levels": int(L), "codes": ks,
           "distinct_tuples": int(unique), "colliding_items": int(n - unique), "max_conflicts": int(max_count),
           "collision_rate": (n - unique) / n if n else 0.0,
           "clamped_items": int((per["flags"] != 0).sum())}
    off = rank > 0
    diverged = off.any(1)
    first = np.where(diverged, off.argmax(1), L) if n else np.zeros(0, dtype=np.int64)
    rep["greedy_items"] = int(n - diverged.sum())
    rep["first_divergence"] = [int((first == l).sum()) for l in range(L)]
    early = first < max(L - 2, 0)                          # no pass of this project moves a code above the last two levels
    rep["early_divergence"] = int(early.sum())
    tie_bit = (np.asarray(neartie).astype(np.int64) >> np.minimum(first, L - 1)) & 1 if n else np.zeros(0, dtype=np.int64)
    rep["early_divergence_neartie"] = int((early & (tie_bit != 0)).sum())
    dh, db = per["d_held"].astype(np.float64), per["d_best"].astype(np.float64)
    clamped = np.clip(held, 0, np.asarray(ks, dtype=np.int64)[None, :] - 1)
    rep.update(rank0_items=[], rank_max=[], rank_mean=[], regret_mean=[], codes_used=[])
    for l in range(L):
        rep["rank0_items"].append(int((rank[:, l] == 0).sum()))
        rep["rank_max"].append(int(rank[:, l].max()) if n else 0)
        rep["rank_mean"].append(float(rank[:, l].mean()) if n else 0.0)
        ok = np.isfinite(dh[:, l]) & np.isfinite(db[:, l])
        rep["regret_mean"].append(float((dh[ok, l] - db[ok, l]).mean()) if ok.any() else 0.0)
        rep["codes_used"].append(int(np.count_nonzero(np.bincount(clamped[:, l], minlength=ks[l]))))
    ef, eg = per["err_file"].astype(np.float64), per["err_greedy"].astype(np.float64)
    ok = np.isfinite(ef) & np.isfinite(eg)
    rep["err_file_mean"] = float(ef[ok].mean()) if ok.any() else 0.0
    rep["err_greedy_mean"] = float(eg[ok].mean()) if ok.any() else 0.0
    moved = diverged & ok
    rep["err_added_mean_diverged"] = float((ef[moved] - eg[moved]).mean()) if moved.any() else 0.0
    added = np.where(ok, ef - eg, -np.inf)
    # by err_file - err_greedy descending, a tie to the lower id: everything at or above the WORST-th largest value, sorted
    near = np.flatnonzero(added >= np.partition(added, n - WORST)[n - WORST]) if n > WORST else np.arange(n)
    order = near[np.lexsort((near, -added[near]))][:WORST]
    rep["worst"] = [{"item": int(i) + int(first_item), "tuple": [int(v) for v in held[i]], "greedy_tuple": [int(v) for v in greedy[i]],
                     "ranks": [int(v) for v in rank[i]], "err_file": float(ef[i]), "err_greedy": float(eg[i])} for i in order]
    return rep


def summary(rep):
    """The report in a few lines of text."""
    n, L = rep["items"], rep["levels"]
    lines = [f"index audit: {n} items, {L} levels of {rep['codes']} codes; {rep['distinct_tuples']} distinct tuples, "
             f"{rep['colliding_items']} colliding items (rate {rep['collision_rate']:.6g}, at most {rep['max_conflicts']} on one tuple)",
             f"  on the model's own greedy path: {rep['greedy_items']} items; the others leave it first at level "
             + ", ".join(f"{l}: {c}" for l, c in enumerate(rep["first_divergence"]))]
    for l in range(L):
        lines.append(f"  level {l}: {rep['rank0_items'][l]} items on their nearest code, rank mean {rep['rank_mean'][l]:.4g} max "
                     f"{rep['rank_max'][l]}, mean distance regret {rep['regret_mean'][l]:.6g}, {rep['codes_used'][l]} of "
                     f"{rep['codes'][l]} codes used")
    ratio = rep["err_file_mean"] / rep["err_greedy_mean"] - 1.0 if rep["err_greedy_mean"] > 0 else 0.0
    lines.append(f"  quantisation error (squared norm of the last residual): file mean {rep['err_file_mean']:.6g}, greedy mean "
                 f"{rep['err_greedy_mean']:.6g} ({100.0 * ratio:+.4g} %); the items off the greedy path carry "
                 f"{rep['err_added_mean_diverged']:.6g} more each on average")
    if rep["clamped_items"]:
        lines.append(f"  {rep['clamped_items']} items hold a code outside their level's range (counted as the nearest valid code)")
    return lines


def warn_if_foreign(rep):
    """The one condition under which the file cannot have been written from this checkpoint."""
    foreign = rep["early_divergence"] - rep["early_divergence_neartie"]
    if foreign > 0:
        log.warning("%d items leave the model's own path before the last two levels and are no near-ties: the file was probably "
                    "not written from this checkpoint", foreign)
    return foreign


@torch.no_grad()
def report_for(flat, ks, latent, greedy, neartie, held, first_item=0):
    """The report for tuples `held` (int64 [n, L], device) given what pass 1 computed for the same items: latent float32 [n, e],
    greedy int64 [n, L], neartie int32 [n] (all on the device); flat / ks: the codebooks as ops.flatten_codebooks returns them;
    first_item: the item id of row 0."""
    n, L = held.shape
    parts = [audit_chunk(flat, ks, latent[lo:lo + CHUNK_ROWS], greedy[lo:lo + CHUNK_ROWS].contiguous(),
                         held[lo:lo + CHUNK_ROWS].contiguous()) for lo in range(0, n, CHUNK_ROWS)]
    per = _joined(parts, L)
    found = ops.collision_groups(held.contiguous(), ks, want_groups=False) if n else {"unique": 0, "max_count": 0}
    return build_report(per, ks, held.cpu().numpy(), greedy.cpu().numpy(), neartie.cpu().numpy(), found["unique"], found["max_count"],
                        first_item=first_item)


@torch.no_grad()
def audit(ckpt_path, index_file, device="cuda:0", data_path=None, trust_checkpoint=False, recon=False):
    """The report dict (build_report names its keys) of `index_file` against the checkpoint and its data file.  ValueError: under
    torchrun; a file the reader refuses (a level count or a code that does not go with the checkpoint); a file whose item count
    is not the data's row count.  recon: the report also holds, under the key "recon", what the tuples cost in reconstruction loss
    (decode_indices.recon_for: the file's and the greedy tuples through the decoder, against the embeddings)."""
    _refuse_torchrun()
    _, data, model = open_run(ckpt_path, data_path, device, trust=trust_checkpoint)
    ks = [int(q.embedding.weight.shape[0]) for q in model.rq.vq_layers]
    held_host = load_index_json(index_file, ks)
    n = len(data)
    if held_host.shape[0] != n:
        raise ValueError(f"{index_file} holds {held_host.shape[0]} items but the data file {n} rows: an index file is audited "
                         "against the embeddings it was written from")
    dev = torch.device(device)
    model = model.to(dev).eval()
    Ws, bs, scs, shs = model.encoder.folded()
    flat, ks = ops.flatten_codebooks([q.embedding.weight.detach() for q in model.rq.vq_layers])
    held = torch.from_numpy(held_host).to(dev)
    parts, greedy_parts, tie_parts = [], [], []
    for lo in range(0, n, CHUNK_ROWS):
        hi = min(n, lo + CHUNK_ROWS)
        a = {}
        greedy, latent, _, _ = ops.encode_assign(data.to_device(dev, rows=(lo, hi)), Ws, bs, flat, ks, scs, shs, want_latent=True,
                                                 audit=a, tie_tau=ops.NEARTIE_TAU)
        parts.append(audit_chunk(flat, ks, latent, greedy, held[lo:hi]))
        greedy_parts.append(greedy.cpu().numpy())
        tie_parts.append(a["neartie"].cpu().numpy())
    L = len(ks)
    per = _joined(parts, L)
    greedy_host = np.concatenate(greedy_parts) if parts else np.zeros((0, L), np.int64)
    neartie = np.concatenate(tie_parts) if parts else np.zeros(0, np.int32)
    found = ops.collision_groups(held, ks, want_groups=False) if n else {"unique": 0, "max_count": 0}
    rep = build_report(per, ks, held_host, greedy_host, neartie, found["unique"], found["max_count"])
    warn_if_foreign(rep)
    if recon:
        from . import decode_indices
        rep["recon"] = decode_indices.recon_for(model, data, held_host, dev)
    return rep


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Audit an .index.json against the RQ-VAE checkpoint it was written from")
    ap.add_argument("--ckpt_path", type=str, required=True)
    ap.add_argument("--index_file", type=str, required=True)
    ap.add_argument("--data_path", type=str, default=None, help="override the data path stored in the checkpoint")
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--report", type=str, default=None, metavar="OUT.json", help="write the report as JSON")
    ap.add_argument("--recon", action="store_true",
                    help="also report what the tuples cost in reconstruction loss (the decode pass), under the key `recon`")
    ap.add_argument("--trust_checkpoint", action="store_true",
                    help="load the checkpoint with the unrestricted unpickler (executes code from the file)")
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    rep = audit(a.ckpt_path, a.index_file, device=a.device, data_path=a.data_path, trust_checkpoint=a.trust_checkpoint, recon=a.recon)
    for line in summary(rep):
        print(line)
    if a.recon:
        from . import decode_indices
        for line in decode_indices.summary(rep["recon"]):
            print(line)
    if a.report:
        os.makedirs(os.path.dirname(os.path.abspath(a.report)), exist_ok=True)
        with open(a.report, "w") as fp:
            json.dump(rep, fp)
    return rep


if __name__ == "__main__":
    main()
