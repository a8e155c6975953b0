"""Decode pass -- the tuples of an `.index.json` back to embeddings, and what they cost in reconstruction loss.  Beyond the
reference, whose decoder runs only inside a training step (index/models/rqvae.py:57-66).

    python -m lcrec_amd.decode_indices --ckpt_path CKPT.pth --index_file X.index.json [--data_path ...] [--output RECON.npy]
                                       [--report OUT.json] [--no_data]

audit_indices prices a file's tuples in latent space (the squared norm of the last residual).  The quantity the training log prints,
and the one a checkpoint is selected on, is the reconstruction loss: the decoder's output against the item's embedding.  This command
sends the file's tuples through the checkpoint's quantiser tables and decoder (ops.decode_tuples; include/lcrec.h,
lcrec_decode_tuples, states the rule), writes the reconstruction if asked to, and -- given the data the file was written from --
compares every item's error with that of the greedy tuples of the same row (ops.encode_assign, then the same decode).

What runs where: per host chunk of 2^20 rows one ops.decode_tuples of the file's tuples and, with the data, one ops.encode_assign
and one more ops.decode_tuples.  The per-item errors come to the host and every aggregate is a numpy float64 sum there, so the
report is a plain function of exact arrays.  audit_indices --recon puts the same dictionary under the key `recon` of its report.
"""
import argparse
import json
import logging
import os

import numpy as np
import torch

from . import ops
from .checkpoint import load_checkpoint
from .datasets import EmbDataset
from .generate_indices import build_model_from_args, load_index_json

CHUNK_ROWS = 1 << 20
WORST = 10
log = logging.getLogger(__name__)


def _refuse_torchrun():
    from . import dist as ldist
    if ldist.current().enabled or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise ValueError("the decode pass under torchrun is not supported: run it in a single process")


def build_recon_report(err_file, err_greedy, held, greedy, flags, in_dim, loss_type, first_item=0):
    """The report dict from the exact per-item arrays (host, numpy): err_file / err_greedy float32 [n] (every item's reconstruction
    error under the file's and under the greedy tuple), held / greedy int64 [n, L], flags int [n] (bit l: the file's code of
    level l was out of range and clamped).  recon_* are the trainer's reconstruction loss: the mean over all n * in_dim elements,
    summed in float64.  Every float is a float64 aggregate; every count an int."""
    ef, eg = np.asarray(err_file).astype(np.float64), np.asarray(err_greedy).astype(np.float64)
    n = int(ef.shape[0])
    count = float(n) * float(in_dim)
    rf = float(ef.sum() / count) if n else 0.0
    rg = float(eg.sum() / count) if n else 0.0
    added = ef - eg
    order_key = np.where(np.isnan(added), -np.inf, added)
    # by err_file - err_greedy descending, a tie to the lower id: everything at or above the WORST-th largest value, sorted
    near = np.flatnonzero(order_key >= np.partition(order_key, n - WORST)[n - WORST]) if n > WORST else np.arange(n)
    order = near[np.lexsort((near, -order_key[near]))][:WORST]
    return {"items": n, "in_dim": int(in_dim), "loss_type": str(loss_type), "recon_file": rf, "recon_greedy": rg,
            "recon_added_rel": rf / rg - 1.0 if rg > 0 else 0.0,
            "moved_items": int((np.asarray(held) != np.asarray(greedy)).any(1).sum()) if n else 0,
            "clamped_items": int((np.asarray(flags) != 0).sum()),
            "worst": [{"item": int(i) + int(first_item), "tuple": [int(v) for v in held[i]], "greedy_tuple": [int(v) for v in greedy[i]],
                       "err_file": float(ef[i]), "err_greedy": float(eg[i])} for i in order]}


def summary(rep):
    """The report in a few lines of text."""
    lines = [f"decode pass: {rep['items']} items of {rep['in_dim']} dimensions"]
    if "recon_file" in rep:
        lines.append(f"  reconstruction loss ({rep['loss_type']}): file {rep['recon_file']:.6g}, greedy tuples {rep['recon_greedy']:.6g} "
                     f"({100.0 * rep['recon_added_rel']:+.4g} %); {rep['moved_items']} items hold another tuple than their greedy one")
    if rep.get("clamped_items"):
        lines.append(f"  {rep['clamped_items']} items hold a code outside their level's range (counted as the nearest valid code)")
    return lines


def _open_output(path, n, w):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    return np.lib.format.open_memmap(path, mode="w+", dtype=np.float32, shape=(n, w))


@torch.no_grad()
def recon_for(model, data, held_host, device, output=None, first_item=0):
    """The report for tuples held_host (int64 [n, L], host) against the rows of `data` (an EmbDataset of n rows), on `model`
    (on `device`, eval mode).  output: a path, the fp32 reconstruction of the file's tuples is streamed into a memory-mapped .npy."""
    n, w = len(data), data.dim
    Ws, bs, scs, shs = model.encoder.folded()
    dWs, dbs, dscs, dshs = model.decoder.folded()
    flat, ks = ops.flatten_codebooks([q.embedding.weight.detach() for q in model.rq.vq_layers])
    l1 = model.loss_type == "l1"
    sink = _open_output(output, n, w) if output else None
    ef, eg, fl, gr = [], [], [], []
    for lo in range(0, n, CHUNK_ROWS):
        hi = min(n, lo + CHUNK_ROWS)
        x = data.to_device(device, rows=(lo, hi))
        held = torch.from_numpy(held_host[lo:hi]).to(device)
        mine = ops.decode_tuples(held, flat, ks, dWs, dbs, dscs, dshs, x=x, l1=l1, want_out=sink is not None)
        greedy = ops.encode_assign(x, Ws, bs, flat, ks, scs, shs)[0]
        theirs = ops.decode_tuples(greedy, flat, ks, dWs, dbs, dscs, dshs, x=x, l1=l1, want_out=False)
        if sink is not None:
            sink[lo:hi] = mine["out"].cpu().numpy()
        ef.append(mine["err"].cpu().numpy())
        fl.append(mine["flags"].cpu().numpy())
        eg.append(theirs["err"].cpu().numpy())
        gr.append(greedy.cpu().numpy())
    if sink is not None:
        sink.flush()
        del sink
    L = len(ks)
    cat = lambda parts, empty: np.concatenate(parts) if parts else empty
    return build_recon_report(cat(ef, np.zeros(0, np.float32)), cat(eg, np.zeros(0, np.float32)), held_host,
                              cat(gr, np.zeros((0, L), np.int64)), cat(fl, np.zeros(0, np.int32)), w, model.loss_type,
                              first_item=first_item)


@torch.no_grad()
def decode(ckpt_path, index_file, device="cuda:0", data_path=None, output=None, no_data=False, trust_checkpoint=False):
    """The report dict (build_recon_report names its keys; with no_data only items, in_dim, loss_type and clamped_items) of
    `index_file` against the checkpoint and its data file.  ValueError: under torchrun; a file the reader refuses (a level count or
    a code that does not go with the checkpoint); a file whose item count is not the data's row count."""
    _refuse_torchrun()
    ckpt = load_checkpoint(ckpt_path, trust=trust_checkpoint)
    args = ckpt["args"]
    dev = torch.device(device)
    if no_data:
        sd = ckpt["state_dict"]
        in_dim = int(sd["encoder.mlp_layers.1.weight"].shape[1])
        data = None
    else:
        data = EmbDataset(data_path or args.data_path, mmap=str(device).startswith("cuda"))
        in_dim = data.dim
    model = build_model_from_args(args, in_dim)
    model.load_state_dict(ckpt["state_dict"])
    ks = [int(q.embedding.weight.shape[0]) for q in model.rq.vq_layers]
    held_host = load_index_json(index_file, ks)
    if data is not None and held_host.shape[0] != len(data):
        raise ValueError(f"{index_file} holds {held_host.shape[0]} items but the data file {len(data)} rows: an index file is decoded "
                         "against the embeddings it was written from")
    model = model.to(dev).eval()
    if data is not None:
        return recon_for(model, data, held_host, dev, output=output)
    n = held_host.shape[0]
    dWs, dbs, dscs, dshs = model.decoder.folded()
    flat, ks = ops.flatten_codebooks([q.embedding.weight.detach() for q in model.rq.vq_layers])
    sink = _open_output(output, n, in_dim) if output else None
    clamped = 0
    for lo in range(0, n, CHUNK_ROWS):
        held = torch.from_numpy(held_host[lo:lo + CHUNK_ROWS]).to(dev)
        res = ops.decode_tuples(held, flat, ks, dWs, dbs, dscs, dshs, want_out=sink is not None, want_xq=sink is None)
        clamped += int((res["flags"] != 0).sum())
        if sink is not None:
            sink[lo:lo + CHUNK_ROWS] = res["out"].cpu().numpy()
    if sink is not None:
        sink.flush()
        del sink
    return {"items": int(n), "in_dim": int(in_dim), "loss_type": str(model.loss_type), "clamped_items": clamped}


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Decode an .index.json through the RQ-VAE checkpoint it was written from")
    ap.add_argument("--ckpt_path", type=str, required=True)
    ap.add_argument("--index_file", type=str, required=True)
    ap.add_argument("--data_path", type=str, default=None, help="override the data path stored in the checkpoint")
    ap.add_argument("--output", type=str, default=None, metavar="RECON.npy", help="write the fp32 reconstruction [items, in_dim]")
    ap.add_argument("--report", type=str, default=None, metavar="OUT.json", help="write the report as JSON")
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--no_data", action="store_true", help="decode only: no data file is read and no error is reported")
    ap.add_argument("--trust_checkpoint", action="store_true",
                    help="load the checkpoint with the unrestricted unpickler (executes code from the file)")
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    rep = decode(a.ckpt_path, a.index_file, device=a.device, data_path=a.data_path, output=a.output, no_data=a.no_data,
                 trust_checkpoint=a.trust_checkpoint)
    for line in summary(rep):
        print(line)
    if a.report:
        os.makedirs(os.path.dirname(os.path.abspath(a.report)), exist_ok=True)
        with open(a.report, "w") as fp:
            json.dump(rep, fp)
    return rep


if __name__ == "__main__":
    main()
