"""Query pass -- which catalogue items an embedding lands on.  Beyond the reference, whose index/ stage has no way back from a tuple
to the items that hold it.

    python -m lcrec_amd.query_indices --ckpt_path CKPT.pth --index_file X.index.json --queries Q.npy [--beam W] [--report OUT.json]
                                      [--device cuda:0] [--trust_checkpoint]

Q.npy holds fp32 rows [q, in_dim] -- a cold-start item, a query -- of the width the checkpoint's encoder takes.  Every row is encoded
(ops.encode_assign), its W best tuples are listed (ops.rq_beam, W in 1, 2, 4, 8), and every tuple is joined against the index file
through the file's prefix trie (IndexTrie.find with longest=True): the ids of the items that hold the tuple where one does, and
otherwise how far the tuple's prefix is shared with the file and how many items lie under that prefix.

What runs where: one ops.trie_build of the file, one ops.encode_assign, one ops.rq_beam and one ops.trie_find of all q * W tuples;
the spans and holders come to the host and the report is a plain function of exact arrays (build_query_report).
"""
import argparse
import json
import logging
import os

import numpy as np
import torch

from . import ops
from .checkpoint import load_checkpoint
from .decode_indices import _refuse_torchrun
from .generate_indices import build_model_from_args, load_index_json
from .trie import IndexTrie

log = logging.getLogger(__name__)


def build_query_report(tuples, err, depth, lo, hi, order, L):
    """The report dict from the exact arrays (host, numpy): tuples int64 [q, W, L] and err float32 [q, W] (ops.rq_beam's; a beam past
    the live count holds -1 codes and is left out), depth int [q, W] (levels of the tuple matched in the file), lo / hi int64 [q, W]
    (the positions of `order` under the deepest matched prefix), order int64 [n] (the trie's).  A beam whose match is exact
    (depth == L) lists the ids of the items that hold its tuple, ascending; any other the number of items under its prefix."""
    tuples, err, depth = np.asarray(tuples), np.asarray(err), np.asarray(depth)
    lo, hi, order = np.asarray(lo), np.asarray(hi), np.asarray(order)
    q, W = err.shape
    live = tuples[:, :, 0] >= 0 if L else np.ones((q, W), dtype=bool)
    exact = live & (depth == L)
    results = []
    for i in range(q):
        beams = []
        for w in range(W):
            if not live[i, w]:
                continue
            one = {"beam": w, "tuple": [int(v) for v in tuples[i, w]], "err": float(err[i, w]), "depth": int(depth[i, w])}
            if exact[i, w]:
                one["items"] = [int(v) for v in order[int(lo[i, w]):int(hi[i, w])]]
            else:
                one["items_under_prefix"] = int(hi[i, w] - lo[i, w])
            beams.append(one)
        results.append(beams)
    return {"queries": int(q), "beam": int(W), "levels": int(L), "items": int(order.shape[0]),
            "exact_beam0": int(exact[:, 0].sum()) if W else 0, "exact_any": int(exact.any(1).sum()) if W else 0,
            "mean_depth": float(depth[live].astype(np.float64).mean()) if live.any() else 0.0, "results": results}


def summary(rep):
    """The report in a few lines of text."""
    return [f"query pass: {rep['queries']} queries, beam {rep['beam']}, against {rep['items']} items of {rep['levels']} levels",
            f"  exact hit on beam 0: {rep['exact_beam0']}; on any beam: {rep['exact_any']}; mean matched depth {rep['mean_depth']:.4g}"]


def _span(trie, node, depth):
    """(lo, hi) of every (node, depth) pair: IndexTrie.span depth by depth"""
    lo, hi = torch.zeros_like(node), torch.zeros_like(node)
    for d in range(trie.L + 1):
        rows = torch.nonzero(depth == d).view(-1)
        if rows.numel():
            lo[rows], hi[rows] = trie.span(node[rows], d)
    return lo, hi


@torch.no_grad()
def query(ckpt_path, index_file, queries, beam=4, device="cuda:0", trust_checkpoint=False):
    """The report dict (build_query_report names its keys) of the rows of the .npy file `queries` against `index_file`.  ValueError:
    under torchrun; a beam width other than 1, 2, 4, 8; a file the reader refuses (a level count or a code that does not go with the
    checkpoint); a query matrix whose width is not the encoder's -- each before the device is touched."""
    _refuse_torchrun()
    if beam not in ops.BEAM_WIDTHS:
        raise ValueError(f"--beam {beam!r}: one of {ops.BEAM_WIDTHS}")
    ckpt = load_checkpoint(ckpt_path, trust=trust_checkpoint)
    args, sd = ckpt["args"], ckpt["state_dict"]
    in_dim = int(sd["encoder.mlp_layers.1.weight"].shape[1])
    x = np.load(queries, mmap_mode="r")
    if x.ndim != 2 or x.shape[1] != in_dim:
        raise ValueError(f"{queries} holds an array of shape {tuple(x.shape)} but the checkpoint's encoder takes rows of {in_dim} floats")
    if x.dtype != np.float32:
        raise ValueError(f"{queries} holds {x.dtype}, not float32")
    model = build_model_from_args(args, in_dim)
    model.load_state_dict(sd)
    ks = [int(q.embedding.weight.shape[0]) for q in model.rq.vq_layers]
    held = load_index_json(index_file, ks)
    dev = torch.device(device)
    model = model.to(dev).eval()
    Ws, bs, scs, shs = model.encoder.folded()
    flat, ks = ops.flatten_codebooks([q.embedding.weight.detach() for q in model.rq.vq_layers])
    L = len(ks)
    trie = IndexTrie.from_indices(torch.from_numpy(held).to(dev), ks)
    xd = torch.from_numpy(np.array(x)).to(dev)                                        # (a copy: the file is mapped read-only)
    _, latent, _, _ = ops.encode_assign(xd, Ws, bs, flat, ks, scs, shs, want_latent=True)
    res = ops.rq_beam(latent, flat, ks, beam)
    node, depth = trie.find(res["tuples"].view(-1, L), L, longest=True)
    lo, hi = _span(trie, node, depth.to(torch.int64))
    shape = (xd.shape[0], beam)
    host = lambda t: t.cpu().numpy()
    return build_query_report(host(res["tuples"]), host(res["err"]), host(depth).reshape(shape), host(lo).reshape(shape),
                              host(hi).reshape(shape), host(trie.order), L)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Which items of an .index.json an embedding lands on, through the RQ-VAE checkpoint")
    ap.add_argument("--ckpt_path", type=str, required=True)
    ap.add_argument("--index_file", type=str, required=True)
    ap.add_argument("--queries", type=str, required=True, metavar="Q.npy", help="fp32 rows [q, in_dim]")
    ap.add_argument("--beam", type=int, default=4, help="tuples listed per query: 1, 2, 4 or 8")
    ap.add_argument("--report", type=str, default=None, metavar="OUT.json", help="write the report as JSON")
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--trust_checkpoint", action="store_true",
                    help="load the checkpoint with the unrestricted unpickler (executes code from the file)")
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    rep = query(a.ckpt_path, a.index_file, a.queries, beam=a.beam, device=a.device, trust_checkpoint=a.trust_checkpoint)
    for line in summary(rep):
        print(line)
    if a.report:
        os.makedirs(os.path.dirname(os.path.abspath(a.report)), exist_ok=True)
        with open(a.report, "w") as fp:
            json.dump(rep, fp)
    return rep


if __name__ == "__main__":
    main()
