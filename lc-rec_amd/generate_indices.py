"""Index emission + conflict resolution -- the flow of the reference's index/generate_indices.py
(:51-145), as functions and a small CLI instead of a script with hard-coded paths (:44-49).

    python -m lcrec_amd.generate_indices --ckpt_path CKPT.pth --output_dir DIR [--dataset Games]

Same observable behaviour: pass 1 = get_indices(use_sk=False) over all items (:77-95); levels
0..L-2 forced to hard assignment and the last level's sk_epsilon set to 0.003 if it was 0 (:101-105);
up to 20 rounds in which every group of items sharing a tuple is re-assigned with Sinkhorn on the
last level (:107-128); statistics (:131-136); `{item: ["<a_i>", "<b_j>", ...]}` written with
json.dump's default separators (:138-145) so data.py:38-89 reads it unchanged.

What runs where: pass 1 is one lcrec_encode_assign call; the residual entering the last level is
kept in HBM, so a round is {lcrec_collision_groups -> gather -> ONE batched lcrec_sinkhorn_assign
over all groups -> scatter}: no re-encoding, no per-group forward, no Python string keys.
Groups within a round are independent in the reference too (they are listed before any is
re-assigned), so batching them does not change the result.

Documented divergences from the reference script:
  * its 5-entry prefix list (:83) raises IndexError for L > 5; here prefixes continue <f_..>, <g_..>;
  * --finish nearest_free (off by default; `none` writes the reference's bytes) goes BEYOND the reference: after the rounds every
    item that still shares its tuple gets the nearest free last-level code (finish_collisions);
  * --extend BASE.index.json goes BEYOND the reference too: the data file holds a catalogue that has grown, the items of BASE keep
    their tuples byte for byte, and only the new items are indexed, around them (generate_extended);
  * --spill (off by default) follows either of the two: an item they leave colliding, because its bucket holds more items than the
    last level has codes, takes the next-nearest code one level up and the nearest free last-level code there (spill_collisions);
  * --audit (off by default) goes BEYOND the reference as well: the tuples about to be written are walked through the quantiser again
    and what the moves above cost -- ranks, distance regret, added quantisation error -- is reported (audit_indices.report_for);
  * --beam W (off by default: W = 1) goes BEYOND the reference, which is greedy throughout: pass 1 walks the quantiser with a beam of
    W partial tuples per item (ops.rq_beam) and every item gets the best whole tuple found, or its greedy one where that is better;
    the rounds and the passes above then run on those tuples and their residuals (assign_all);
  * --finish beam (off by default) goes BEYOND the reference and beyond --finish nearest_free, which only ever changes a last code:
    every item that still shares its tuple after the rounds moves to the next-best WHOLE tuple nobody holds, out of a beam of
    --finish_width tuples of its own latent (beam_finish_collisions); nearest_free then runs on what that leaves.  --rounds N sets
    the number of conflict rounds before it (20, the reference's; 0 keeps every item that collides with nobody on its pass-1 tuple);
  * --extend_finish beam (off by default) is that step for --extend: a new item whose pass-1 tuple is taken, by a frozen item or by
    a better new holder, first moves to the next-best whole tuple nobody holds (extend_beam_collisions); the nearest-free pass of
    --extend then runs on what that leaves, and the base's tuples stay byte for byte;
  * it stores tokens in fixed-width numpy unicode arrays (:98-99) which silently truncate a
    replacement longer than anything seen in pass 1; integer tuples are kept here, and a warning is
    logged if a run ever hits that case (the reference's output would be corrupt there).
"""
import argparse
import collections
import json
import logging
import os
import re

import numpy as np
import torch

from . import ops
from .checkpoint import _CKPT_GLOBALS, _CheckpointPickle, load_checkpoint  # noqa: F401  (this module's API since before checkpoint.py)
from .datasets import EmbDataset
from .rqvae import RQVAE

PREFIX = ["<{}_{{}}>".format(chr(ord("a") + i)) for i in range(26)]   # "<a_{}>", "<b_{}>", ... (:83 has a..e)
MAX_ROUNDS = 20                                                        # :110
FINISH_MODES = ("none", "nearest_free", "beam")
FINISH_WIDTHS = (2, 4, 8)
EXTEND_FINISH_MODES = ("nearest_free", "beam")
log = logging.getLogger(__name__)


# ---- the reference's helper API (:18-42), on any sequence of hashable index keys
def check_collision(all_indices_str):
    keys = all_indices_str.tolist() if hasattr(all_indices_str, "tolist") else list(all_indices_str)
    keys = [tuple(k) if isinstance(k, list) else k for k in keys]
    return len(keys) == len(set(keys))


def get_indices_count(all_indices_str):
    counts = collections.defaultdict(int)
    for key in all_indices_str:
        counts[tuple(key) if isinstance(key, list) else key] += 1
    return counts


def get_collision_item(all_indices_str):
    """Groups of item ids sharing a key: first-occurrence order, ids ascending (:29-42)."""
    seen = {}
    for i, key in enumerate(all_indices_str):
        seen.setdefault(tuple(key) if isinstance(key, list) else key, []).append(i)
    return [ids for ids in seen.values() if len(ids) > 1]


def build_model_from_args(args, in_dim):
    """:58-70 -- note beta is NOT forwarded (RQVAE's default 0.25 applies; irrelevant in eval)."""
    return RQVAE(in_dim=in_dim, num_emb_list=args.num_emb_list, e_dim=args.e_dim, layers=args.layers,
                 dropout_prob=args.dropout_prob, bn=args.bn, loss_type=args.loss_type,
                 quant_loss_weight=args.quant_loss_weight, kmeans_init=args.kmeans_init,
                 kmeans_iters=args.kmeans_iters, sk_epsilons=args.sk_epsilons, sk_iters=args.sk_iters,
                 ema_decay=getattr(args, "ema_decay", None), epsilon=getattr(args, "epsilon", 1e-5),
                 reset_threshold=getattr(args, "reset_threshold", 1e-5),
                 reset_interval=getattr(args, "reset_interval", 1000))


@torch.no_grad()
def assign_all(model, data, chunk_rows=1 << 20, audit=None, want_prev=False, latents=None, beam=1, beam_info=None):
    """Pass 1 (:77-95): int64 [N, L] hard indices plus the residual entering the last level.
    audit: optional dict; receives "neartie" (int32 [N], ops.NEARTIE_TAU) -- the near-tie flags of pass 1.
    want_prev: a fourth value is returned, the residual entering level L-2 (L = 2: the latent; L = 1: None) -- spill_collisions'.
    latents: optional list; receives every chunk's latents (float32 [rows, e]) in order -- the index audit's (--audit).
    beam: 1 = the greedy walk, and nothing of the beam path is called.  2, 4 or 8: the returned tuples are the CHOSEN tuples of a beam
    of that width (ops.beam_choose: beam 0's tuple, or the greedy one where it leaves the smaller residual), chunk by chunk on the
    latents the one encoder run produced, and the residuals returned are those of the chosen tuples -- ops.rq_audit walks their
    prefixes idx[:, :L-1] / idx[:, :L-2] as tuples of a shorter quantiser.  beam_info: optional dict; receives "greedy" (a list
    of every chunk's greedy tuples), "changed", "kept_greedy" (item counts) and "err_chosen", "err_greedy" (float64 sums over
    the items on which both errors are finite)."""
    if beam not in ops.BEAM_WIDTHS:
        raise ValueError(f"beam={beam!r}: one of {ops.BEAM_WIDTHS}")
    if beam_info is not None:
        beam_info.update(greedy=[], changed=0, kept_greedy=0, err_chosen=0.0, err_greedy=0.0)
    levels = list(model.rq.vq_layers)
    Ws, bs, scs, shs = model.encoder.folded()
    cbs = [q.embedding.weight.detach() for q in levels]
    flat, ks = ops.flatten_codebooks(cbs)
    idx_parts, last_parts, tie_parts, prev_parts = [], [], [], []
    for lo in range(0, data.shape[0], chunk_rows):
        x = data[lo:lo + chunk_rows]
        a = {} if audit is not None else None
        idx, latent, _, _ = ops.encode_assign(x, Ws, bs, flat, ks, scs, shs, want_latent=True, audit=a,
                                              tie_tau=ops.NEARTIE_TAU)
        if latents is not None:
            latents.append(latent)
        if a is not None:
            tie_parts.append(a["neartie"])
        if beam > 1:
            chosen, info = ops.beam_choose(latent, flat, ks, idx, beam)
            if beam_info is not None:
                both = torch.isfinite(info["err_chosen"]) & torch.isfinite(info["err_greedy"])
                beam_info["greedy"].append(idx)
                beam_info["changed"] += int((chosen != idx).any(1).sum())
                beam_info["kept_greedy"] += int(info["kept_greedy"].sum())
                beam_info["err_chosen"] += float(info["err_chosen"][both].double().sum())
                beam_info["err_greedy"] += float(info["err_greedy"][both].double().sum())
            idx_parts.append(chosen)
            L = len(levels)
            for depth, parts in ((L - 1, last_parts), (L - 2, prev_parts if want_prev else None)):
                if parts is None or depth < 0:
                    continue
                if depth == 0:
                    parts.append(latent)
                else:
                    pflat, pks = ops.flatten_codebooks(cbs[:depth])
                    parts.append(ops.rq_audit(latent, pflat, pks, chosen[:, :depth], want_resid=True)["resid"])
            continue
        idx_parts.append(idx)
        if len(levels) > 1:
            pflat, pks = ops.flatten_codebooks(cbs[:-1])
            _, _, _, resid = ops.rq_assign(latent, pflat, pks, want_resid=True)
            last_parts.append(resid[len(levels) - 1].clone())
            if want_prev:
                prev_parts.append(resid[len(levels) - 2].clone())
        else:
            last_parts.append(latent)
    if audit is not None:
        audit["neartie"] = torch.cat(tie_parts) if tie_parts else torch.zeros(0, dtype=torch.int32, device=data.device)
    if want_prev:
        return torch.cat(idx_parts), torch.cat(last_parts), ks, torch.cat(prev_parts) if prev_parts else None
    return torch.cat(idx_parts), torch.cat(last_parts), ks


@torch.no_grad()
def resolve_collisions(model, idx, resid_last, ks, max_rounds=MAX_ROUNDS, on_round=None, ctx=None):
    """:101-128.  Mutates and returns idx; also returns the number of groups seen in each round.

    With a distributed context (torchrun) a round's groups are SHARDED over the ranks: every
    rank lists the groups (a device sort of the full index matrix, identical everywhere), solves a contiguous run of
    them holding about 1/world of the colliding items, and one all-gather of the new last-level codes -- in rank order,
    which is group order -- updates every rank's copy.  Groups are independent within a round, so the result is the
    single-process one."""
    levels = list(model.rq.vq_layers)
    for q in levels[:-1]:
        q.sk_epsilon = 0.0
    if levels[-1].sk_epsilon == 0.0:
        levels[-1].sk_epsilon = 0.003
    last = levels[-1]
    cb_last = last.embedding.weight.detach().contiguous()
    L = len(levels)
    history = []
    sharded = ctx is not None and ctx.enabled
    for _ in range(max_rounds):
        found = ops.collision_groups(idx, ks, want_groups="device")
        if found["n_groups"] == 0:
            break
        history.append(found["n_groups"])
        if on_round is not None:
            on_round(len(history) - 1, found["n_groups"])
        members = found["members"]
        offs = found["offsets"].cpu().numpy()
        if sharded and found["n_groups"] >= ctx.world_size:
            # group boundaries nearest to equal shares of the colliding items
            cuts = np.searchsorted(offs, [offs[-1] * r / ctx.world_size for r in range(1, ctx.world_size)], side="left")
            bounds = np.concatenate([[0], np.minimum(cuts, found["n_groups"]), [found["n_groups"]]])
            bounds = np.maximum.accumulate(bounds)
            g_lo, g_hi = int(bounds[ctx.rank]), int(bounds[ctx.rank + 1])
            mine = members[int(offs[g_lo]):int(offs[g_hi])]
            if g_hi > g_lo:
                rows = resid_last.index_select(0, mine)
                new_mine = ops.sinkhorn_assign(rows, cb_last, last.sk_epsilon, last.sk_iters,
                                               group_offsets=offs[g_lo:g_hi + 1] - offs[g_lo])
            else:
                new_mine = torch.zeros(0, dtype=torch.int64, device=idx.device)
            counts = [int(offs[bounds[r + 1]] - offs[bounds[r]]) for r in range(ctx.world_size)]
            new_last = ctx.gather_rows(new_mine, counts=counts)
        else:
            rows = resid_last.index_select(0, members)
            new_last = ops.sinkhorn_assign(rows, cb_last, last.sk_epsilon, last.sk_iters, group_offsets=offs)
        idx[members, L - 1] = new_last
    return idx, history


def _prefix_groups(idx, ks, depth):
    """The buckets of items sharing idx[:, :depth], in collision_groups' "device" layout: (members, offsets, count, largest).
    depth == 0 is one bucket of all items (none when there are no items)."""
    n = idx.shape[0]
    if depth == 0:
        members = torch.arange(n, dtype=torch.int64, device=idx.device)
        offsets = torch.tensor([0, n] if n else [0], dtype=torch.int64, device=idx.device)
        return members, offsets, (1 if n else 0), n
    found = ops.collision_groups(idx[:, :depth].contiguous(), ks[:depth], want_groups="device")
    return found["members"], found["offsets"], found["n_groups"], found["max_count"] if found["n_groups"] else 0


# ---- opt-in: what the rounds leave colliding gets the nearest free last-level code (--finish nearest_free) ------------------------
@torch.no_grad()
def finish_collisions(model, idx, resid_last, ks):
    """Beyond the reference (which stops at :128 and writes what still collides): ops.finish_nearest_free over the buckets of
    items sharing idx[:, :L-1] -- include/lcrec.h, lcrec_finish_nearest_free, states the rule.  Only the last-level code of the
    items that move changes.  Mutates idx; returns dict(moved, unresolved, buckets, largest_bucket).  Afterwards exactly
    `unresolved` items still collide: 0 unless a bucket with a shared code holds more items than the last level has codes.
    A function of its inputs alone: under torchrun every rank runs it on its identical copy, with no collective."""
    return _nearest_free_pass(model, idx, None, resid_last, ks)


def _nearest_free_pass(model, idx, n_frozen, resid, ks):
    """finish_collisions (n_frozen None: ops.finish_nearest_free, resid holds a row per item) and extend_collisions
    (ops.extend_nearest_free, a row per new item): the buckets are listed and the result is named the same way."""
    cb_last = list(model.rq.vq_layers)[-1].embedding.weight.detach().contiguous()
    members, offsets, buckets, largest = _prefix_groups(idx, ks, idx.shape[1] - 1)
    if n_frozen is None:
        moved, unresolved = ops.finish_nearest_free(idx, resid, cb_last, ks, members, offsets)
    else:
        moved, unresolved = ops.extend_nearest_free(idx, n_frozen, resid, cb_last, ks, members, offsets)
    return {"moved": moved, "unresolved": unresolved, "buckets": buckets, "largest_bucket": largest}


# ---- opt-in: what the rounds leave colliding moves to its next-best whole tuple (--finish beam) -----------------------------------
@torch.no_grad()
def beam_finish_collisions(model, idx, latents, resid_last, ks, width, resid_prev=None):
    """Beyond the reference: ops.finish_beam over the shared tuples -- include/lcrec.h, lcrec_finish_beam, states the rule.  The
    members of the shared tuples, and only they, are walked through ops.rq_beam (their `width` best whole tuples) and ops.rq_audit
    (the error of the tuple they hold); of every shared tuple the member with the smallest error keeps it and the others move to the
    first tuple of their list that nobody holds.  latents: pass 1's latents, float32 [n, e] (or the list of its chunks).  Mutates
    idx (the rows of the items that move) and resid_last -- and resid_prev, the residual entering level L-2, when given -- for those
    rows: the residuals of the tuple's prefix, as assign_all computes them for a chosen tuple, so that finish_collisions and
    spill_collisions behind this pass see the right ones.  Returns dict(movers, moved, unresolved, rounds, err_moved_sum): the last
    the float64 sum of the moved items' new quantisation errors.  A function of its inputs alone."""
    return _beam_step(model, idx, None, latents, resid_last, ks, width, resid_prev)


def _beam_step(model, idx, n_frozen, latents, resid_last, ks, width, resid_prev):
    """beam_finish_collisions (n_frozen None) and extend_beam_collisions, whose docstrings say what happens.  `items` are the
    members that are walked and `rows` their rows in latents, resid_last and resid_prev: all members, by id, for a whole file; the
    new members, by id - n_frozen, around a frozen catalogue.  The whole-file entry takes the walk's results as they are (they
    go by member position already); the frozen-aware one takes them scattered to the positions of the new members."""
    if width not in ops.BEAM_WIDTHS:
        raise ValueError(f"width={width!r}: one of {ops.BEAM_WIDTHS}")
    out = {"movers": 0, "moved": 0, "unresolved": 0, "rounds": 0, "err_moved_sum": 0.0}
    found = ops.collision_groups(idx, ks, want_groups="device")
    if found["n_groups"] == 0:
        return out
    members = items = rows = found["members"]
    if n_frozen is not None:
        fresh = torch.nonzero(members >= n_frozen).flatten()      # the positions of the new members
        if fresh.numel() == 0:
            return out                                              # (the base collides with itself only: nobody can move)
        items = members[fresh]
        rows = items - n_frozen
    if isinstance(latents, (list, tuple)):
        latents = torch.cat(latents)
    cbs = [q.embedding.weight.detach() for q in model.rq.vq_layers]
    flat, _ = ops.flatten_codebooks(cbs)
    z = latents.index_select(0, rows)
    beams = ops.rq_beam(z, flat, ks, width)
    err_held = ops.rq_audit(z, flat, ks, idx.index_select(0, items))["err"]
    if n_frozen is None:
        took, counters = ops.finish_beam(idx, ks, members, found["offsets"], err_held, beams["tuples"], beams["err"])
    else:
        M, L, dev = members.numel(), idx.shape[1], idx.device
        held_at = torch.empty(M, dtype=torch.float32, device=dev)
        cand = torch.empty((M, width, L), dtype=torch.int64, device=dev)
        cand_err = torch.empty((M, width), dtype=torch.float32, device=dev)
        held_at[fresh], cand[fresh], cand_err[fresh] = err_held, beams["tuples"], beams["err"]
        choice, counters = ops.extend_finish_beam(idx, n_frozen, ks, members, found["offsets"], held_at, cand, cand_err)
        took = choice[fresh]                                        # (a frozen member's choice is -1)
    out.update(counters)
    pos = torch.nonzero(took >= 0).flatten()
    if pos.numel():
        out["err_moved_sum"] = float(beams["err"][pos, took[pos].long()].double().sum())
        _refresh_moved_residuals(cbs, idx, items[pos], z.index_select(0, pos), rows[pos], resid_last, resid_prev)
    return out


def _refresh_moved_residuals(cbs, idx, items, zm, rows, resid_last, resid_prev):
    """Behind a beam step: the moved `items` (latents zm) hold new whole tuples in idx, so rows `rows` of resid_last -- and of
    resid_prev, the residual entering level L-2, when given -- become the residuals of the new tuple's prefix, as assign_all computes
    them for a chosen tuple."""
    L = idx.shape[1]
    held = idx.index_select(0, items)
    for depth, resid in ((L - 1, resid_last), (L - 2, resid_prev)):
        if resid is None or depth < 0:
            continue
        if depth == 0:
            resid[rows] = zm
        else:
            pflat, pks = ops.flatten_codebooks(cbs[:depth])
            resid[rows] = ops.rq_audit(zm, pflat, pks, held[:, :depth], want_resid=True)["resid"]


# ---- opt-in: new items around an index file whose tuples are frozen (--extend BASE.index.json) -------------------------------------
_TOKEN = re.compile(r"<([a-z])_(0|[1-9][0-9]*)>")


def load_index_json(path, ks):
    """int64 [N0, L] numpy array of the tuples in an `.index.json`, L = len(ks).  The library's strict reader
    (ops.index_json_parse) takes the files this project and the reference write -- json.dump with default separators, keys "0",
    "1", ... in order -- in one scan.  What it refuses goes through json.load and a token regex: any valid JSON whose keys are
    exactly "0" .. "N0-1", in any order, with any white space.  Anything else raises ValueError naming the item and the level: a
    wrong level count, a wrong prefix letter, a code >= ks[l] of the checkpoint, missing or duplicate keys."""
    L = len(ks)
    if L > len(PREFIX):
        raise ValueError(f"{L} levels: no token prefix beyond <z_..>")
    with open(path, "rb") as fp:
        text = fp.read()
    try:
        idx = ops.index_json_parse(text, L)
    except ops._lib.LcrecError as strict:
        log.info("%s is not in the writer's own form (%s): reading it with json.load", path, strict)
        idx = _load_index_json_slow(path, text, L)
    for l in range(L):
        bad = np.flatnonzero(idx[:, l] >= int(ks[l]))
        if bad.size:
            raise ValueError(f"{path}: item {int(bad[0])}, level {l}: code {int(idx[bad[0], l])} but the checkpoint's level {l} has "
                             f"{int(ks[l])} codes")
    return idx


def _load_index_json_slow(path, text, L):
    seen = []

    def pairs(items):                                     # (json.load alone would keep the last of two equal keys silently)
        seen.extend(k for k, _ in items)
        return dict(items)
    try:
        doc = json.loads(text.decode("utf-8"), object_pairs_hook=pairs)
    except (UnicodeDecodeError, ValueError) as exc:
        raise ValueError(f"{path}: not an index file: {exc}") from exc
    if not isinstance(doc, dict):
        raise ValueError(f"{path}: not an index file: the top level is not an object")
    n0 = len(doc)
    if len(seen) != n0:
        dup = collections.Counter(seen).most_common(1)[0][0]
        raise ValueError(f"{path}: duplicate key {dup!r}")
    idx = np.empty((n0, L), dtype=np.int64)
    for i in range(n0):
        toks = doc.get(str(i))
        if str(i) not in doc:
            extra = next(k for k in doc if not (k.isascii() and k.isdigit() and str(int(k)) == k and int(k) < n0))
            raise ValueError(f"{path}: {n0} entries but no item {i} (keys must be \"0\" .. \"{n0 - 1}\"; found {extra!r})")
        if not isinstance(toks, list) or len(toks) != L:
            raise ValueError(f"{path}: item {i}: {len(toks) if isinstance(toks, list) else 'no'} tokens, the checkpoint has {L} levels")
        for l, t in enumerate(toks):
            m = _TOKEN.fullmatch(t) if isinstance(t, str) else None
            if m is None or m.group(1) != chr(ord("a") + l) or int(m.group(2)) >= 1 << 63:
                raise ValueError(f"{path}: item {i}, level {l}: {t!r} is not a token <{chr(ord('a') + l)}_CODE>")
            idx[i, l] = int(m.group(2))
    return idx


@torch.no_grad()
def extend_collisions(model, idx, n_frozen, resid_new, ks):
    """ops.extend_nearest_free over the buckets of ALL items sharing idx[:, :L-1] -- include/lcrec.h, lcrec_extend_nearest_free,
    states the rule.  Rows 0 .. n_frozen-1 of idx never change; resid_new holds the rows of the new items only.  Mutates idx;
    returns dict(moved, unresolved, buckets, largest_bucket)."""
    return _nearest_free_pass(model, idx, int(n_frozen), resid_new, ks)


# ---- opt-in: a new item that meets a taken tuple first moves to its next-best whole tuple (--extend --extend_finish beam) ----------
@torch.no_grad()
def extend_beam_collisions(model, idx, n_frozen, latents_new, resid_new, ks, width, resid_prev=None):
    """ops.extend_finish_beam over the shared tuples of ALL items -- include/lcrec.h, lcrec_extend_finish_beam, states the rule:
    beam_finish_collisions around a frozen catalogue.  Rows 0 .. n_frozen-1 of idx never change.  latents_new: pass 1's latents of
    the NEW items only, float32 [n - n_frozen, e] (or the list of its chunks), row i - n_frozen for item i; resid_new and resid_prev
    likewise.  Only the new members of the shared tuples are walked through ops.rq_beam and ops.rq_audit; their results are
    scattered to the members' positions, and the positions of frozen members stay unwritten: the entry never reads them.  Mutates
    idx (the rows of the new items that move) and resid_new -- and resid_prev when given -- for those rows, as
    beam_finish_collisions does, so that extend_collisions and spill_collisions behind this pass see the right residuals.
    Returns dict(movers, moved, unresolved, rounds, err_moved_sum).  A function of its inputs alone."""
    return _beam_step(model, idx, int(n_frozen), latents_new, resid_new, ks, width, resid_prev)


# ---- opt-in: what the two passes above leave colliding moves to a sibling bucket (--spill) ---------------------------------------
@torch.no_grad()
def spill_collisions(model, idx, n_frozen, resid_prev, resid_last, ks):
    """ops.spill_nearest_free over the shared tuples and the super-buckets (the items sharing idx[:, :L-2]) -- include/lcrec.h,
    lcrec_spill_nearest_free, states the rule.  An item whose bucket holds more items than the last level has codes is left colliding
    by finish_collisions / extend_collisions; here it takes the nearest code of level L-2 whose row has a free cell and the nearest
    free last-level code there.  Rows 0 .. n_frozen-1 of idx never change; resid_prev / resid_last hold the rows of the new items
    only (all items when n_frozen == 0): the residuals entering levels L-2 and L-1.  Mutates idx (its last two columns, movers only);
    returns dict(moved, unresolved, super_buckets, largest_super_bucket)."""
    levels = list(model.rq.vq_layers)
    n, L = idx.shape
    if L < 2:
        raise ValueError("--spill moves an item one level above the last: a one-level model has none")
    cb_prev = levels[-2].embedding.weight.detach().contiguous()
    cb_last = levels[-1].embedding.weight.detach().contiguous()
    shared = ops.collision_groups(idx, ks, want_groups="device")
    members, offsets, supers, largest = _prefix_groups(idx, ks, L - 2)
    moved, unresolved = ops.spill_nearest_free(idx, n_frozen, resid_prev, resid_last, cb_prev, cb_last, ks,
                                               (shared["members"], shared["offsets"]), (members, offsets))
    return {"moved": moved, "unresolved": unresolved, "super_buckets": supers, "largest_super_bucket": largest}


def _spill_and_log(model, idx, n_frozen, resid_prev, resid_last, ks, stats):
    """--spill behind --finish nearest_free / --extend: runs spill_collisions, fills the four statistics, logs."""
    stats.update(spill_moved=0, spill_unresolved=0, spill_super_buckets=0, largest_super_bucket=0)
    try:
        done = spill_collisions(model, idx, n_frozen, resid_prev, resid_last, ks)
    except ops._lib.LcrecError as exc:
        if getattr(exc, "code", None) != ops._lib.EUNSUPPORTED:
            raise
        log.warning("--spill: skipped, the earlier pass's result is kept: %s", exc)
        return
    stats.update(spill_moved=done["moved"], spill_unresolved=done["unresolved"], spill_super_buckets=done["super_buckets"],
                 largest_super_bucket=done["largest_super_bucket"])
    log.info("--spill: %d items moved to a free cell of a sibling bucket, %d unresolved (%d super-buckets listed, largest %d items)",
             done["moved"], done["unresolved"], done["super_buckets"], done["largest_super_bucket"])
    if done["unresolved"]:
        log.warning("--spill: %d items still collide: the largest super-bucket (items sharing all codes but the last two) holds %d "
                    "items, the last two levels have %d x %d = %d cells", done["unresolved"], done["largest_super_bucket"],
                    ks[-2], ks[-1], ks[-2] * ks[-1])


def _audit_and_log(model, latents, greedy, neartie, held, stats, what="", first_item=0, foreign_check=True):
    """--audit: the report of the tuples `held` about to be written (audit_indices.report_for, on pass 1's latents, greedy tuples and
    near-tie flags of the same items) goes into stats["audit"]; its summary is logged.  foreign_check=False (--beam: such a
    file leaves the greedy path early by design) skips the warning about a file that was not written from this checkpoint."""
    from . import audit_indices
    flat, ks = ops.flatten_codebooks([q.embedding.weight.detach() for q in model.rq.vq_layers])
    stats["audit"] = audit_indices.report_for(flat, ks, torch.cat(latents), greedy, neartie, held, first_item=first_item)
    for line in audit_indices.summary(stats["audit"]):
        log.info("--audit%s: %s", what, line)
    if foreign_check:
        audit_indices.warn_if_foreign(stats["audit"])


def _refuse_one_level(args):
    if len(args.num_emb_list) < 2:
        raise ValueError("--spill moves an item one level above the last: this checkpoint's model has one level "
                         f"(num_emb_list={list(args.num_emb_list)})")


def _colliding(rows):
    """items that share their tuple with an earlier one, on the host (the N == N0 path launches nothing)"""
    return int(rows.shape[0] - np.unique(rows, axis=0).shape[0]) if rows.shape[0] else 0


def open_run(ckpt_path, data_path=None, device="cuda:0", trust=False, spill=False, sharded=False):
    """How every run over a checkpoint and its data file opens -> (checkpoint dict, EmbDataset, model): the checkpoint is read
    (load_checkpoint, `trust` as its unrestricted unpickler); with `spill` a one-level model is refused as soon as the checkpoint's
    arguments are read, before the data file is opened; the data file is `data_path` or the one the checkpoint names,
    memory-mapped when its rows go to a GPU range by range (a cuda `device`, or `sharded` ranks); the model is built from the
    checkpoint's arguments with the state dict loaded, still on the host and in training mode."""
    ckpt = load_checkpoint(ckpt_path, trust=trust)
    args = ckpt["args"]
    if spill:
        _refuse_one_level(args)
    data = EmbDataset(data_path or args.data_path, mmap=sharded or str(device).startswith("cuda"))
    model = build_model_from_args(args, data.dim)
    model.load_state_dict(ckpt["state_dict"])
    return ckpt, data, model


def _refusals(beam=1, finish="none", extend=None, extend_finish="nearest_free", spill=False, audit=False, recheck=False,
              sharded=False, rounds=MAX_ROUNDS, finish_width=8):
    """What generate() refuses before it opens any file: (condition, message) pairs in the order in which they win when several
    apply (tests/golden/f13_generate_refusals.json records which does, for every combination).  `finish` is looked at last and
    only without `extend`, which ignores it."""
    beamed = beam in ops.BEAM_WIDTHS and beam > 1
    extended = extend is not None
    return [
        (beam not in ops.BEAM_WIDTHS, f"--beam {beam!r}: one of {ops.BEAM_WIDTHS}"),
        (beamed and extended, "--beam with --extend is not supported: the new items are indexed around frozen tuples by the distance "
                              "rule alone"),
        (beamed and recheck, "--beam with --recheck_neartie is not supported: the re-evaluation reproduces the reference's greedy walk"),
        (beamed and sharded, "--beam under torchrun is not supported: run it in a single process"),
        (not (isinstance(rounds, int) and rounds >= 0), f"--rounds {rounds!r}: an integer >= 0"),
        (finish_width not in FINISH_WIDTHS, f"--finish_width {finish_width!r}: one of {FINISH_WIDTHS}"),
        (extend_finish not in EXTEND_FINISH_MODES, f"extend_finish={extend_finish!r}: one of {EXTEND_FINISH_MODES}"),
        (extend_finish != "nearest_free" and not extended,
         f"--extend_finish {extend_finish} finishes the new items of --extend: give --extend BASE.index.json"),
        (finish == "beam" and extended, "--finish beam with --extend is not supported: the conflict rounds and --finish do not run around "
                                        "frozen tuples; --extend_finish beam is that step for the new items"),
        (finish == "beam" and recheck, "--finish beam with --recheck_neartie is not supported: the beam starts from the latents of pass 1, "
                                       "which the re-evaluation does not patch"),
        (finish == "beam" and sharded, "--finish beam under torchrun is not supported: run it in a single process"),
        (spill and not extended and finish not in ("nearest_free", "beam"),
         "--spill runs over what --finish nearest_free or --extend leave unresolved: give one of them"),
        (spill and recheck, "--spill with --recheck_neartie is not supported: the residuals of level L-2 that the re-evaluation "
                            "patches are not kept"),
        (spill and sharded, "--spill under torchrun is not supported: run it in a single process"),
        (audit and recheck, "--audit with --recheck_neartie is not supported: the audit starts from the latents of pass 1, which the "
                            "re-evaluation does not patch"),
        (audit and sharded, "--audit under torchrun is not supported: run it in a single process"),
        (extended and recheck, "--extend with --recheck_neartie is not supported: the re-evaluation works on the reference's 64-row "
                               "batches of a whole file"),
        (extended and sharded, "--extend under torchrun is not supported: run it in a single process"),
        (not extended and finish not in FINISH_MODES, f"finish={finish!r}: one of {FINISH_MODES}"),
    ]


def _refuse(**flags):
    for refused, message in _refusals(**flags):
        if refused:
            raise ValueError(message)


# the finishing pipeline's log lines, by the prefix of its statistics: `finish` for a whole file, `extend` around a frozen catalogue
_WORDING = {
    "finish": {"beam": "--finish beam: of %d items that share a tuple with a better holder %d moved to a free whole tuple out of a beam of "
                       "%d (%d rounds, their quantisation error sums to %.6g), %d are left to the nearest free last-level code",
               "nearest_free": "--finish nearest_free: %d items moved to the nearest free last-level code, %d unresolved "
                               "(%d buckets listed, largest %d items)",
               "left": "--finish nearest_free: %d items still collide: the largest bucket (items sharing all codes but the "
                       "last) holds %d items, the last level has %d codes"},
    "extend": {"beam": "--extend_finish beam: of %d new items whose tuple is taken %d moved to a free whole tuple out of a beam of %d "
                       "(%d rounds, their quantisation error sums to %.6g), %d are left to the nearest free last-level code",
               "nearest_free": "--extend: %d base items kept, %d new items, %d of them moved to the nearest free last-level code, "
                               "%d unresolved (%d buckets listed, largest %d items)",
               "left": "--extend: %d new items still collide: the largest bucket (items sharing all codes but the last) holds %d "
                       "items, the last level has %d codes"},
}


def _finish_passes(model, idx, ks, resid_last, resid_prev, latents, first_pass, stats, prefix, n_frozen=None, beam_width=None,
                   nearest_free=True, audit=None, lead=True):
    """The finishing pipeline behind pass 1 (and the conflict rounds), the same for a whole file and for --extend: the beam step
    (beam_width: 2, 4 or 8; None: not asked for), the nearest-free pass (unless nearest_free is False: --finish none), --spill
    (resid_prev, the residual entering level L-2, is given), the truncation warning against `first_pass`, --audit, and the
    collision statistics of what is left.  Mutates idx and the residuals; fills stats -- `prefix`_beam_*, `prefix`_moved,
    `prefix`_unresolved, spill_*, audit, max_conflicts, collision_rate -- and logs under _WORDING[prefix].
    n_frozen: None for a whole file (the whole-file kernels); N0 around a frozen catalogue, where resid_last, resid_prev and
    latents hold the rows of the new items only and the audit covers those.  audit: None, or dict(greedy, neartie, what,
    foreign_check) for _audit_and_log.  lead: False on the ranks of a torchrun that leave the nearest-free pass's log lines to
    rank 0.  Returns the nearest-free pass's dict, or None."""
    says, n, first = _WORDING[prefix], idx.shape[0], n_frozen or 0
    done = None
    if beam_width is not None:
        done = _beam_step(model, idx, n_frozen, latents, resid_last, ks, beam_width, resid_prev)
        stats.update({f"{prefix}_beam_width": beam_width, f"{prefix}_beam_movers": done["movers"], f"{prefix}_beam_moved": done["moved"],
                      f"{prefix}_beam_unresolved": done["unresolved"], f"{prefix}_beam_rounds": done["rounds"]})
        log.info(says["beam"], done["movers"], done["moved"], beam_width, done["rounds"], done["err_moved_sum"], done["unresolved"])
        done = None
    if nearest_free:
        done = _nearest_free_pass(model, idx, n_frozen, resid_last, ks)      # every rank, on its identical copy: no collective
        stats.update({f"{prefix}_moved": done["moved"], f"{prefix}_unresolved": done["unresolved"]})
        if lead:
            counts = () if n_frozen is None else (n_frozen, n - n_frozen)
            log.info(says["nearest_free"], *counts, done["moved"], done["unresolved"], done["buckets"], done["largest_bucket"])
            if done["unresolved"]:
                log.warning(says["left"], done["unresolved"], done["largest_bucket"], ks[-1])
    if resid_prev is not None:
        _spill_and_log(model, idx, first, resid_prev, resid_last, ks, stats)
    _warn_if_reference_would_truncate(first_pass, idx)
    if audit is not None:
        _audit_and_log(model, latents, audit["greedy"], audit["neartie"], idx[first:], stats, audit["what"], first_item=first,
                       foreign_check=audit["foreign_check"])
    final = ops.collision_groups(idx, ks, want_groups=False)
    stats.update(max_conflicts=final["max_count"], collision_rate=(n - final["unique"]) / n if n else 0.0)
    return done


def _print_and_write(final, stats, output_file, verbose, lead=True):
    """The reference's three closing lines (:131-136) and the file (rank 0's, under torchrun)."""
    if verbose:
        print("All indices number: ", stats["items"])
        print("Max number of conflicts: ", stats["max_conflicts"])
        print("Collision Rate", stats["collision_rate"])
    if lead:
        os.makedirs(os.path.dirname(os.path.abspath(output_file)), exist_ok=True)
        dump_index_json(final, output_file)


def generate_extended(ckpt_path, output_file, base_file, device="cuda:0", data_path=None, verbose=True, trust_checkpoint=False,
                      spill=False, audit=False, extend_finish="nearest_free", finish_width=8):
    """--extend: the data file holds the whole catalogue, its first N0 rows are the items of `base_file` (keys "0" .. "N0-1") and
    rows N0 .. N-1 are new.  The output holds all N items; the first N0 entries carry exactly the base file's tuples (and, for a
    base written by this project or by the reference, the output's first len(base) - 1 bytes are the base file's without its
    closing brace); each new item gets its pass-1 tuple unless that tuple is taken, and then the nearest free last-level code
    of its bucket (extend_collisions).

    The Sinkhorn conflict rounds are NOT run here: they re-assign within a group of colliding items and know nothing of codes held
    outside it, so beside a frozen catalogue most of their work would be undone again.  The distance rule alone decides.
    --finish is ignored for the same reason.  N == N0 launches nothing and rewrites the base.
    extend_finish: "nearest_free" is the flow above.  "beam": a new item whose pass-1 tuple is taken first moves to the next-best
        whole tuple nobody holds, out of a beam of `finish_width` (2, 4 or 8) tuples of its own (extend_beam_collisions), and
        extend_collisions runs on what that leaves.  The statistics then gain extend_beam_width, extend_beam_movers,
        extend_beam_moved, extend_beam_unresolved and extend_beam_rounds; extend_moved and extend_unresolved keep their meaning, the
        nearest-free pass.  N == N0: the five are 0 (and the width).
    spill: the new items that extend_collisions leaves unresolved go through spill_collisions.
    audit: stats["audit"] is the index audit of the NEW rows' tuples (no latents exist for the frozen items); N == N0: no report."""
    _refuse(extend=base_file, extend_finish=extend_finish, spill=spill, audit=audit, finish_width=finish_width)
    beam_step = extend_finish == "beam"
    _, data, model = open_run(ckpt_path, data_path, device, trust=trust_checkpoint, spill=spill)
    ks = [int(q.embedding.weight.shape[0]) for q in model.rq.vq_layers]
    base = load_index_json(base_file, ks)
    n0, n = base.shape[0], len(data)
    if n < n0:
        raise ValueError(f"--extend: {base_file} holds {n0} items but the data file only {n} rows: the data file must hold the whole "
                         "catalogue, the base's items first")
    stats = {"items": n, "base_items": n0, "new_items": n - n0, "extend_moved": 0, "extend_unresolved": 0, "buckets": 0,
             "largest_bucket": 0, "neartie_items": 0, "neartie_tau": ops.NEARTIE_TAU}
    if beam_step:
        stats.update(extend_beam_width=finish_width, extend_beam_movers=0, extend_beam_moved=0, extend_beam_unresolved=0,
                     extend_beam_rounds=0)
    if spill:
        stats.update(spill_moved=0, spill_unresolved=0, spill_super_buckets=0, largest_super_bucket=0)
    if n == n0:
        final = base
        stats["base_colliding"] = _colliding(base)
        stats["collision_rate"] = stats["base_colliding"] / n if n else 0.0
        stats["max_conflicts"] = int(np.unique(base, axis=0, return_counts=True)[1].max()) if n else 0
    else:
        dev = torch.device(device)
        model = model.to(dev).eval()
        ties = {}
        latents = [] if audit or beam_step else None
        idx_new, resid_new, ks, *prev = assign_all(model, data.to_device(dev, rows=(n0, n)), audit=ties, want_prev=spill, latents=latents)
        stats["neartie_items"] = int((ties["neartie"] != 0).sum())
        base_dev = torch.from_numpy(base).to(dev)
        stats["base_colliding"] = n0 - ops.collision_groups(base_dev, ks, want_groups=False)["unique"] if n0 else 0
        idx = torch.cat([base_dev, idx_new])
        report = dict(greedy=idx_new, neartie=ties["neartie"], what=" (new items)", foreign_check=True) if audit else None
        done = _finish_passes(model, idx, ks, resid_new, prev[0] if spill else None, latents, idx.clone(), stats, "extend", n_frozen=n0,
                              beam_width=finish_width if beam_step else None, audit=report)
        stats.update(buckets=done["buckets"], largest_bucket=done["largest_bucket"])
        final = idx
    _print_and_write(final, stats, output_file, verbose)
    return stats


# ---- opt-in: re-evaluate near-tie items in the reference's own operation order (--recheck_neartie) -----------------------------
def reference_order_indices(state_dict, n_layers, bn, levels, x, eps=1e-5):
    """RQVAE.get_indices(x, use_sk=False) (rqvae.py:68-72) as the reference's torch CPU op sequence on ONE batch `x` (a CPU
    float tensor): nn.Linear / BatchNorm1d(eval) / ReLU per encoder layer (layers.py:18-30,42), then per level
    d = sum(x^2) + sum(w^2)^T - 2 x w^T, argmin, gather, straight-through, residual (vq.py:71-95, rq.py:45-48).
    This is the ONE place the product computes on the host: by request, for the ~0.1 % of items whose assignment hangs on
    the last bits of d -- which bits come out depends on the BLAS under torch (MKL's blocking changes with the batch size and
    the CPU), so the call reproduces "the reference's CPU run" only on a host like the reference's; DESIGN.md section 2.1.
    Returns (indices int64 [n, L], residual entering the last level [n, e])."""
    import torch.nn.functional as F
    step = 4 if bn else 3
    h = x
    for l in range(n_layers):
        slot = l * step + 1
        h = F.linear(h, state_dict[f"encoder.mlp_layers.{slot}.weight"], state_dict[f"encoder.mlp_layers.{slot}.bias"])
        if l != n_layers - 1:
            if bn:
                b = f"encoder.mlp_layers.{slot + 1}"
                h = F.batch_norm(h, state_dict[b + ".running_mean"], state_dict[b + ".running_var"], state_dict[b + ".weight"],
                                 state_dict[b + ".bias"], False, 0.1, eps)
            h = F.relu(h)
    residual, cols, before_last = h, [], h
    for l in range(levels):
        w = state_dict[f"rq.vq_layers.{l}.embedding.weight"]
        if l == levels - 1:
            before_last = residual
        d = torch.sum(residual ** 2, dim=1, keepdim=True) + torch.sum(w ** 2, dim=1, keepdim=True).t() \
            - 2 * torch.matmul(residual, w.t())
        idx = torch.argmin(d, dim=-1)
        q = F.embedding(idx, w)
        q = residual + (q - residual).detach()
        residual = residual - q
        cols.append(idx)
    return torch.stack(cols, dim=-1), before_last


@torch.no_grad()
def recheck_neartie(state_dict, args, data, idx, resid_last, flags, batch_size=64):
    """For every item flagged by the near-tie audit, recompute its tuple the way index/generate_indices.py:77-79 computes it
    -- the reference's op sequence on the CPU, on the very 64-row batch the reference's DataLoader would have put the item in
    (shuffle=False: batch b = items 64 b .. 64 b + 63) -- and overwrite it; items whose code changed before the last level also
    get that evaluation's last-level residual (the conflict rounds re-assign from it).  `data`: EmbDataset or a host array.
    Returns (items re-evaluated, items whose tuple changed)."""
    flagged = torch.nonzero(flags != 0).flatten().cpu().numpy()
    if flagged.size == 0:
        return 0, 0
    sd = {k: v.detach().to("cpu", torch.float32) if v.dtype.is_floating_point else v.detach().cpu() for k, v in state_dict.items()}
    n_layers = len(args.layers) + 1
    levels = idx.shape[1]
    rows = data.embeddings if isinstance(data, EmbDataset) else data
    n = idx.shape[0]
    changed = 0
    new_idx, new_res = [], []
    for b in np.unique(flagged // batch_size):
        lo, hi = int(b) * batch_size, min(n, (int(b) + 1) * batch_size)
        x = torch.from_numpy(np.array(rows[lo:hi], dtype=np.float32))                 # a copy: the file may be a read-only memory map
        bi, br = reference_order_indices(sd, n_layers, bool(args.bn), levels, x)
        mine = flagged[(flagged >= lo) & (flagged < hi)] - lo
        new_idx.append(bi[mine])
        new_res.append(br[mine])
    new_idx, new_res = torch.cat(new_idx).to(idx.device), torch.cat(new_res).to(resid_last.device)
    where = torch.from_numpy(flagged).to(idx.device)
    old = idx[where]
    differ = (old != new_idx).any(1)
    changed = int(differ.sum())
    idx[where] = new_idx
    early = (old[:, :-1] != new_idx[:, :-1]).any(1) if levels > 1 else torch.zeros_like(differ)
    if bool(early.any()):
        resid_last[where[early]] = new_res[early]
    return int(flagged.size), changed


def tokens_for(idx_rows):
    """[[i, j, ...], ...] -> [["<a_i>", "<b_j>", ...], ...] (:83-92)."""
    L = len(idx_rows[0]) if idx_rows else 0
    if L > len(PREFIX):
        raise ValueError(f"{L} levels: no token prefix beyond <z_..>")
    return [[PREFIX[l].format(int(v)) for l, v in enumerate(row)] for row in idx_rows]


def dump_index_json(idx_rows, path, chunk_items=1 << 20):
    """Exactly the bytes of `json.dump({str(item): tokens}, fp)` (:138-145) for an int64 [N, L] index
    matrix (tensor, ndarray or nested list): keys are item ids in order, separators are json's defaults.
    The text is produced by the library (lcrec_index_json_format), a chunk of items at a time."""
    if isinstance(idx_rows, torch.Tensor):
        idx_rows = idx_rows.detach().cpu().numpy()
    rows = np.asarray(idx_rows, dtype=np.int64)
    if rows.ndim != 2:
        rows = rows.reshape(len(rows), -1)
    if rows.shape[1] > len(PREFIX):
        raise ValueError(f"{rows.shape[1]} levels: no token prefix beyond <z_..>")
    with open(path, "wb") as fp:
        fp.write(b"{")
        for lo in range(0, rows.shape[0], chunk_items):
            if lo:
                fp.write(b", ")
            fp.write(ops.index_json_text(rows[lo:lo + chunk_items], first_item=lo))
        fp.write(b"}")


def _digits(t):
    """decimal digit count of non-negative int64 values, elementwise"""
    d = torch.ones_like(t)
    p = 10
    for _ in range(18):
        d += (t >= p).to(t.dtype)
        p *= 10
    return d


def _warn_if_reference_would_truncate(first_pass, final):
    def widths(t):
        if t.numel() == 0:
            return 0, 0
        d = _digits(t.clamp_min(0))
        return int(d.max()), int(d.sum(1).max())
    tok0, sum0 = widths(first_pass)
    tok1, sum1 = widths(final)
    if tok1 > tok0 or sum1 > sum0:
        log.warning("a re-assigned index is wider than anything in pass 1: the reference's fixed-width numpy "
                    "string arrays (generate_indices.py:98-99) would truncate it; this output keeps it intact")


def sharded_assign(ctx, data, assign_fn, device):
    """Pass 1 over this rank's contiguous item range, then ONE gather of (index rows, last-level
    residuals) in rank order: afterwards every rank holds what a single process would have computed
    (items are independent in pass 1, so the shard boundaries do not show in the result).
    `assign_fn(x) -> (idx [n, L], resid_last [n, e], ks)`; `data` is an EmbDataset or a tensor."""
    from . import dist as ldist
    n = len(data)
    lo, hi = ldist.shard_range(n, ctx.rank, ctx.world_size)
    x = data.to_device(device, rows=(lo, hi)) if isinstance(data, EmbDataset) else data[lo:hi].to(device)
    idx, resid_last, ks = assign_fn(x)
    return ctx.gather_rows(idx), ctx.gather_rows(resid_last), ks


def generate(ckpt_path, output_file, device="cuda:0", data_path=None, verbose=True, ctx=None, trust_checkpoint=False,
             recheck=False, finish="none", extend=None, spill=False, audit=False, beam=1, rounds=MAX_ROUNDS, finish_width=8,
             extend_finish="nearest_free"):
    """Whole flow of generate_indices.py:51-145.  Returns a dict of the statistics it prints.
    recheck: re-evaluate the near-tie items of pass 1 in the reference's CPU operation order (recheck_neartie).
    finish: "none" (the reference's bytes), "nearest_free" (finish_collisions after the rounds; beyond the reference) or "beam":
        beam_finish_collisions after the rounds with a beam of `finish_width` (2, 4 or 8) tuples per colliding item, then
        finish_collisions on what it leaves; `spill` stays available behind it.  The statistics gain finish_beam_width,
        finish_beam_movers, finish_beam_moved, finish_beam_unresolved and finish_beam_rounds; finish_moved and finish_unresolved
        keep their meaning for the nearest-free step.  `audit` skips the foreign-file warning for such a run: these tuples leave
        the greedy path early by design.  Refused with ValueError, as `spill` is, with `extend`, `recheck` and under torchrun.
    rounds: the number of conflict rounds at most (resolve_collisions' max_rounds), 20 = the reference's; 0 runs none, and
        rounds=0 with finish="beam" moves only the items that collide in pass 1.

    extend: path of an existing `.index.json` whose items are the first rows of the data file: their tuples are kept and only
        the new rows are indexed, around them (generate_extended, which says why neither the conflict rounds nor `finish` run).
    extend_finish: with `extend` only (ValueError without it): "nearest_free" (the default, today's bytes) or "beam": the new items
        that meet a taken tuple first move to their next-best whole tuple out of a beam of `finish_width` tuples
        (generate_extended names the statistics this adds).
    spill: after finish="nearest_free" or `extend`, the items that pass leaves unresolved move to a sibling bucket
        (spill_collisions; beyond the reference).  Refused with ValueError before the checkpoint is opened: without one of those two
        passes, with `recheck` (the level L-2 residuals it patches are not kept) and under torchrun; and as soon as the checkpoint's
        arguments are read, before the data or the device are touched, for a one-level model.

    audit: the tuples about to be written are walked through the quantiser again, from the latents and the greedy tuples of pass 1
        (kept; the encoder does not run twice), and stats["audit"] says what the moves cost (audit_indices.build_report names its
        keys).  With `extend` it covers the new rows only.  Refused with ValueError, as `spill` is, with `recheck` and under
        torchrun.  Without it the returned dict and the file are exactly what they were.

    beam: 1 (the default) is the code path above, untouched: lcrec_rq_beam is not even called.  2, 4 or 8: pass 1's tuples are the
        chosen tuples of a beam of that width (assign_all); the conflict rounds, `finish`, `spill` and the writer then run as they do
        on those tuples and their residuals, and the statistics gain beam_width, beam_changed (items whose chosen tuple is not the
        greedy one), beam_kept_greedy (items where beam 0 lost to the greedy tuple), beam_err_ratio (the sum of the chosen tuples'
        quantisation errors over the greedy tuples', in float64 over the items where both are finite; at most 1 by construction)
        and collision_rate_pass1 (of the chosen tuples, before the rounds).  With `audit` the report's greedy side stays pass 1's
        greedy tuples, so err_file_mean against err_greedy_mean shows what the beam bought net of the collision moves.  Refused
        with ValueError, as `spill` is, with `extend`, `recheck` and under torchrun.

    Under torchrun (ctx = dist.init_from_env()) pass 1 is item-sharded over the ranks and each conflict round's
    groups are sharded too (resolve_collisions); rank 0 writes the file."""
    from . import dist as ldist
    ctx = ctx or ldist.current()
    _refuse(beam=beam, finish=finish, extend=extend, extend_finish=extend_finish, spill=spill, audit=audit, recheck=recheck,
            sharded=ctx.enabled, rounds=rounds, finish_width=finish_width)
    if extend is not None:
        return generate_extended(ckpt_path, output_file, extend, device=device, data_path=data_path, verbose=verbose,
                                 trust_checkpoint=trust_checkpoint, spill=spill, audit=audit, extend_finish=extend_finish,
                                 finish_width=finish_width)
    lead = ctx.rank == 0
    verbose = verbose and lead
    ckpt, data, model = open_run(ckpt_path, data_path, device, trust=trust_checkpoint, spill=spill, sharded=ctx.enabled)
    args = ckpt["args"]
    model = model.to(torch.device(device)).eval()
    if verbose:
        print(model)
    ties = {}
    prev = []                                              # spill: the residual entering level L-2 (one process: nothing to gather)
    latents = [] if audit or finish == "beam" else None    # audit, finish beam: pass 1's latents (one process too)
    beamed = {} if beam > 1 else None                      # beam: pass 1's greedy tuples and what the beam changed (one process too)

    def assign(x):
        out = assign_all(model, x, audit=ties, want_prev=spill, latents=latents, beam=beam, beam_info=beamed)
        prev.extend(out[3:])
        return out[:3]

    idx, resid_last, ks = sharded_assign(ctx, data, assign, device)
    first_pass = idx.clone()
    beam_stats = {}
    if beam > 1:
        n1 = idx.shape[0]
        pass1 = ops.collision_groups(idx, ks, want_groups=False)
        beam_stats = {"beam_width": beam, "beam_changed": beamed["changed"], "beam_kept_greedy": beamed["kept_greedy"],
                      "beam_err_ratio": beamed["err_chosen"] / beamed["err_greedy"] if beamed["err_greedy"] else 1.0,
                      "collision_rate_pass1": (n1 - pass1["unique"]) / n1 if n1 else 0.0}
        log.info("--beam %d: %d of %d items leave their greedy tuple, %d keep it because beam 0 was worse; quantisation error "
                 "%.4f x the greedy tuples'; collision rate of pass 1 %.6f", beam, beam_stats["beam_changed"], n1,
                 beam_stats["beam_kept_greedy"], beam_stats["beam_err_ratio"], beam_stats["collision_rate_pass1"])
    # near-tie audit of pass 1: items whose two best codes at some level are closer than the rounding noise of
    # vq.py:71-73 -- the only ones a CPU run of the reference could index differently (ops.NEARTIE_TAU)
    neartie_items = int(ctx.sum_int(int((ties["neartie"] != 0).sum())))
    rechecked = (0, 0)
    if recheck:
        flags = ctx.gather_rows(ties["neartie"]) if ctx.enabled else ties["neartie"]
        if lead:
            rechecked = recheck_neartie(ckpt["state_dict"], args, data, idx, resid_last, flags)
        if ctx.enabled:                                    # rank 0's host decides (ranks on other CPUs could round differently)
            ctx.broadcast_(idx)
            ctx.broadcast_(resid_last)
        if lead:
            log.info("--recheck_neartie: %d near-tie items re-evaluated with the reference's torch CPU ops on their batch-64 "
                     "neighbours, %d tuples changed", *rechecked)
        first_pass = idx.clone()

    def show(round_no, n_groups):
        if verbose:
            print(n_groups)

    idx, history = resolve_collisions(model, idx, resid_last, ks, max_rounds=rounds, on_round=show, ctx=ctx)
    n = idx.shape[0]
    stats = {"items": n, "rounds": len(history), "groups_per_round": history, "neartie_items": neartie_items,
             "neartie_tau": ops.NEARTIE_TAU, "rechecked_items": rechecked[0], "recheck_changed": rechecked[1],
             "finish": finish, "finish_moved": 0, "finish_unresolved": 0}
    stats.update(beam_stats)
    report = None
    if audit:                                              # (--beam: the report's greedy side stays pass 1's greedy tuples)
        report = dict(greedy=torch.cat(beamed["greedy"]) if beam > 1 else first_pass, neartie=ties["neartie"], what="",
                      foreign_check=beam == 1 and finish != "beam")
    _finish_passes(model, idx, ks, resid_last, prev[0] if spill else None, latents, first_pass, stats, "finish",
                   beam_width=finish_width if finish == "beam" else None, nearest_free=finish != "none", audit=report, lead=lead)
    if lead:
        log.info("near-tie items in pass 1: %d of %d (top-2 code gap <= %.3g x distance magnitude at some level); only "
                 "these could receive a different tuple from a CPU run of the reference", neartie_items, n, ops.NEARTIE_TAU)
    _print_and_write(idx, stats, output_file, verbose, lead)
    ctx.barrier()
    return stats


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Generate <dataset>.index.json from an RQ-VAE checkpoint")
    ap.add_argument("--dataset", type=str, default="Games")
    ap.add_argument("--ckpt_path", type=str, required=True)
    ap.add_argument("--output_dir", type=str, required=True)
    ap.add_argument("--data_path", type=str, default=None, help="override the data path stored in the checkpoint")
    ap.add_argument("--device", type=str, default="cuda:0")
    ap.add_argument("--recheck_neartie", action="store_true",
                    help="re-evaluate the ~0.1 %% of items flagged by the near-tie audit with the reference's own torch CPU op "
                         "sequence on the 64-row batches generate_indices.py:77-79 forms, and use those tuples (the only items a "
                         "CPU run of the reference can index differently; the outcome depends on the host's BLAS)")
    ap.add_argument("--trust_checkpoint", action="store_true",
                    help="load the checkpoint with the unrestricted unpickler (executes code from the file)")
    ap.add_argument("--finish", choices=FINISH_MODES, default="none",
                    help="after the conflict rounds: none = write what still collides, as the reference does (byte-identical "
                         "output); nearest_free = every item that still shares its tuple gets the nearest free last-level code "
                         "(goes beyond the reference; only those items' last token changes); beam = every such item first "
                         "moves to the next-best whole tuple nobody holds, out of a beam of --finish_width tuples of its own, "
                         "and nearest_free runs on what that leaves (beyond the reference; not with --extend, --recheck_neartie or "
                         "torchrun)")
    ap.add_argument("--finish_width", type=int, choices=FINISH_WIDTHS, default=8, metavar="W",
                    help="--finish beam: the number of whole tuples listed for every colliding item (2, 4 or 8; default 8).  "
                         "Independent of --beam, which shapes pass 1; both may be given")
    ap.add_argument("--rounds", type=int, default=MAX_ROUNDS, metavar="N",
                    help="the number of Sinkhorn conflict rounds at most (default 20, the reference's; 0 = none: with --finish beam "
                         "or nearest_free only the items that collide in pass 1 then leave their pass-1 tuple)")
    ap.add_argument("--extend", type=str, default=None, metavar="BASE.index.json",
                    help="the data file holds a catalogue that has grown: its first N0 rows are the items of BASE.index.json, which "
                         "keep their tuples byte for byte; only the rows after them are indexed, each new item keeping its tuple "
                         "unless it is taken and then moving to the nearest free last-level code (goes beyond the reference).  The "
                         "conflict rounds are not run and --finish is ignored; not with --recheck_neartie or torchrun")
    ap.add_argument("--extend_finish", choices=EXTEND_FINISH_MODES, default="nearest_free",
                    help="--extend: what a new item does whose pass-1 tuple is taken.  nearest_free = the nearest free last-level code "
                         "of its bucket (the default).  beam = it first moves to the next-best whole tuple nobody holds, out of a "
                         "beam of --finish_width tuples of its own, and nearest_free runs on what that leaves (beyond the reference; "
                         "the base's tuples stay byte for byte either way)")
    ap.add_argument("--spill", action="store_true",
                    help="after --finish nearest_free or --extend: an item that pass leaves colliding, because its bucket holds more "
                         "items than the last level has codes, takes the next-nearest code one level up and the nearest free "
                         "last-level code there (goes beyond the reference; the last two tokens of those items change).  Not with "
                         "--recheck_neartie or torchrun; needs at least two levels")
    ap.add_argument("--audit", action="store_true",
                    help="walk the tuples about to be written through the quantiser again and log what the conflict rounds and the "
                         "passes above cost: how many items hold a code that is not their nearest, at which level and rank, and the "
                         "quantisation error that added (audit_indices.py does the same for an existing file).  With --extend the "
                         "new rows only: there are no latents for the frozen items.  Not with --recheck_neartie or torchrun")
    ap.add_argument("--beam", type=int, choices=ops.BEAM_WIDTHS, default=1, metavar="W",
                    help="walk the quantiser's levels in pass 1 with a beam of W partial tuples per item (1, 2, 4 or 8) instead of the "
                         "greedy walk, and give every item the best whole tuple found -- or its greedy one where that leaves the "
                         "smaller residual (goes beyond the reference; 1 = the greedy walk, the default, and the reference's bytes). "
                         "Not with --extend, --recheck_neartie or torchrun")
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    from . import dist as ldist
    ctx = ldist.init_from_env(a)                       # torchrun: one rank per GPU; plain python: inert
    out = os.path.join(a.output_dir, f"{a.dataset}.index.json")
    try:
        return generate(a.ckpt_path, out, device=a.device, data_path=a.data_path, ctx=ctx,
                        trust_checkpoint=a.trust_checkpoint, recheck=a.recheck_neartie, finish=a.finish, extend=a.extend,
                        spill=a.spill, audit=a.audit, beam=a.beam, rounds=a.rounds, finish_width=a.finish_width,
                        extend_finish=a.extend_finish)
    finally:
        ldist.shutdown(ctx)


if __name__ == "__main__":
    main()
