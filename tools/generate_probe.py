#!/usr/bin/env python3
"""Wall-clock of the index-emission flow (generate_indices.py:51-145) at BASELINE sizes on one GPU:
pass 1 (encode + assign), the conflict rounds, the opt-in nearest-free finishing pass, the .index.json text.

    python tools/generate_probe.py [--items 1000000] [--in_dim 768] [--levels 4] [--codes 256]
    python tools/generate_probe.py --extend_new 10000,100000   # then --extend: the finished tuples as base, that many new items
    python tools/generate_probe.py --spill [--extend_new 100000]  # then --spill over what the finishing pass (and --extend) leave
    python tools/generate_probe.py --audit                     # then the index audit of the tuples about to be written (--audit)
    python tools/generate_probe.py --decode                    # then the decode pass over them: tuples -> embeddings -> error per item
    python tools/generate_probe.py --beam 2,4,8                # then the beam-search quantiser (--beam W) at each width over pass 1's latents
    python tools/generate_probe.py --finish_beam 2,4,8         # then the beam finishing step (--rounds 0 --finish beam) at each width on pass 1's tuples
    python tools/generate_probe.py --extend_new 10000,100000 --extend_finish_beam 2,4,8   # --extend's beam step (--extend_finish beam) at each width, beside the plain --extend step
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lcrec_amd  # noqa: E402
from lcrec_amd import audit_indices, generate_indices as gen, ops  # noqa: E402


def spill_line(what, done, t, tr, after):
    """One line for a timed gen.spill_collisions call and its trace."""
    k = lambda name: tr.get(name, (0, 0.0))
    return (f"{what}: {t * 1e3:.2f} ms (collision_groups {k('collision_groups')[1]:.2f} ms/{k('collision_groups')[0]}, spill_keepers "
            f"{k('spill_keepers')[1]:.3f}, spill_nearest_free {k('spill_nearest_free')[1]:.3f} by the trace brackets)   super-buckets "
            f"{done['super_buckets']}, largest {done['largest_super_bucket']} items, moved {done['moved']}, unresolved "
            f"{done['unresolved']}, collision rate afterwards {after['collision_rate']:.6f}")


def extend_probe(model, x_new, base_file, n0, timed, spill=False):
    """The steps of generate_indices.generate_extended on a base file of n0 items and the rows x_new, each timed on its own; the
    yardstick (a full flow over all N items) is the caller's.  Returns the lines to print."""
    dev = x_new.device
    ks = [int(q.embedding.weight.shape[0]) for q in model.rq.vq_layers]
    base, t_read = timed(lambda: gen.load_index_json(base_file, ks))
    base_dev, t_up = timed(lambda: torch.from_numpy(base).to(dev))
    ops.trace_enable(True)
    (idx_new, resid_new, ks, *prev), t_pass1 = timed(lambda: gen.assign_all(model, x_new, want_prev=spill))
    tr1 = ops.trace_collect()
    idx = torch.cat([base_dev, idx_new])
    done, t_ext = timed(lambda: gen.extend_collisions(model, idx, n0, resid_new, ks))
    tr2 = ops.trace_collect()
    ops.trace_enable(False)
    after = ops.collision_groups(idx, ks, want_groups=False)
    assert bool((idx[:n0] == base_dev).all())
    k = lambda tr, name: tr.get(name, (0, 0.0))[1]
    more = []
    if spill:
        ops.trace_enable(True)
        sp, t_sp = timed(lambda: gen.spill_collisions(model, idx, n0, prev[0], resid_new, ks))
        tr3 = ops.trace_collect()
        ops.trace_enable(False)
        assert bool((idx[:n0] == base_dev).all())
        more = ["  " + spill_line("--spill behind it", sp, t_sp, tr3, ops.collision_groups(idx, ks, want_groups=False))]
    return [f"--extend, {n0} base + {x_new.shape[0]} new items: read + parse {t_read * 1e3:.1f} ms, upload {t_up * 1e3:.2f} ms, "
            f"pass 1 (new rows) {t_pass1 * 1e3:.1f} ms (kernel brackets {sum(v[1] for v in tr1.values()):.1f}), buckets + kernel "
            f"{t_ext * 1e3:.2f} ms (collision_groups {k(tr2, 'collision_groups'):.2f}, extend_nearest_free "
            f"{k(tr2, 'extend_nearest_free'):.2f} by the trace brackets)",
            f"  buckets {done['buckets']}, largest {done['largest_bucket']} items, moved {done['moved']}, unresolved "
            f"{done['unresolved']}, collision rate afterwards {after['collision_rate']:.6f}"] + more


def extend_beam_probe(model, x_new, base_file, n0, widths, runs):
    """--extend --extend_finish beam on a base file of n0 items and the rows x_new: per width one warm-up, then `runs` timed runs on
    fresh copies of pass 1's tuples and residuals; medians of the whole step (gen.extend_beam_collisions), of lcrec_extend_finish_beam
    alone and of the new-members-only rq_beam by the trace brackets; the plain --extend step (gen.extend_collisions on pass 1's
    tuples) timed the same way in the same run as the yardstick; and the NEW items' quantisation error against their greedy tuples'
    for both flows.  Returns the lines to print."""
    dev = x_new.device
    ks = [int(q.embedding.weight.shape[0]) for q in model.rq.vq_layers]
    base_dev = torch.from_numpy(gen.load_index_json(base_file, ks)).to(dev)
    lat = []
    idx_new, resid0, ks = gen.assign_all(model, x_new, latents=lat)
    latent = torch.cat(lat)
    flat, _ = ops.flatten_codebooks([q.embedding.weight.detach() for q in model.rq.vq_layers])
    union = torch.cat([base_dev, idx_new])
    err_sum = lambda t: float(torch.nan_to_num(ops.rq_audit(latent, flat, ks, t[n0:].contiguous())["err"], nan=0.0, posinf=0.0).double().sum())
    e_greedy = err_sum(union)

    def timed_on_copies(fn):
        """fn(idx, resid) on fresh copies: one warm-up, then `runs` timed and traced runs -> (idx, resid, result, walls, traces)"""
        walls, traces = [], []
        for k in range(runs + 1):
            i, r = union.clone(), resid0.clone()
            ops.trace_enable(k > 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            done = fn(i, r)
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
            if k > 0:
                walls.append(t)
                traces.append(ops.trace_collect())
            ops.trace_enable(False)
        return i, r, done, walls, traces

    med = lambda traces, name: float(np.median([q.get(name, (0, 0.0))[1] for q in traces]))
    spread = lambda walls: f"{np.median(walls) * 1e3:.2f} ms (median of {len(walls)}, min {min(walls) * 1e3:.2f}, max {max(walls) * 1e3:.2f})"
    i, _, plain, walls, traces = timed_on_copies(lambda i, r: gen.extend_collisions(model, i, n0, r, ks))
    assert bool((i[:n0] == base_dev).all())
    rate = ops.collision_groups(i, ks, want_groups=False)["collision_rate"]
    lines = [f"--extend_finish beam, {n0} base + {x_new.shape[0]} new items; yardstick of this run, the plain --extend step "
             f"(extend_collisions): {spread(walls)}, collision_groups {med(traces, 'collision_groups'):.3f} ms, extend_nearest_free "
             f"{med(traces, 'extend_nearest_free'):.3f} ms by the trace brackets; moved {plain['moved']}, unresolved {plain['unresolved']}, "
             f"collision rate afterwards {rate:.6f}, error of the new items {err_sum(i) / e_greedy:.4f} x greedy"]
    for W in widths:
        i, r, done, walls, traces = timed_on_copies(lambda i, r: gen.extend_beam_collisions(model, i, n0, latent, r, ks, W))
        assert bool((i[:n0] == base_dev).all())
        e_beam = err_sum(i)
        j, _, fin, walls2, _ = timed_on_copies(lambda a, b: (a.copy_(i), b.copy_(r), gen.extend_collisions(model, a, n0, b, ks))[2])
        rate = ops.collision_groups(j, ks, want_groups=False)["collision_rate"]
        parts = {name: med(traces, name) for name in ("extend_finish_beam", "rq_beam", "rq_audit", "collision_groups")}
        lines.append(
            f"  --finish_width {W}: whole step {spread(walls)}; by the trace brackets lcrec_extend_finish_beam {parts['extend_finish_beam']:.3f} "
            f"ms, new-members-only rq_beam {parts['rq_beam']:.3f} ms, rq_audit {parts['rq_audit']:.3f} ms, collision_groups "
            f"{parts['collision_groups']:.3f} ms (largest: {max(parts, key=parts.get)}); movers {done['movers']}, placed {done['moved']}, "
            f"left to nearest_free {done['unresolved']}, rounds {done['rounds']}; error of the new items {e_beam / e_greedy:.4f} x greedy; "
            f"then extend_collisions (with the copies) {spread(walls2)} moved {fin['moved']}, unresolved {fin['unresolved']}: collision "
            f"rate {rate:.6f}, error of the new items {err_sum(j) / e_greedy:.4f} x greedy")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--in_dim", type=int, default=768)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--codes", type=int, default=256)
    ap.add_argument("--out", type=str, default="/tmp/probe.index.json")
    ap.add_argument("--extend_new", type=str, default="", help="comma-separated counts of new items: time --extend's steps for each, "
                    "with the run's finished tuples as the base file")
    ap.add_argument("--spill", action="store_true", help="time --spill behind the finishing pass (and behind each --extend run); the "
                    "base file of the --extend runs is then the spilled one")
    ap.add_argument("--audit", action="store_true", help="time the index audit (generate_indices --audit) of the finished tuples: one "
                    "warm-up pass, then --audit_runs timed ones, the median reported, with the run's pass 1 and rq_assign as yardsticks")
    ap.add_argument("--audit_runs", type=int, default=5)
    ap.add_argument("--decode", action="store_true", help="time the decode pass (ops.decode_tuples with the items as x, no `out`) over "
                    "the finished tuples: one warm-up pass, then --audit_runs timed ones, the median reported; the two new kernels' "
                    "achieved bytes/s against the HBM peak, the decoder layers beside the encoder's, and the reconstruction loss of "
                    "the finished tuples against the greedy ones")
    ap.add_argument("--beam", type=str, default="", metavar="W[,W...]", help="time the beam-search quantiser (ops.rq_beam, generate "
                    "--beam W) over pass 1's latents at each width given: one warm-up call, then --audit_runs timed ones, the median "
                    "of the rq_beam trace brackets reported beside pass 1's rq_assign and one rq_audit over the same rows in the same "
                    "run, the achieved fma rate against the fp32 vector peak, and what the chosen tuples change")
    ap.add_argument("--finish_beam", type=str, default="", metavar="W[,W...]", help="time the beam finishing step (generate --rounds 0 "
                    "--finish beam --finish_width W) on pass 1's tuples at each width given: one warm-up, then --audit_runs timed runs "
                    "on fresh copies, medians of the whole step (beam_finish_collisions), of lcrec_finish_beam alone and of the "
                    "members-only rq_beam by the trace brackets, beside the conflict rounds and the nearest-free pass of this run, "
                    "and the quantisation error of both flows against the greedy tuples'")
    ap.add_argument("--extend_finish_beam", type=str, default="", metavar="W[,W...]", help="with --extend_new: time --extend's beam step "
                    "(generate --extend --extend_finish beam --finish_width W) at each width given, for each count of new items: one "
                    "warm-up, then --audit_runs timed runs on fresh copies, medians of the whole step (extend_beam_collisions), of "
                    "lcrec_extend_finish_beam alone and of the new-members-only rq_beam by the trace brackets, beside the plain "
                    "--extend step of the same run, and the new items' quantisation error of both flows against their greedy tuples'")
    a = ap.parse_args()
    if a.extend_finish_beam and not a.extend_new:
        ap.error("--extend_finish_beam times a step of --extend: give --extend_new N[,N...]")
    dev = "cuda:0"
    torch.manual_seed(2024)
    model = lcrec_amd.RQVAE(in_dim=a.in_dim, num_emb_list=[a.codes] * a.levels, e_dim=32,
                            layers=[2048, 1024, 512, 256, 128, 64], kmeans_init=False,
                            sk_epsilons=[0.0] * a.levels, sk_iters=50).to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(2024)
    x = torch.randn((a.items, a.in_dim), generator=g, device=dev)
    with torch.no_grad():
        z = model.encoder(x[:65536])
        resid = z
        unused = torch.ones(resid.shape[0], dtype=torch.bool, device=dev)
        for l in range(a.levels):                          # data-scale codebooks: rows of the level's residuals
            perm = torch.randperm(resid.shape[0], generator=g, device=dev)
            pick = perm[unused[perm]][:a.codes]            # never a row that was a code before (its residual is 0)
            unused[pick] = False
            cb = resid[pick].clone()
            model.rq.vq_layers[l].embedding.weight.data.copy_(cb)
            resid = resid - cb[ops.rq_assign(resid.contiguous(), cb.reshape(-1), [a.codes])[0][:, 0]]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    def alloc_stats():
        st = torch.cuda.memory_stats()
        return {k: st.get(k, 0) for k in ("num_device_alloc", "num_device_free", "num_alloc_retries",
                                          "reserved_bytes.all.current")}

    def clocks():
        """current sclk / mclk of card 0 as the driver reports them (a pass that runs 3x slow at a third of the clock
        is a power-state matter, not a scheduling one)"""
        out = []
        for name in ("pp_dpm_sclk", "pp_dpm_mclk"):
            for card in ("card0", "card1"):
                path = f"/sys/class/drm/{card}/device/{name}"
                try:
                    with open(path) as fh:
                        cur = [ln.strip() for ln in fh if "*" in ln]
                    out.append(f"{name}={cur[0] if cur else '?'}")
                    break
                except OSError:
                    continue
        return " ".join(out) or "clocks unreadable"

    w_idx, w_resid, w_ks, *w_prev = gen.assign_all(model, x[:300_000], want_prev=a.spill)   # warm-up: every kernel form and both helper streams used once
    gen.resolve_collisions(model, w_idx, w_resid, w_ks)
    gen.finish_collisions(model, w_idx, w_resid, w_ks)
    if a.spill:
        gen.spill_collisions(model, w_idx, 0, w_prev[0], w_resid, w_ks)
    # Pass 1, first time at full size.  What the round-1 version of this probe timed here -- and sometimes saw take 185 ms
    # instead of 62 -- includes every first-time allocation at the 1 M-item sizes (idx 32 MB, latents 128 MB, the
    # [L][n][e] residual stack 512 MB, its clone): the allocator statistics around the call say whether it went to the device
    # for memory, and the traced repeats below give kernel time against wall time once the sizes are cached.
    a0 = alloc_stats()
    (idx, resid_last, ks, *resid_prev), t_pass1 = timed(lambda: gen.assign_all(model, x, want_prev=a.spill))
    a1 = alloc_stats()
    print(f"pass 1, first call at full size: {t_pass1 * 1e3:.1f} ms; allocator: "
          + ", ".join(f"{k} +{a1[k] - a0[k]}" for k in a0) + f"; {clocks()}")
    reps = []
    for streams in (2, 1, 2):
        ops.set_pipelines(streams)
        b0 = alloc_stats()
        ops.trace_enable(True)
        _, t_rep = timed(lambda: gen.assign_all(model, x))
        tr = ops.trace_collect()
        ops.trace_enable(False)
        b1 = alloc_stats()
        reps.append(t_rep)
        print(f"pass 1 repeated, {streams} pipeline(s): wall {t_rep * 1e3:.1f} ms, kernel brackets {sum(v[1] for v in tr.values()):.1f} ms, "
              f"device allocs +{b1['num_device_alloc'] - b0['num_device_alloc']}; "
              + ", ".join(f"{k} {v[1]:.1f}/{v[0]}" for k, v in sorted(tr.items(), key=lambda kv: -kv[1][1])[:4]))
    ops.set_pipelines(2)
    if t_pass1 > 2.0 * min(reps):
        print(f"SLOW FIRST CALL: {t_pass1 * 1e3:.1f} ms against {min(reps) * 1e3:.1f} ms repeated -- see the allocator line above")
    t_pass1 = min(t_pass1, *reps)
    first = ops.collision_groups(idx, ks, want_groups=False)
    ops.trace_enable(True)
    (idx, history), t_rounds = timed(lambda: gen.resolve_collisions(model, idx, resid_last, ks))
    trace = ops.trace_collect()
    ops.trace_enable(False)
    final = ops.collision_groups(idx, ks, want_groups=False)
    # --finish nearest_free on what the rounds left: the pass alone (the prefix sort that lists the buckets, then the kernel)
    ops.trace_enable(True)
    fin, t_finish = timed(lambda: gen.finish_collisions(model, idx, resid_last, ks))
    ftrace = ops.trace_collect()
    ops.trace_enable(False)
    finished = ops.collision_groups(idx, ks, want_groups=False)
    spill_lines = []
    if a.spill:
        ops.trace_enable(True)
        sp, t_spill = timed(lambda: gen.spill_collisions(model, idx, 0, resid_prev[0], resid_last, ks))
        strace = ops.trace_collect()
        ops.trace_enable(False)
        spill_lines = [spill_line("spill", sp, t_spill, strace, ops.collision_groups(idx, ks, want_groups=False)),
                       f"  yardsticks of this run: conflict rounds {t_rounds * 1e3:.1f} ms, finish nearest_free {t_finish * 1e3:.2f} ms"]
    audit_lines = []
    if a.audit:
        # what generate(audit=True) does behind the passes above: pass 1's latents, greedy tuples and near-tie flags are kept, the
        # tuples about to be written are walked through the quantiser (two rq_audit calls per chunk) and the report is formed on the host
        ties, lat = {}, []
        ops.trace_enable(True)
        (greedy, _, _), t_keep = timed(lambda: gen.assign_all(model, x, audit=ties, latents=lat))
        tr_keep = ops.trace_collect()
        ops.trace_enable(False)
        flat, _ = ops.flatten_codebooks([q.embedding.weight.detach() for q in model.rq.vq_layers])
        latent = torch.cat(lat)
        del lat
        report = lambda: audit_indices.report_for(flat, ks, latent, greedy, ties["neartie"], idx)
        report()                                           # warm-up
        walls, kernels, calls = [], [], 0
        for _ in range(max(a.audit_runs, 1)):
            ops.trace_enable(True)
            rep, t_audit = timed(report)
            tr = ops.trace_collect()
            ops.trace_enable(False)
            walls.append(t_audit)
            calls = tr["rq_audit"][0]
            kernels.append(tr["rq_audit"][1] / calls)
        k = lambda name: tr_keep.get(name, (0, 0.0))
        per_call = float(np.median(kernels))
        audit_lines = [f"audit (report_for)       {np.median(walls) * 1e3:9.1f} ms   median of {len(walls)} runs after one warm-up (min "
                       f"{min(walls) * 1e3:.1f}, max {max(walls) * 1e3:.1f}); rq_audit {per_call:.2f} ms per call by the trace brackets, "
                       f"{calls} calls per run",
                       f"  yardsticks of this run: pass 1 keeping the latents {t_keep * 1e3:.1f} ms (best pass 1 above {t_pass1 * 1e3:.1f} ms), "
                       f"rq_assign {k('rq_assign')[1]:.2f} ms/{k('rq_assign')[0]} by the trace brackets"
                       + ("   ONE rq_audit CALL COSTS MORE THAN THE WHOLE PASS 1" if per_call > t_pass1 * 1e3 else "")]
        audit_lines += ["  " + line for line in audit_indices.summary(rep)]
        del latent
    decode_lines = []
    if a.decode:
        HBM_PEAK = 8.0e12                                  # bytes/s, the part's specified peak (a float4 copy measures 6.29e12)
        CH = 1 << 20                                       # the host chunk of decode_indices
        ops.set_pipelines(1)                               # one stream, as the decode pass runs: the brackets then add up to the wall time
        ops.trace_enable(True)
        (greedy, _, _), t_enc = timed(lambda: gen.assign_all(model, x))
        tr_enc = ops.trace_collect()
        ops.trace_enable(False)
        ops.set_pipelines(2)
        dW, db, dsc, dsh = model.decoder.folded()
        flat, _ = ops.flatten_codebooks([q.embedding.weight.detach() for q in model.rq.vq_layers])

        def decode(tuples):
            return torch.cat([ops.decode_tuples(tuples[lo:lo + CH], flat, ks, dW, db, dsc, dsh, x=x[lo:lo + CH], want_out=False)["err"]
                              for lo in range(0, a.items, CH)])
        decode(idx)                                        # warm-up
        walls, runs = [], []
        for _ in range(max(a.audit_runs, 1)):
            ops.trace_enable(True)
            err_file, t_dec = timed(lambda: decode(idx))
            runs.append(ops.trace_collect())
            ops.trace_enable(False)
            walls.append(t_dec)
        err_greedy = decode(greedy)
        med = lambda name: float(np.median([r.get(name, (0, 0.0))[1] for r in runs]))
        layers = lambda tr: sum(v[1] for k, v in tr.items() if k.startswith("linear_fwd"))
        t_gather, t_err = med("rq_decode_gather"), med("recon_row_error")
        b_gather = a.items * (32 * 4 + a.levels * 8)       # q written once, the tuples read once (the code rows come from L2)
        b_err = 2 * a.items * a.in_dim * 4 + a.items * 4   # y and x read once, err written
        count = float(a.items) * a.in_dim
        rf = float(err_file.cpu().numpy().astype(np.float64).sum() / count)
        rg = float(err_greedy.cpu().numpy().astype(np.float64).sum() / count)
        rate = lambda b, ms: b / (ms * 1e-3) if ms > 0 else 0.0
        decode_lines = [
            f"decode (decode_tuples)   {np.median(walls) * 1e3:9.1f} ms   median of {len(walls)} runs after one warm-up (min {min(walls) * 1e3:.1f}, "
            f"max {max(walls) * 1e3:.1f}); {runs[-1]['rq_decode_gather'][0]} chunks per run",
            f"  rq_decode_gather {t_gather:.3f} ms per run by the trace brackets: {rate(b_gather, t_gather) / 1e12:.2f} TB/s = "
            f"{100 * rate(b_gather, t_gather) / HBM_PEAK:.1f} % of the 8.0 TB/s HBM peak (memory-bound: q written once)",
            f"  recon_row_error  {t_err:.3f} ms per run by the trace brackets: {rate(b_err, t_err) / 1e12:.2f} TB/s = "
            f"{100 * rate(b_err, t_err) / HBM_PEAK:.1f} % of the 8.0 TB/s HBM peak (memory-bound: y and x read once)",
            f"  decoder layers {float(np.median([layers(r) for r in runs])):.1f} ms per run by the trace brackets; the encoder's in this run "
            f"{layers(tr_enc):.1f} ms (pass 1 {t_enc * 1e3:.1f} ms wall)",
            f"  reconstruction loss (mse): finished tuples {rf:.6g}, greedy tuples {rg:.6g} ({100.0 * (rf / rg - 1.0):+.4g} %); "
            f"{int((idx != greedy).any(1).sum())} items hold another tuple than their greedy one"]
        del err_file, err_greedy
    beam_lines = []
    if a.beam:
        FMA_PEAK = 157.3e12 / 2                            # fp32 fma/s of the vector units (157.3 TFLOPS specified)
        lat = []
        ops.trace_enable(True)
        (greedy, _, _), _ = timed(lambda: gen.assign_all(model, x, latents=lat))
        tr_p1 = ops.trace_collect()
        ops.trace_enable(False)
        flat, _ = ops.flatten_codebooks([q.embedding.weight.detach() for q in model.rq.vq_layers])
        latent = torch.cat(lat)
        del lat
        ops.rq_audit(latent, flat, ks, greedy)             # warm-up
        t_aud = []
        for _ in range(max(a.audit_runs, 1)):
            ops.trace_enable(True)
            aud, _ = timed(lambda: ops.rq_audit(latent, flat, ks, greedy))
            t_aud.append(ops.trace_collect()["rq_audit"][1])
            ops.trace_enable(False)
        t_aud = float(np.median(t_aud))
        t_asg = tr_p1.get("rq_assign", (0, 0.0))
        rate0 = ops.collision_groups(greedy, ks, want_groups=False)["collision_rate"]
        beam_lines = [f"beam: yardsticks of this run over the same {a.items} rows: rq_audit {t_aud:.2f} ms per call (median of "
                      f"{max(a.audit_runs, 1)}), pass 1's rq_assign {t_asg[1]:.2f} ms/{t_asg[0]} by the trace brackets; greedy collision "
                      f"rate {rate0:.6f}"]
        for W in [int(w) for w in a.beam.split(",") if w]:
            ops.rq_beam(latent, flat, ks, W)               # warm-up
            ms, calls = [], 0
            for _ in range(max(a.audit_runs, 1)):
                ops.trace_enable(True)
                _, _ = timed(lambda: ops.rq_beam(latent, flat, ks, W))
                calls, t = ops.trace_collect()["rq_beam"]
                ops.trace_enable(False)
                ms.append(t)
            t_beam = float(np.median(ms))
            fmas, live = 0.0, 1
            for k in ks:                                   # the sweep's dot products: live parents x codes x e per item and level
                fmas += float(a.items) * live * k * 32
                live = min(W, live * k)
            chosen, info = ops.beam_choose(latent, flat, ks, greedy, W)
            both = torch.isfinite(info["err_chosen"]) & torch.isfinite(info["err_greedy"])
            ratio = float(info["err_chosen"][both].double().sum() / info["err_greedy"][both].double().sum())
            rate1 = ops.collision_groups(chosen, ks, want_groups=False)["collision_rate"]
            beam_lines.append(
                f"  rq_beam W={W}: {t_beam:.2f} ms per run over {calls} chunk calls (median of {len(ms)}, min {min(ms):.2f}, max "
                f"{max(ms):.2f}) = {t_beam / t_aud:.2f} x rq_audit, {t_beam / (W * t_aud):.2f} x W x rq_audit; {fmas / 1e12:.3f} T fma -> "
                f"{fmas / (t_beam * 1e-3) / 1e12:.2f} T fma/s = {100 * fmas / (t_beam * 1e-3) / FMA_PEAK:.1f} % of the fp32 vector peak; "
                f"beam_err_ratio {ratio:.4f}, changed {int((chosen != greedy).any(1).sum())}, kept greedy "
                f"{int(info['kept_greedy'].sum())}, collision rate of the chosen tuples {rate1:.6f}")
            del chosen, info
        del latent
    fbeam_lines = []
    if a.finish_beam:
        lat = []
        (greedy, resid0, _), _ = timed(lambda: gen.assign_all(model, x, latents=lat))
        flat, _ = ops.flatten_codebooks([q.embedding.weight.detach() for q in model.rq.vq_layers])
        latent = torch.cat(lat)
        del lat
        err_sum = lambda t: float(torch.nan_to_num(ops.rq_audit(latent, flat, ks, t)["err"], nan=0.0, posinf=0.0).double().sum())
        e_greedy, e_today = err_sum(greedy), err_sum(idx)
        shared = ops.collision_groups(greedy, ks, want_groups="device")
        fbeam_lines = [f"finish beam: pass 1 leaves {int(shared['members'].numel())} items in {shared['n_groups']} shared tuples "
                       f"(collision rate {first['collision_rate']:.6f}); yardsticks of this run: conflict rounds {t_rounds * 1e3:.1f} ms, finish "
                       f"nearest_free {t_finish * 1e3:.2f} ms; quantisation error of today's rounds + nearest_free"
                       f"{' (+ spill)' if a.spill else ''}: {e_today / e_greedy:.4f} x greedy"]
        del shared
        for W in [int(w) for w in a.finish_beam.split(",") if w]:
            def step():
                i, r = greedy.clone(), resid0.clone()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                done = gen.beam_finish_collisions(model, i, latent, r, ks, W)
                torch.cuda.synchronize()
                return i, r, done, time.perf_counter() - t0
            step()                                         # warm-up
            walls, runs = [], []
            for _ in range(max(a.audit_runs, 1)):
                ops.trace_enable(True)
                i, r, done, t = step()
                runs.append(ops.trace_collect())
                ops.trace_enable(False)
                walls.append(t)
            med = lambda name: float(np.median([q.get(name, (0, 0.0))[1] for q in runs]))
            e_beam = err_sum(i)
            fin2, t_fin2 = timed(lambda: gen.finish_collisions(model, i, r, ks))
            rate2 = ops.collision_groups(i, ks, want_groups=False)["collision_rate"]
            whole = float(np.median(walls)) * 1e3
            parts = {name: med(name) for name in ("finish_beam", "rq_beam", "rq_audit", "collision_groups")}
            fbeam_lines.append(
                f"  --finish_width {W}: whole step {whole:.2f} ms (median of {len(walls)}, min {min(walls) * 1e3:.2f}, max "
                f"{max(walls) * 1e3:.2f}) = {whole / (t_rounds * 1e3):.2f} x the conflict rounds; by the trace brackets lcrec_finish_beam "
                f"{parts['finish_beam']:.3f} ms, members-only rq_beam {parts['rq_beam']:.3f} ms, rq_audit {parts['rq_audit']:.3f} ms, "
                f"collision_groups {parts['collision_groups']:.3f} ms (largest: {max(parts, key=parts.get)}); movers {done['movers']}, moved "
                f"{done['moved']}, unresolved {done['unresolved']}, rounds {done['rounds']}; error {e_beam / e_greedy:.4f} x greedy; then "
                f"nearest_free {t_fin2 * 1e3:.2f} ms moved {fin2['moved']}, unresolved {fin2['unresolved']}: collision rate {rate2:.6f}, "
                f"error {err_sum(i) / e_greedy:.4f} x greedy")
            del i, r
        del latent, greedy, resid0
    _, t_json = timed(lambda: gen.dump_index_json(idx, a.out))
    size = os.path.getsize(a.out)
    extend_lines = []
    for count in [int(c) for c in a.extend_new.split(",") if c]:
        x_new = torch.randn((count, a.in_dim), generator=g, device=dev)
        extend_probe(model, x_new[:min(count, 4096)], a.out, a.items, timed, a.spill)       # warm-up of the small-launch forms
        extend_lines += extend_probe(model, x_new, a.out, a.items, timed, a.spill)
        if a.extend_finish_beam:
            extend_lines += extend_beam_probe(model, x_new, a.out, a.items, [int(w) for w in a.extend_finish_beam.split(",") if w],
                                              max(a.audit_runs, 1))
        # the yardstick: what a user does today, the whole flow again over all N items (without the file's text)
        x_all = torch.cat([x, x_new])
        def full():
            i, r, k = gen.assign_all(model, x_all)
            i, _ = gen.resolve_collisions(model, i, r, k)
            return gen.finish_collisions(model, i, r, k)
        fin_all, t_full = timed(full)
        extend_lines.append(f"  yardstick, pass 1 + rounds + finish nearest_free over all {x_all.shape[0]} items: {t_full * 1e3:.1f} ms "
                            f"(moved {fin_all['moved']}, unresolved {fin_all['unresolved']})")
        del x_all
    os.remove(a.out)
    print(f"items {a.items}  in_dim {a.in_dim}  {a.levels} x {a.codes} codes")
    print(f"pass 1 (encode+assign)   {t_pass1 * 1e3:9.1f} ms   {a.items / t_pass1 / 1e6:7.2f} M items/s")
    print(f"conflict rounds ({len(history):2d})     {t_rounds * 1e3:9.1f} ms   groups/round {history[:6]}{' ...' if len(history) > 6 else ''}")
    print("  kernels: " + ", ".join(f"{k} {v[1]:.1f} ms/{v[0]}" for k, v in sorted(trace.items(), key=lambda kv: -kv[1][1])))
    print(f"  collision rate {first['collision_rate']:.6f} -> {final['collision_rate']:.6f}")
    print(f"finish nearest_free      {t_finish * 1e3:9.1f} ms   (conflict rounds: {t_rounds * 1e3:.1f} ms)   buckets {fin['buckets']}, "
          f"largest {fin['largest_bucket']} items, moved {fin['moved']}, unresolved {fin['unresolved']}")
    print("  kernels: " + ", ".join(f"{k} {v[1]:.2f} ms/{v[0]}" for k, v in sorted(ftrace.items(), key=lambda kv: -kv[1][1])))
    print(f"  collision rate {final['collision_rate']:.6f} -> {finished['collision_rate']:.6f}")
    for line in spill_lines + audit_lines + decode_lines + beam_lines + fbeam_lines:
        print(line)
    print(f".index.json ({size / 1e6:.0f} MB)     {t_json * 1e3:9.1f} ms   {a.items / t_json / 1e6:7.2f} M items/s (D2H + text + write)")
    for line in extend_lines:
        print(line)


if __name__ == "__main__":
    main()
