"""CPU: the table of tests/optim_cases.py and the oracle's optimiser step (oracle/lcrec_oracle.c, lcrec_oracle_optim_step), which
tests/test_gpu_optim_forms.py holds the kernel to bit for bit.

(a) the library's launch plan gives every row the loops and trips the table lists for it;
(b) the oracle against torch's CPU optimisers (foreach=False) driven through clip_grad_norm_ and the schedulers of
    lcrec_amd.trainer: bit for bit on the tensors of ROOT_FREE and, where torch's own sqrt is correctly rounded, of AFTER_ROOT;
    on every element of the tensors of WITH_EXACT_ROOTS against torch with its sqrt replaced by the correctly rounded one; the
    identical share printed for every tensor;
(c) the oracle against a float64 statement of each rule: no further from it than twice what torch's own fp32 result is, torch's
    roots taken correctly rounded;
(d) every hyper-parameter of every rule changes the float64 result of some row by more than 1000 fp32 ulps on half its elements;
(e) Adam's folded constants do not move when the double pow results move by 2 ulp (the device's pow is not correctly rounded);
(f) the schedule rows' learning rates are the float of the Python-double expressions of lcrec_amd.trainer."""
import contextlib
import functools
import warnings

import numpy as np
import pytest
import torch

import optim_cases as oc

# Which tensors of the oracle have torch's bits (torch 2.10 CPU kernels, measured; DESIGN.md, the learners).  torch's CPU sqrt is
# MKL's vector sqrt, which is not IEEE-rounded in every code path MKL picks for a host: one ulp off on 1 % to 30 % of these
# inputs on AVX-512 hosts, on none with MKL_ENABLE_INSTRUCTIONS=AVX2.  So what a rule computes before any root (ROOT_FREE) is held
# to torch on every element, and what follows a root (AFTER_ROOT: Adagrad's and RMSprop's parameters and momentum buffer, and
# through the weight decay g + wd * p everything of a later step) on the elements whose root torch took correctly at every step
# of the row -- where MKL rounds correctly, every element.
ROOT_FREE = {"sgd": ("p", "g", "buf"), "adagrad": ("g", "sq"), "rmsprop": ("g", "sq", "gavg"), "adam": ("g",)}
AFTER_ROOT = {"sgd": (), "adagrad": ("p", "sq"), "rmsprop": ("p", "sq", "buf", "gavg"), "adam": ()}
# with torch's roots taken correctly rounded (ieee_roots): on every element.  Adam's exp_avg: but under L2, which the kernel adds unfused
WITH_EXACT_ROOTS = {"sgd": ("p", "g", "buf"), "adagrad": ("p", "g", "sq"), "rmsprop": ("p", "g", "sq", "buf", "gavg"), "adam": ("g", "buf")}
TORCH_NAMES = dict(adam=dict(buf="exp_avg", sq="exp_avg_sq"), sgd=dict(buf="momentum_buffer"), adagrad=dict(sq="sum"),
                   rmsprop=dict(sq="square_avg", buf="momentum_buffer", gavg="grad_avg"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def ops():
    import lcrec_amd
    lcrec_amd._lib.load()
    return lcrec_amd.ops


# ---------------------------------------------------------------- (a)

@pytest.mark.parametrize("ticket", (True, False))
def test_the_plan_gives_every_row_what_the_table_lists(ops, ticket):
    for r in oc.ROWS + oc.SKIP_ROWS:
        plan = ops.optim_plan(r.count, r.off == "none", ticket)
        assert plan == oc.want_plan(r, ticket), oc.row_id(r)
        assert all(plan[k] == v for k, v in r.reach), f"{oc.row_id(r)}: listed for {dict(r.reach)} ({r.why}), the plan says {plan}"
    assert all(r.reach for r in oc.SHAPE_ROWS)


def test_the_table_reaches_every_path_of_the_kernel(ops):
    plans = [(r, ops.optim_plan(r.count, r.off == "none", True)) for r in oc.SHAPE_ROWS]
    for rule in oc.RULES:
        mine = [p for r, p in plans if r.rule == rule]
        assert {p["scalars"] for p in mine if p["quads"]} >= {0, 1, 2, 3}, "every tail length after a 16-byte loop"
        assert any(p["quads"] == 0 and p["scalars"] < 4 for p in mine), "count < 4"
        assert any(p["workgroups"] == oc.CAP and p["quad_trips_max"] > oc.PER_WG // (4 * oc.THREADS) and p["scalars"] for p in mine), \
            "past the cap: a trip more than a full workgroup's own, and a tail"
        assert any(p["quad_trips_max"] > p["quad_trips_min"] for p in mine) and any(p["scalar_trips_max"] > 1 for p in mine)
        assert {r.off for r, _ in plans if r.rule == rule} == {"none", "all", "p", "g", "state"}
    assert all(sum(oc.offsets(r).values()) == 1 for r in oc.SHAPE_ROWS if r.off in ("p", "g", "state"))
    for rule in oc.RULES:
        clips = {r.clip for r in oc.RULE_ROWS if r.rule == rule and dict(r.opts) == oc.FULL[rule]}
        assert clips == {None, 1.0, oc.COEF}
    assert {r.ready0 for r in oc.RULE_ROWS if r.rule == "sgd" and oc.opts_of(r)["momentum"]} == {0, 1}
    assert all(r.ready0 == 0 for r in oc.SKIP_ROWS) and {r.rule for r in oc.SKIP_ROWS} == set(oc.RULES)


def test_the_planted_elements_sit_where_the_table_says():
    for count in sorted({r.count for r in oc.ROWS}):
        where = oc.planted(count)
        assert all(0 <= i < count for i in where)
        if count >= 16:
            base = 4 * (count // 4)
            for lo, hi in ((0, 4), (base - 4, base)) + (((base, count),) if count > base else ()):
                kinds = [where.get(i) for i in range(lo, hi)]
                assert all(kinds), "a planted element in every lane of the first quad, the last quad and the tail"
                assert ("nan" in kinds) == (hi - lo >= 2)
    r = oc.RULE_ROWS[-3]
    t = oc.inputs(r)
    zero = [i for i, k in oc.planted(r.count).items() if k == "zero"]
    assert zero and all(t[k][i] == 0 and not np.signbit(t[k][i]) for i in zero for k in t if k != "p")
    assert np.isnan(t["g"]).sum() == 3 and np.signbit(t["p"][2]) and t["p"][2] == 0
    clean = oc.inputs(r, plant=False)
    assert all(np.isfinite(v).all() and (v != 0).all() for v in clean.values())


# ---------------------------------------------------------------- the float64 statement of each rule

def schedule_lr(r, s):
    """Python's double arithmetic of lcrec_amd.trainer's multipliers (transformers' schedules) times the base rate."""
    kind, warmup, total = r.sched
    lr = oc.LR[r.rule]
    if kind < 0:
        return lr
    if s < warmup:
        return lr * (float(s) / float(max(1, warmup)))
    return lr * (max(0.0, float(total - s) / float(max(1, total - warmup))) if kind == 1 else 1.0)


def f64_steps(r, clips, lrs, **override):
    """torch's documented update of the row's rule in NumPy double from the row's fp32 inputs (no planted elements): r.steps steps
    with the given coefficient (None: no clipping) and learning rate per step.  override: options replaced (to neutralise one)."""
    o = dict(oc.opts_of(r), **override)
    t = {k: v.astype(np.float64) for k, v in oc.inputs(r, plant=False).items()}
    p, first = t["p"], r.ready0 == 0
    for i in range(r.steps):
        s, lr = r.s0 + i, lrs[i]
        if clips[i] is not None:
            t["g"] = t["g"] * float(clips[i])
        g = t["g"]
        if o["wd"] and not (r.rule == "adam" and o["decoupled"]):
            g = g + o["wd"] * p
        if r.rule == "adam":
            if o["wd"] and o["decoupled"]:
                p = p * (1.0 - lr * o["wd"])
            t["buf"] = o["beta1"] * t["buf"] + (1.0 - o["beta1"]) * g
            t["sq"] = o["beta2"] * t["sq"] + (1.0 - o["beta2"]) * g * g
            bc1, bc2 = 1.0 - o["beta1"] ** (s + 1), 1.0 - o["beta2"] ** (s + 1)
            p = p - (lr / bc1) * t["buf"] / (np.sqrt(t["sq"]) / np.sqrt(bc2) + o["eps"])
        elif r.rule == "sgd":
            if o["momentum"] and "buf" in t:
                t["buf"] = g.copy() if first else o["momentum"] * t["buf"] + (1.0 - o["dampening"]) * g
                g = g + o["momentum"] * t["buf"] if o["nesterov"] else t["buf"]
            first = False
            p = p - lr * g
        elif r.rule == "adagrad":
            clr = lr / (1.0 + s * o["lr_decay"])
            t["sq"] = t["sq"] + g * g
            p = p - clr * g / (np.sqrt(t["sq"]) + o["eps"])
        else:
            t["sq"] = o["alpha"] * t["sq"] + (1.0 - o["alpha"]) * g * g
            if o["centered"] and "gavg" in t:
                t["gavg"] = t["gavg"] + (1.0 - o["alpha"]) * (g - t["gavg"])
                with np.errstate(invalid="ignore"):             # alpha neutralised to 0: sq = g^2 = gavg^2, the difference rounds either way
                    avg = np.sqrt(t["sq"] - t["gavg"] ** 2) + o["eps"]
            else:
                avg = np.sqrt(t["sq"]) + o["eps"]
            if o["momentum"] and "buf" in t:
                t["buf"] = o["momentum"] * t["buf"] + g / avg
                p = p - lr * t["buf"]
            else:
                p = p - lr * g / avg
    t["p"] = p
    return t


def ulps_from(x32, x64):
    """|x32 - x64| in fp32 ulps of the float64 value, per element."""
    with np.errstate(over="ignore"):
        ulp = np.spacing(np.abs(x64).astype(np.float32)).astype(np.float64)
    return np.abs(x32.astype(np.float64) - x64) / ulp


# ---------------------------------------------------------------- (b) torch

@contextlib.contextmanager
def ieee_roots():
    """torch's optimisers with Tensor.sqrt / sqrt_ computed by the hardware's correctly rounded square root (NumPy's), not by MKL's
    vector sqrt: torch as it computes where MKL rounds correctly, whatever the host."""
    def sqrt(self):
        with np.errstate(invalid="ignore"):
            return torch.from_numpy(np.sqrt(self.detach().numpy()))

    def sqrt_(self):
        return self.copy_(sqrt(self))

    own = {k: torch.Tensor.__dict__[k] for k in ("sqrt", "sqrt_") if k in torch.Tensor.__dict__}
    torch.Tensor.sqrt, torch.Tensor.sqrt_ = sqrt, sqrt_
    try:
        yield
    finally:
        for k in ("sqrt", "sqrt_"):
            if k in own:
                setattr(torch.Tensor, k, own[k])
            else:
                delattr(torch.Tensor, k)


def torch_steps(r, ieee=False):
    """The row's steps by torch's CPU optimiser (foreach=False) from the row's inputs without the planted elements, the state
    preset to them, the step counter to r.s0; ieee: under ieee_roots().  Returns ({p, g, state...} as numpy, the clip coefficient
    of each step -- what clip_grad_norm_ multiplied by, or None --, the learning rate of each step)."""
    from lcrec_amd.trainer import constant_schedule_with_warmup, linear_schedule_with_warmup
    o, t0, lr = oc.opts_of(r), oc.inputs(r, plant=False), oc.LR[r.rule]
    pr = torch.nn.Parameter(torch.from_numpy(t0["p"].copy()))
    pr.grad = torch.from_numpy(t0["g"].copy())
    if r.rule == "adam":
        cls = torch.optim.AdamW if o["decoupled"] else torch.optim.Adam
        opt = cls([pr], lr=lr, betas=(o["beta1"], o["beta2"]), eps=o["eps"], weight_decay=o["wd"], foreach=False)
    elif r.rule == "sgd":
        opt = torch.optim.SGD([pr], lr=lr, momentum=o["momentum"], dampening=o["dampening"], nesterov=o["nesterov"], weight_decay=o["wd"],
                              foreach=False)
    elif r.rule == "adagrad":
        opt = torch.optim.Adagrad([pr], lr=lr, lr_decay=o["lr_decay"], eps=o["eps"], weight_decay=o["wd"], foreach=False)
    else:
        opt = torch.optim.RMSprop([pr], lr=lr, alpha=o["alpha"], eps=o["eps"], weight_decay=o["wd"], momentum=o["momentum"],
                                  centered=o["centered"], foreach=False)
    names = TORCH_NAMES[r.rule]
    state = {names[k]: torch.from_numpy(t0[k].copy()) for k in oc.state_names(r)}
    if r.rule == "sgd":
        if r.ready0 == 0:
            state = {}
    else:
        state["step"] = torch.tensor(float(r.s0))
    opt.state[pr] = state
    sched = None
    if r.sched[0] >= 0:
        opt.param_groups[0]["initial_lr"] = lr
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sched = (linear_schedule_with_warmup(opt, r.sched[1], r.sched[2], last_epoch=r.s0 - 1) if r.sched[0] == 1
                     else constant_schedule_with_warmup(opt, r.sched[1], last_epoch=r.s0 - 1))
    clips, lrs = [], []
    for _ in range(r.steps):
        lrs.append(opt.param_groups[0]["lr"])
        if r.clip is None:
            clips.append(None)
        else:
            max_norm = 1e9 if r.clip == 1.0 else r.clip * float(torch.linalg.vector_norm(pr.grad))
            norm = torch.nn.utils.clip_grad_norm_([pr], max_norm, foreach=False)
            clips.append(np.float32(torch.clamp(max_norm / (norm + 1e-6), max=1.0).item()))     # clip_grad_norm_'s own expression
        with ieee_roots() if ieee else contextlib.nullcontext():
            opt.step()
        if sched is not None:
            sched.step()
    st = opt.state[pr]
    out = {"p": pr.detach().numpy(), "g": pr.grad.numpy()}
    out.update({k: st[names[k]].numpy() for k in oc.state_names(r)})
    return out, clips, lrs


@functools.lru_cache(maxsize=None)
def four_ways(r):
    """(torch's result, torch's with correctly rounded roots, the oracle's, the float64 statement's, kept) of a rule row, all with
    torch's clip coefficients.  kept: the elements at which torch's own sqrt of what the rule takes the root of was the correctly
    rounded root at every step (Adagrad, RMSprop; None for the other rules)."""
    from oracle import cpu_oracle
    ref, clips, lrs = torch_steps(r)
    exact_roots, clips2, lrs2 = torch_steps(r, ieee=True)
    assert clips == clips2 and lrs == lrs2
    t = {k: v.copy() for k, v in oc.inputs(r, plant=False).items()}
    ready = oc.ready_byte(r)
    kept = np.ones(r.count, dtype=bool) if r.rule in ("adagrad", "rmsprop") else None
    for i in range(r.steps):
        lr = oc.oracle_step(cpu_oracle, r, t, r.s0 + i, ready, clips[i])
        assert bits(lr) == bits(np.float32(lrs[i])) and lrs[i] == schedule_lr(r, r.s0 + i)
        if kept is not None:
            x = t["sq"].astype(np.float64)
            if "gavg" in t:                 # centered: the root of fma(-grad_avg, grad_avg, square_avg); the product is exact in double
                x = (x - t["gavg"].astype(np.float64) ** 2).astype(np.float32).astype(np.float64)
            with np.errstate(invalid="ignore"):
                kept &= torch.from_numpy(x.astype(np.float32)).sqrt().numpy() == np.sqrt(x).astype(np.float32)
    assert ready is None or ready[0] == 1
    if r.clip == 1.0:
        assert all(c == np.float32(1.0) for c in clips)
    return ref, exact_roots, t, f64_steps(r, clips, lrs), kept


def assert_torch_bits(got, ref, where, what):
    bad = np.flatnonzero((bits(got) != bits(ref)) & where)
    assert bad.size == 0, f"{what}: {bad.size} of {int(where.sum())} elements differ from torch, first at {bad[0]}: {got[bad[0]]!r} vs {ref[bad[0]]!r}"


def shares(got, ref):
    return ", ".join(f"{k} {100 * float((bits(got[k]) == bits(ref[k])).mean()):.2f}%" for k in got)


@pytest.mark.parametrize("r", oc.RULE_ROWS, ids=oc.row_id)
def test_the_oracle_against_torch(r):
    ref, exact_roots, got, _, kept = four_ways(r)
    assert sorted(ref) == sorted(got) == sorted(exact_roots)
    print(f"\n{oc.row_id(r)}: identical to torch: {shares(got, ref)}"
          + ("" if kept is None else f"; torch's roots correctly rounded on {100 * kept.mean():.2f}%")
          + f"\n    to torch with correctly rounded roots: {shares(got, exact_roots)}")
    everywhere = np.ones(r.count, dtype=bool)
    for k in got:
        if k in ROOT_FREE[r.rule] and (k == "g" or r.rule == "sgd" or not oc.opts_of(r)["wd"]):
            assert_torch_bits(got[k], ref[k], everywhere, k)
        elif kept is not None and k in AFTER_ROOT[r.rule]:
            assert kept.any()
            assert_torch_bits(got[k], ref[k], kept, f"{k}, where torch's roots are correctly rounded")
        if k in WITH_EXACT_ROOTS[r.rule] and not (r.rule == "adam" and k == "buf" and oc.opts_of(r)["wd"] and not oc.opts_of(r)["decoupled"]):
            assert_torch_bits(got[k], exact_roots[k], everywhere, f"{k}, torch's roots taken correctly rounded")
    if r.clip is None or r.clip == 1.0:
        assert bits(got["g"]).tobytes() == bits(oc.inputs(r, plant=False)["g"]).tobytes(), "grads untouched"


# ---------------------------------------------------------------- (c) float64

@pytest.mark.parametrize("r", oc.RULE_ROWS, ids=oc.row_id)
def test_the_oracle_is_as_close_to_float64_as_torch_is(r):
    """torch's own error is that of torch with correctly rounded roots: what MKL's sqrt adds or, on a value that cancels to near
    zero, happens to take away differs from host to host (printed beside it)."""
    ref, exact_roots, got, exact, _ = four_ways(r)
    for k in got:
        e_torch, e_oracle = float(ulps_from(exact_roots[k], exact[k]).max()), float(ulps_from(got[k], exact[k]).max())
        print(f"\n{oc.row_id(r)} {k}: max error against float64, in fp32 ulps: torch {e_torch:.4g}, oracle {e_oracle:.4g}"
              f" (torch with this host's sqrt {float(ulps_from(ref[k], exact[k]).max()):.4g})")
        assert e_oracle <= 2.0 * e_torch, f"{k}: the oracle is {e_oracle:.4g} ulps from float64, torch {e_torch:.4g}"


# ---------------------------------------------------------------- (d) visibility

NEUTRAL = dict(wd=dict(wd=0.0), eps=dict(eps=0.0), beta1=dict(beta1=0.0), beta2=dict(beta2=0.0), momentum=dict(momentum=0.0),
               dampening=dict(dampening=0.0), nesterov=dict(nesterov=False), lr_decay=dict(lr_decay=0.0), alpha=dict(alpha=0.0),
               centered=dict(centered=False), decoupled=dict(decoupled=False))
HYPER = dict(adam=("wd", "eps", "beta1", "beta2", "decoupled"), sgd=("wd", "momentum", "dampening", "nesterov"),
             adagrad=("wd", "eps", "lr_decay"), rmsprop=("wd", "eps", "alpha", "momentum", "centered"))


def visible_share(r, what):
    """The share of elements whose float64 parameter moves by more than 1000 fp32 ulps when `what` is neutralised."""
    clips = [r.clip] * r.steps
    lrs = [schedule_lr(r, r.s0 + i) for i in range(r.steps)]
    true = f64_steps(r, clips, lrs)["p"]
    if what == "clip":
        other = f64_steps(r, [1.0] * r.steps, lrs)
    elif what == "schedule":
        other = f64_steps(r, clips, [oc.LR[r.rule]] * r.steps)
    else:
        other = f64_steps(r, clips, lrs, **NEUTRAL[what])
    return float((ulps_from(other["p"].astype(np.float32), true) > 1000.0).mean())


@pytest.mark.parametrize("rule", oc.RULES)
def test_every_hyper_parameter_is_visible_in_some_row(rule):
    rows = [r for r in oc.RULE_ROWS if r.rule == rule]
    for what in HYPER[rule] + ("clip", "schedule"):
        best = max(visible_share(r, what) for r in rows
                   if (what == "clip" and r.clip not in (None, 1.0)) or (what == "schedule" and r.sched[0] >= 0)
                   or (what in NEUTRAL and any(oc.opts_of(r)[k] != v for k, v in NEUTRAL[what].items())))
        print(f"\n{rule} {what}: neutralised, it moves {100 * best:.1f}% of the parameters of its best row by more than 1000 fp32 ulps")
        assert best >= 0.5, f"{rule}: no row in which {what} acts on half of the elements"


# ---------------------------------------------------------------- (e) robust constants

def moved(x, ulps):
    for _ in range(abs(ulps)):
        x = np.nextafter(x, np.inf if ulps > 0 else -np.inf)
    return float(x)


def test_adams_folded_constants_survive_a_pow_two_ulps_off():
    rows = [r for r in oc.ROWS + oc.SKIP_ROWS if r.rule == "adam"]
    assert {r.s0 for r in rows} >= {0, 1, 999, 2 ** 31 + 5}
    for r in rows:
        o = oc.opts_of(r)
        for s in range(r.s0, r.s0 + r.steps):
            lr, t = schedule_lr(r, s), float(s + 1)
            p1, p2 = o["beta1"] ** t, o["beta2"] ** t
            want = (np.float32(lr / (1.0 - p1)), np.float32(np.sqrt(1.0 - p2)))
            for d in (-2, -1, 1, 2):
                got = (np.float32(lr / (1.0 - moved(p1, d))), np.float32(np.sqrt(1.0 - moved(p2, d))))
                assert got == want, f"{oc.row_id(r)} step {s}: pow moved by {d} ulp moves a float constant"


# ---------------------------------------------------------------- (f) schedule

@pytest.mark.parametrize("r", oc.SCHEDULE_ROWS, ids=oc.row_id)
def test_the_schedule_rows_learning_rate_is_the_trainers(oracle, r):
    from lcrec_amd.trainer import constant_schedule_with_warmup, linear_schedule_with_warmup
    kind, warmup, total = r.sched
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=oc.LR[r.rule])
    opt.param_groups[0]["initial_lr"] = oc.LR[r.rule]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if kind == 1:
            linear_schedule_with_warmup(opt, warmup, total, last_epoch=r.s0 - 1)
        elif kind == 0:
            constant_schedule_with_warmup(opt, warmup, last_epoch=r.s0 - 1)
    want = opt.param_groups[0]["lr"]
    assert want == schedule_lr(r, r.s0)
    t = {k: v.copy() for k, v in oc.inputs(r).items()}
    lr = oc.oracle_step(oracle, r, t, r.s0, oc.ready_byte(r), r.clip)
    print(f"\n{oc.row_id(r)}: lr {want!r}")
    assert lr.dtype == np.float32 and bits(lr) == bits(np.float32(want))
    assert bits(oc.expected(r)["lr"]) == bits(np.float32(want))


def test_a_skipped_oracle_step_changes_nothing(oracle):
    for r in oc.SKIP_ROWS:
        t = {k: v.copy() for k, v in oc.inputs(r).items()}
        ready = oc.ready_byte(r)
        assert oc.oracle_step(oracle, r, t, r.s0, ready, r.clip, skip=True) is None
        assert all(bits(t[k]).tobytes() == bits(v).tobytes() for k, v in oc.inputs(r).items()) and (ready is None or ready[0] == 0)
