"""The case table of the optimiser step kernel -- csrc/train_ops.hip, optim_step_kernel<RULE> behind lcrec_adamw_step,
lcrec_sgd_step, lcrec_adagrad_step and lcrec_rmsprop_step -- shared by tests/test_optim_host.py (CPU: every row reaches the
loops it is listed for, asked of the library's own plan; the oracle's step against torch's CPU optimisers and against a float64
statement; every hyper-parameter visible in some row) and tests/test_gpu_optim_forms.py (GPU: every row against the oracle, bit
for bit, with and without a ticket).

A row names a rule with its options, a size, the buffers that sit off 16 bytes, the clip coefficient, the schedule and the
step it starts from, and says what it is there for.  `reach` lists the fields of lcrec_optim_plan the row relies on."""
import functools
from collections import namedtuple

import numpy as np

from step_tail_cases import Arena, _ptr, _rc

F32 = np.float32
RULES = ("sgd", "adagrad", "rmsprop", "adam")
COEF = 0.37                        # the clip coefficient of every row that does not say otherwise
LR = dict(adam=1e-2, sgd=1e-1, adagrad=1e-1, rmsprop=1e-2)
NO_SCHEDULE = (-1, 0, 0)
LINEAR_2_10 = (1, 2, 10)           # linear warm-up over 2 steps, decay to 0 at step 10
CAP, PER_WG, THREADS = 256, 8192, 1024

# opts: what a row may set, with torch's defaults.  acc (Adagrad): the caller's fill of state_sum (initial_accumulator_value),
# None = a random positive state
DEFAULTS = dict(adam=dict(wd=0.0, beta1=0.9, beta2=0.999, eps=1e-8, decoupled=False),
                sgd=dict(wd=0.0, momentum=0.0, dampening=0.0, nesterov=False),
                adagrad=dict(wd=0.0, lr_decay=0.0, eps=1e-10, acc=None),
                rmsprop=dict(wd=0.0, alpha=0.99, eps=1e-8, momentum=0.0, centered=False))
# the variant of each rule in which every option acts
FULL = dict(adam=dict(wd=0.1, decoupled=True), sgd=dict(wd=0.1, momentum=0.9, nesterov=True),
            adagrad=dict(wd=0.1, lr_decay=0.01, eps=1e-3), rmsprop=dict(wd=0.1, momentum=0.9, centered=True, eps=1e-3))
FULL_S0 = dict(adam=1, sgd=1, adagrad=7, rmsprop=1)

Row = namedtuple("Row", "kind rule opts count steps s0 clip ready0 off sched reach why")


def _row(kind, rule, opts, why, count=PER_WG + 7, steps=3, s0=0, clip=COEF, ready0=0, off="none", sched=NO_SCHEDULE, reach=()):
    assert set(opts) <= set(DEFAULTS[rule]), opts
    return Row(kind, rule, tuple(sorted(opts.items())), count, steps, s0, clip, ready0, off, sched, tuple(sorted(dict(reach).items())), why)


def _full(kind, rule, why, **kw):
    kw.setdefault("s0", FULL_S0[rule])
    kw.setdefault("sched", LINEAR_2_10)
    return _row(kind, rule, FULL[rule], why, **kw)


RULE_ROWS = [
    _row("rule", "adam", dict(wd=0.1, decoupled=True), "AdamW, decoupled decay"),
    _row("rule", "adam", dict(wd=0.1), "Adam, L2 decay added to the gradient"),
    _row("rule", "adam", dict(), "no decay, betas (0.9, 0.999), eps 1e-8, from step 0"),
    _row("rule", "adam", dict(beta1=0.5, beta2=0.9), "betas (0.5, 0.9)"),
    _row("rule", "adam", dict(eps=1e-3), "eps 1e-3"),
    _row("rule", "adam", dict(wd=0.1, decoupled=True), "AdamW from step 1", s0=1),
    _row("rule", "adam", dict(wd=0.1, decoupled=True), "AdamW from step 999: bias corrections near 1 and 0.63", s0=999),
    _row("rule", "adam", dict(beta1=0.5, beta2=0.9, wd=0.1), "Adam (L2), betas (0.5, 0.9), from step 999", s0=999),
    _row("rule", "sgd", dict(), "plain"),
    _row("rule", "sgd", dict(wd=0.1), "weight decay"),
    _row("rule", "sgd", dict(momentum=0.9), "momentum from an empty buffer: the first step is buf = g", ready0=0),
    _row("rule", "sgd", dict(momentum=0.9), "momentum from a buffer that holds a value", ready0=1),
    _row("rule", "sgd", dict(momentum=0.9, dampening=0.1), "dampening", ready0=1),
    _row("rule", "sgd", dict(momentum=0.9, nesterov=True), "nesterov", ready0=1),
    _row("rule", "adagrad", dict(acc=0.0), "lr_decay 0 from step 0, accumulator 0"),
    _row("rule", "adagrad", dict(), "lr_decay 0 from step 7", s0=7),
    _row("rule", "adagrad", dict(lr_decay=0.01, acc=0.0), "lr_decay 0.01 from step 0, accumulator 0"),
    _row("rule", "adagrad", dict(lr_decay=0.01), "lr_decay 0.01 from step 7", s0=7),
    _row("rule", "adagrad", dict(eps=1e-3), "eps 1e-3"),
    _row("rule", "adagrad", dict(acc=0.1), "accumulator 0.1"),
    _row("rule", "adagrad", dict(wd=0.1), "weight decay"),
    _row("rule", "rmsprop", dict(), "plain, alpha 0.99"),
    _row("rule", "rmsprop", dict(centered=True), "centered: the lerp's small-weight branch"),
    _row("rule", "rmsprop", dict(momentum=0.9), "momentum"),
    _row("rule", "rmsprop", dict(momentum=0.9, centered=True), "centered with momentum"),
    _row("rule", "rmsprop", dict(alpha=0.3, centered=True), "alpha 0.3: the lerp's large-weight branch"),
    _row("rule", "rmsprop", dict(alpha=0.3), "alpha 0.3, not centered"),
    _row("rule", "rmsprop", dict(eps=1e-3), "eps 1e-3"),
    _row("rule", "rmsprop", dict(wd=0.1), "weight decay"),
]
for _rule in RULES:
    RULE_ROWS += [_full("rule", _rule, "every option, clipped by 0.37, linear schedule"),
                  _full("rule", _rule, "every option, clip == NULL: grads untouched", clip=None),
                  _full("rule", _rule, "every option, coefficient exactly 1: grads untouched", clip=1.0)]

# (schedule, warmup, total, s): one step each, the step counter written directly
_EDGES = [(0, 10, 0, "warmup 0"), (1, 10, 0, "warmup 1, s = 0: lr 0"), (1, 10, 1, "warmup 1, s == warmup"), (4, 10, 3, "s < warmup"),
          (4, 10, 4, "s == warmup"), (4, 10, 7, "between warmup and total"), (4, 10, 10, "s == total"), (4, 10, 13, "s > total"),
          (4, 4, 4, "total == warmup, s == total"), (4, 4, 3, "total == warmup, s < warmup"), (4, 4, 9, "total == warmup, s > total"),
          (4, 2 ** 32, 2 ** 31 + 5, "s = 2^31 + 5 below total"), (2 ** 32, 2 ** 33, 2 ** 31 + 5, "s = 2^31 + 5 inside the warm-up")]
SCHEDULE_ROWS = [_row("schedule", "adagrad", FULL["adagrad"], "no schedule, s = 2^31 + 5", count=8, steps=1, s0=2 ** 31 + 5)]
for _kind in (0, 1):
    for _w, _t, _s, _why in _EDGES:
        SCHEDULE_ROWS.append(_row("schedule", "adagrad", FULL["adagrad"], f"schedule {_kind}: {_why}", count=8, steps=1, s0=_s, sched=(_kind, _w, _t)))
SCHEDULE_ROWS += [_row("schedule", "adam", FULL["adam"], "Adam at s = 2^31 + 5: both pow underflow", count=8, steps=1, s0=2 ** 31 + 5,
                       sched=(1, 4, 2 ** 32)),
                  _row("schedule", "adam", FULL["adam"], "Adam at s == total: lr 0", count=8, steps=1, s0=10, sched=(1, 4, 10))]

_BIG = CAP * PER_WG + PER_WG + 3
_SHAPES = [(1, dict(quads=0, scalars=1), "count < 4: one scalar"), (3, dict(quads=0, scalars=3), "count < 4"),
           (4, dict(quads=1, scalars=0), "one quad, no tail"), (6, dict(quads=1, scalars=2), "one quad and a tail of 2"),
           (7, dict(quads=1, scalars=3), "one quad and a tail of 3"),
           (8191, dict(workgroups=1, quad_trips_max=2, quad_trips_min=1, scalars=3), "one workgroup, its last lane one trip short"),
           (8192, dict(workgroups=1, quad_trips_max=2, quad_trips_min=2, scalars=0), "one full workgroup"),
           (8193, dict(workgroups=2, quad_trips_max=1, quad_trips_min=1, scalars=1), "one past a workgroup: a tail of 1"),
           (16387, dict(workgroups=3, quad_trips_max=2, quad_trips_min=1, scalars=3), "three workgroups"),
           (_BIG, dict(workgroups=CAP, quad_trips_max=3, quad_trips_min=2, scalars=3), "past the 256-workgroup cap: a third trip for some lanes, then a tail")]
SHAPE_ROWS = [_full("shape", rule, why, count=c, steps=2, reach=reach) for rule in RULES for c, reach, why in _SHAPES]
_ALIGN = [("none", dict(quads=2049, scalars=3), "every buffer on 16 bytes"), ("all", dict(quads=0, scalars=8199), "every buffer one float off"),
          ("p", dict(quads=0, scalars=8199), "params alone off 16 bytes"), ("g", dict(quads=0, scalars=8199), "grads alone off 16 bytes"),
          ("state", dict(quads=0, scalars=8199, scalar_trips_max=5, scalar_trips_min=4), "one state buffer alone off 16 bytes")]
SHAPE_ROWS += [_full("shape", rule, why, count=8199, steps=2, off=off, reach=reach) for rule in RULES for off, reach, why in _ALIGN]

SKIP_ROWS = [_full("skip", rule, "skip_flag set on the first call, momentum_ready 0", steps=1) for rule in RULES]

ROWS = RULE_ROWS + SCHEDULE_ROWS + SHAPE_ROWS


def row_id(r):
    opts = ",".join(f"{k}={v}" for k, v in r.opts)
    return f"{r.kind}-{r.rule}[{opts}]-n{r.count}x{r.steps}-s{r.s0}-clip{r.clip}-r{r.ready0}-off_{r.off}-sched{'_'.join(map(str, r.sched))}"


def opts_of(r):
    return dict(DEFAULTS[r.rule], **dict(r.opts))


def state_names(r):
    """The state buffers the row's rule uses, in the order of its entry point: buf (momentum buffer | exp_avg), sq (state_sum |
    square_avg | exp_avg_sq), gavg (grad_avg)."""
    o = opts_of(r)
    if r.rule == "adam":
        return ("buf", "sq")
    if r.rule == "sgd":
        return ("buf",) if o["momentum"] else ()
    if r.rule == "adagrad":
        return ("sq",)
    return ("sq",) + (("buf",) if o["momentum"] else ()) + (("gavg",) if o["centered"] else ())


def offsets(r):
    """Element offset of each buffer from a 16-byte boundary."""
    names = ("p", "g") + state_names(r)
    off = {"none": (), "all": names, "p": ("p",), "g": ("g",), "state": names[-1:]}[r.off]
    return {n: int(n in off) for n in names}


def want_plan(r, has_ticket):
    """What lcrec_debug_optim_plan must report for the row: the launch rule restated."""
    aligned = r.off == "none"
    wg = min(CAP, -(-r.count // PER_WG))
    lanes = wg * THREADS
    quads = r.count // 4 if aligned else 0
    scalars = r.count - 4 * quads
    return dict(workgroups=wg, second_launch=int(not has_ticket), quads=quads, scalars=scalars, quad_trips_max=-(-quads // lanes),
                quad_trips_min=quads // lanes, scalar_trips_max=-(-scalars // lanes), scalar_trips_min=scalars // lanes)


# ---------------------------------------------------------------- inputs (host, deterministic; shared: read only)

PLANTS = ("zero", "nan", "p_neg0", "g_neg0", "big")       # g = +0 with zero state | g = NaN | p = -0 | g = -0 | g = 1e30


def planted(count):
    """{index: plant}: the first quad, the last quad and the scalar tail of an aligned buffer each hold a NaN lane among planted
    neighbours; a count below 16 takes what fits, from an ordinary element 0 on."""
    if count < 16:
        small = (None, "nan", "g_neg0", "big", "zero", "p_neg0", None, None)
        return {i: k for i, k in enumerate(small[:count]) if k}
    base = 4 * (count // 4)
    where = {0: "zero", 1: "nan", 2: "p_neg0", 3: "g_neg0", base - 4: "big", base - 3: "g_neg0", base - 2: "nan", base - 1: "p_neg0"}
    where.update(zip(range(base, count), ("big", "nan", "zero")))
    return where


@functools.lru_cache(maxsize=8)
def _inputs(rule, count, names, acc, plant):
    rs = np.random.RandomState(1000 * RULES.index(rule) + count % 997)
    t = {"p": (0.1 * rs.standard_normal(count)).astype(F32), "g": (0.01 * rs.standard_normal(count)).astype(F32),
         "buf": (0.01 * rs.standard_normal(count)).astype(F32), "sq": (1e-4 * (1.0 + rs.uniform(size=count))).astype(F32),
         "gavg": (0.005 * rs.uniform(-1.0, 1.0, size=count)).astype(F32)}
    if acc is not None:
        t["sq"][:] = acc
    t = {k: v for k, v in t.items() if k in ("p", "g") + names}
    if plant:
        for i, kind in planted(count).items():
            if kind == "zero":
                for k in t:
                    if k != "p":
                        t[k][i] = 0.0
            elif kind == "p_neg0":
                t["p"][i] = -0.0
            else:
                t["g"][i] = {"nan": np.nan, "g_neg0": -0.0, "big": 1e30}[kind]
    for v in t.values():
        v.setflags(write=False)
    return t


def inputs(r, plant=True):
    """{p, g, and the row's state buffers}: p ~ 0.1 N(0,1), g ~ 0.01 N(0,1), a non-zero random state (sq above grad_avg^2, so a
    centered RMSprop takes the root of a positive number), with the planted elements when `plant`."""
    return _inputs(r.rule, r.count, state_names(r), opts_of(r).get("acc"), bool(plant))


def oracle_kwargs(r):
    """The row's options as keyword arguments of cpu_oracle.optim_step."""
    o = opts_of(r)
    kw = dict(weight_decay=o["wd"])
    if r.rule == "adam":
        kw.update(beta1=o["beta1"], beta2=o["beta2"], eps=o["eps"], decoupled=o["decoupled"])
    elif r.rule == "sgd":
        kw.update(momentum=o["momentum"], dampening=o["dampening"], nesterov=o["nesterov"])
    elif r.rule == "adagrad":
        kw.update(lr_decay=o["lr_decay"], eps=o["eps"])
    else:
        kw.update(alpha=o["alpha"], eps=o["eps"], momentum=o["momentum"], centered=o["centered"])
    return kw


def oracle_step(oracle, r, t, s, ready, clip, skip=False):
    """One step of the oracle in place on the arrays of `t` at step counter `s`; ready: the uint8 array of the ready byte or None.
    Returns the learning rate used (None when skipped)."""
    return oracle.optim_step(r.rule, t["p"], t["g"], s, LR[r.rule], buf=t.get("buf"), sq=t.get("sq"), gavg=t.get("gavg"), clip=clip,
                             schedule=r.sched[0], warmup_steps=r.sched[1], total_steps=r.sched[2], momentum_ready=ready, skip=skip,
                             **oracle_kwargs(r))


def ready_byte(r):
    return np.array([r.ready0], dtype=np.uint8) if r.rule == "sgd" and "buf" in state_names(r) else None


def oracle_steps(oracle, r, t, steps, clips=None):
    """`steps` steps of the oracle in place on the arrays of `t` from step r.s0; clips: one coefficient per step (default: the
    row's).  Returns (steps taken, the ready byte or None, the learning rate of each step)."""
    ready, lrs = ready_byte(r), []
    for i in range(steps):
        lrs.append(oracle_step(oracle, r, t, r.s0 + i, ready, r.clip if clips is None else clips[i]))
    return r.s0 + steps, (None if ready is None else int(ready[0])), lrs


@functools.lru_cache(maxsize=4)
def expected(r, steps=None):
    """What the row's calls must leave, by the oracle: {p, g, state..., step, ready, lr} (shared: read only)."""
    from oracle import cpu_oracle
    t = {k: v.copy() for k, v in inputs(r).items()}
    s, ready, lrs = oracle_steps(cpu_oracle, r, t, r.steps if steps is None else steps)
    return dict(t, step=s, ready=ready, lr=lrs[-1])


# ---------------------------------------------------------------- device side

SENT32 = 0x7FC5A5A5


def _call(lib, hip, r, d, count, clip, step, ready, lr_out, ticket_ptr, skip):
    o, (sched, warmup, total), lr = opts_of(r), r.sched, LR[r.rule]
    tail = (sched, warmup, total, lr_out.ptr, ticket_ptr, _ptr(skip), hip.ops._stream_ptr())
    if r.rule == "adam":
        return lib.lcrec_adamw_step(d["p"].ptr, d["g"].ptr, d["buf"].ptr, d["sq"].ptr, count, _ptr(clip), step.ptr, lr, o["beta1"], o["beta2"],
                                    o["eps"], o["wd"], int(o["decoupled"]), *tail)
    if r.rule == "sgd":
        return lib.lcrec_sgd_step(d["p"].ptr, d["g"].ptr, _ptr(d.get("buf")), _ptr(ready), count, _ptr(clip), step.ptr, lr, o["momentum"],
                                  o["dampening"], int(o["nesterov"]), o["wd"], *tail)
    if r.rule == "adagrad":
        return lib.lcrec_adagrad_step(d["p"].ptr, d["g"].ptr, d["sq"].ptr, count, _ptr(clip), step.ptr, lr, o["lr_decay"], o["eps"], o["wd"], *tail)
    return lib.lcrec_rmsprop_step(d["p"].ptr, d["g"].ptr, d["sq"].ptr, _ptr(d.get("buf")), _ptr(d.get("gavg")), count, _ptr(clip), step.ptr, lr,
                                  o["alpha"], o["eps"], o["wd"], o["momentum"], int(o["centered"]), *tail)


def run(hip, r, dev, ticket, skip_first=False):
    """The row's r.steps calls of its entry point, enqueued back to back, every buffer and scalar between sentinels, buffers the
    rule does not use passed as NULL, the ticket word (when `ticket`) the middle one of three zeroed words.  skip_first: one call
    with skip_flag set comes first, the flag is then cleared and the row's calls follow; its result is returned too.
    Returns (the state read back after the skipped call or None, the state read back at the end): {p, g, state..., step, ready,
    lr: the bits of lr_out}."""
    import torch
    lib, a = hip._lib.load(), Arena(dev)
    off = offsets(r)
    d = {k: a.put(v.copy(), off[k]) for k, v in inputs(r).items()}
    step = a.put(np.array([r.s0], dtype=np.int64))
    has_ready = r.rule == "sgd" and "buf" in d
    ready = a.put(np.array([r.ready0], dtype=np.uint8), 3) if has_ready else None
    clip = None if r.clip is None else a.put(np.array([123.0, r.clip], dtype=F32), 1)
    lr_out = a.put(None, 1, np.float32, (1,))
    skip = a.put(np.array([1], dtype=np.uint8), 5) if skip_first else None
    words = torch.zeros(3, dtype=torch.int32, device=dev)
    ticket_ptr = words.data_ptr() + 4 if ticket else None

    def read():
        out = {k: v.numpy().copy() for k, v in d.items()}
        out.update(step=int(step.numpy()[0]), ready=None if ready is None else int(ready.numpy()[0]), lr=lr_out.numpy().view(np.uint32)[0])
        a.check()
        assert not bool(words.any()), "the ticket word, or a word beside it, is not zero after the call"
        return out

    skipped = None
    with torch.cuda.device(dev):
        if skip_first:
            _rc(hip, _call(lib, hip, r, d, r.count, clip, step, ready, lr_out, ticket_ptr, skip), "the skipped call")
            skipped = read()
            skip.view.zero_()
        for _ in range(r.steps):
            _rc(hip, _call(lib, hip, r, d, r.count, clip, step, ready, lr_out, ticket_ptr, skip), f"lcrec_{r.rule}_step")
    return skipped, read()
