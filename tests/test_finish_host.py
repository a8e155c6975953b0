"""CPU: the host side of the nearest-free-code finishing pass (--finish nearest_free) -- the lcrec_finish_nearest_free entry
(declared, exported, bound; its argument checks return before any launch), the CLI flag, and the numpy statement of the rule
(tests/finish_ref.py) on the F6 fixture and on the cases a wrong kernel would plausibly get wrong."""
import os
import re
import subprocess

import numpy as np

import finish_cases as fc
from finish_ref import colliding_items, finish_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_finish_entry():
    import lcrec_amd
    header = open(os.path.join(ROOT, "include", "lcrec.h")).read()
    assert "#define LCREC_ABI_VERSION 3" in header
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(lcrec_[a-z_0-9]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", lcrec_amd._lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (lcrec_[a-z_0-9]+)", out))
    name = "lcrec_finish_nearest_free"
    assert name in declared and name in exported and name in lcrec_amd._lib.EXPORTS
    assert hasattr(lcrec_amd._lib.load(), name)
    assert callable(lcrec_amd.ops.finish_nearest_free)


def test_finish_entry_reports_argument_errors_before_any_launch():
    """Each refusal names the dimension it is about and comes back before anything is enqueued, so no device is needed.  (In a
    thread of its own: the library's last-error text is per thread, and other tests expect this thread's to be empty.)"""
    import ctypes
    import threading
    import lcrec_amd
    lib = lcrec_amd._lib.load()
    seen = []

    def calls():
        buf = (ctypes.c_double * 64)()
        base = ctypes.cast(buf, ctypes.c_void_p).value
        p = ctypes.c_void_p((base + 15) & ~15)                       # 16-byte aligned
        off4, off8 = ctypes.c_void_p(p.value + 4), ctypes.c_void_p(p.value + 8)
        ints = lambda *v: (ctypes.c_int * len(v))(*v)
        f = lib.lcrec_finish_nearest_free

        def call(word, idx=p, n=8, L=3, K=ints(48, 48, 48), resid=p, e=16, cb=p, mem=p, off=p, nb=1, counters=p):
            seen.append((f(idx, n, L, K, resid, e, cb, mem, off, nb, counters, None), word, lib.lcrec_last_error()))

        for e in (0, 8, 24, 128):
            call(b"e_dim=%d" % e, e=e)
        call(b"K[2]=0", K=ints(48, 48, 0))
        call(b"level 2 (K=4096, e=64) does not fit", K=ints(48, 48, 4096), e=64)          # lcrec_rq_assign refuses it too
        call(b"level 0 (K=2048, e=16) does not fit", L=1, K=ints(2048))
        call(b"L=0", L=0)
        call(b"L=17", L=17)
        call(b"n=-1", n=-1)
        call(b"n_buckets=-1", nb=-1)
        call(b"resid_last and codebook_last must be 16-byte aligned", resid=off8)
        call(b"resid_last and codebook_last must be 16-byte aligned", cb=off4)
        call(b"must be 8-byte aligned", idx=off4)
        call(b"must be 8-byte aligned", mem=off4)
        call(b"must be 8-byte aligned", off=off4)
        call(b"counters_out is NULL", counters=None)
        call(b"K is NULL", K=None)
        call(b"NULL pointer", mem=None)

    worker = threading.Thread(target=calls)
    worker.start()
    worker.join()
    assert len(seen) == 19
    for rc, word, text in seen:
        assert rc in (-1, -2) and word in text and b"finish_nearest_free" in text, (rc, word, text)


def test_cli_accepts_finish_and_defaults_to_none():
    from lcrec_amd import generate_indices as gen
    base = ["--ckpt_path", "c.pth", "--output_dir", "out"]
    assert gen.parse_args(base).finish == "none"
    assert gen.parse_args(base + ["--finish", "nearest_free"]).finish == "nearest_free"
    assert gen.parse_args(base + ["--finish", "none"]).finish == "none"
    try:
        gen.parse_args(base + ["--finish", "suffix"])
    except SystemExit:
        pass
    else:
        raise AssertionError("--finish suffix was accepted")
    assert callable(gen.finish_collisions)


def test_reference_on_the_f6_tuples(oracle):
    """The reference's own final tuples still collide on 69 items (the count is recomputed here); the largest bucket that has a
    shared code holds fewer items than K = 48, so the rule must place every one of them."""
    idx, resid, cb, g = fc.f6_case()
    K = cb.shape[0]
    want_movers = fc.movers_by_count(idx)
    assert want_movers == colliding_items(idx) > 0
    new, movers, unresolved = finish_ref(idx, resid, cb)
    print("F6: movers", len(movers), "unresolved", unresolved, "colliding before", colliding_items(idx), "after", colliding_items(new))
    assert len(movers) == want_movers
    assert len(set(movers)) == len(movers)
    assert unresolved == 0
    assert colliding_items(new) == 0
    still = np.ones(len(idx), dtype=bool)
    still[movers] = False
    assert np.array_equal(new[still], idx[still])                                  # every non-mover's tuple is unchanged
    assert np.array_equal(new[:, :-1], idx[:, :-1])                                # only the last level moves
    assert (new[movers, -1] != idx[movers, -1]).all() and (new[:, -1] >= 0).all() and (new[:, -1] < K).all()
    # the precondition the issue reasons from: no touched bucket has more items than K
    sizes = {}
    for row in idx:
        sizes[tuple(row[:-1])] = sizes.get(tuple(row[:-1]), 0) + 1
    touched = {tuple(idx[i, :-1]) for i in movers}
    assert max(sizes[b] for b in touched) <= K


def test_second_mover_does_not_get_a_code_the_first_took(oracle):
    """Four items on code 0 of a 1-d-like codebook: codes at 0, 1, 1.25, 9 along the first axis.  Item 0 sits on code 0 and
    keeps it; items 1, 2 and 3 all have code 1 as their nearest free code.  Served in id order: 1 -> code 1, 2 -> code 2 (its
    next nearest), 3 -> code 3."""
    e = 16
    cb = np.zeros((4, e), dtype=np.float32)
    cb[:, 0] = [0.0, 1.0, 1.25, 9.0]
    resid = np.zeros((4, e), dtype=np.float32)
    resid[:, 0] = [0.0, 0.75, 0.875, 0.8125]
    idx = np.zeros((4, 1), dtype=np.int64)
    new, movers, unresolved = finish_ref(idx, resid, cb)
    assert movers == [1, 2, 3] and unresolved == 0
    assert new[:, 0].tolist() == [0, 1, 2, 3]
    # ... and with one code fewer the last mover has nowhere to go
    new, movers, unresolved = finish_ref(idx, resid, cb[:3])
    assert movers == [1, 2, 3] and unresolved == 1 and new[:, 0].tolist() == [0, 1, 2, 0]


def test_identical_codebook_rows_give_the_lower_code(oracle):
    """Codes 2 and 4 are the same row and the mover sits next to it: its two nearest free codes tie exactly; it takes code 2."""
    e = 16
    r = np.random.RandomState(3)
    cb = r.standard_normal((6, e)).astype(np.float32)
    cb[4] = cb[2]
    resid = np.stack([cb[0], cb[2] + np.float32(0.01) * (cb[0] - cb[2]), cb[1]]).astype(np.float32)
    idx = np.array([[0], [0], [1]], dtype=np.int64)
    d = oracle.distances(resid, cb)
    assert d[1, 2] == d[1, 4] == d[1, [2, 3, 4, 5]].min() and d[0, 0] < d[1, 0]
    new, movers, unresolved = finish_ref(idx, resid, cb)
    assert movers == [1] and unresolved == 0 and new[:, 0].tolist() == [0, 2, 1]


def test_identical_residual_rows_let_the_lower_id_keep(oracle):
    """The fixture's own duplicates (golden_inputs.toy_items: 17 and 1200 copy item 5) can never be told apart by distance."""
    e = 16
    r = np.random.RandomState(4)
    cb = r.standard_normal((5, e)).astype(np.float32)
    row = r.standard_normal(e).astype(np.float32)
    resid = np.stack([row, row, row]).astype(np.float32)
    idx = np.array([[3], [3], [3]], dtype=np.int64)
    new, movers, unresolved = finish_ref(idx, resid, cb)
    assert movers == [1, 2] and unresolved == 0 and new[0, 0] == 3
    order = np.argsort(oracle.distances(resid[:1], cb)[0], kind="stable")
    free = [k for k in order.tolist() if k != 3]
    assert new[1:, 0].tolist() == free[:2]
    # a NaN never wins: an all-NaN holder loses its code to a finite one with a higher id, and goes to the first free code
    resid2 = resid.copy()
    resid2[0] = np.nan
    new, movers, unresolved = finish_ref(idx[:2], resid2[:2], cb)
    assert movers == [0] and new[:, 0].tolist() == [0, 3]
