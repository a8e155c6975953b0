"""CPU: the ctypes binding derives everything from include/lcrec.h (lcrec_amd/_lib.py parse_header).  The C compiler is the
reference for every record's layout; damaged copies of the header text show that the parser refuses what it cannot type and
follows what changes; the name tables of ops.py are tied to the header's enumerators; linear_bn_supported asks the library and
answers as the rule it used to restate."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def binding():
    import lcrec_amd
    return lcrec_amd._lib


@pytest.fixture(scope="module")
def header():
    return open(os.path.join(ROOT, "include", "lcrec.h")).read()


def damaged(header, old, new):
    assert header.count(old) == 1, old
    return header.replace(old, new)


def test_records_have_the_layout_the_c_compiler_gives_them(binding, tmp_path):
    """sizeof of every record and offsetof / sizeof of every field, as the oracle's C compiler lays out include/lcrec.h, against
    the derived ctypes classes: exact.  The field list is the derived classes' own, so a new record is covered as it is declared."""
    lines = []
    for name, cls in binding.STRUCTS.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name} *)0)->{f}));' for f, _ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "lcrec.h"\nint main(void)\n{\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CC", "cc"), "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = {key: tuple(map(int, rest)) for key, *rest in (l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())}
    want = {}
    for name, cls in binding.STRUCTS.items():
        want[name] = (ctypes.sizeof(cls),)
        want.update({f"{name}.{f}": (getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_})
    assert len(binding.STRUCTS) >= 13 and sum(len(c._fields_) for c in binding.STRUCTS.values()) >= 133
    assert got == want


def test_constants_follow_c(binding, header):
    """#defines with and without parentheses, enumerators with C's numbering."""
    c = binding.parse_header(header)[0]
    assert (c["LCREC_ABI_VERSION"], c["LCREC_OK"], c["LCREC_EINVAL"], c["LCREC_EHIP"], c["LCREC_MAX_LEVELS"]) == (3, 0, -1, -4, 16)
    assert (c["LCREC_DTYPE_F16"], c["LCREC_DTYPE_F64"], c["LCREC_SK_GROUP_CLASSES"]) == (1, 2, 5)
    assert (c["LCREC_ENC_PIPES_MAX"], c["LCREC_ENC_ACT_BUFFERS"]) == (2, 4)
    assert (c["LCREC_SK_TABLE_SYNCHRONOUS"], c["LCREC_BN_BACKWARD_APPLY"], c["LCREC_TAILK_CS_PER_LEVEL"], c["LCREC_GEMMR_FORWARD"]) == (3, 4, 8, 3)
    c = binding.parse_header(damaged(header, "LCREC_GEMMK_32x64,", "LCREC_GEMMK_32x64 = 0x10,"))[0]
    assert (c["LCREC_GEMMK_TILE_BODY"], c["LCREC_GEMMK_32x64"], c["LCREC_GEMMK_REDUCER"], c["LCREC_GEMMK_PP"]) == (0, 16, 17, 18)
    assert binding.ABI_VERSION == 3 and binding.EUNSUPPORTED == -2 and binding.MAX_LEVELS == 16 and binding.SK_GROUP_CLASSES == 5


@pytest.mark.parametrize("old,new,named", [
    ("int src_dtype", "long double src_dtype", "lcrec_cast_rows"),                      # a parameter type outside the table
    ("int rows_per_lane;", "short rows_per_lane;", "lcrec_bn_plan"),                    # a field of unknown type
    ("int row_off[LCREC_MAX_LEVELS];", "int row_off[LCREC_NO_SUCH];", "lcrec_rq_plan"),  # an array length that is no constant
    ("int row_off[LCREC_MAX_LEVELS];", "int row_off[2 * 8];", "lcrec_rq_plan"),         # ... nor a number
    ("int lcrec_version(void);", "int lcrec_version(void)", "lcrec_version"),           # a prototype without its semicolon
    ("size_t lcrec_train_reduce_workspace(void);", "ssize_t lcrec_train_reduce_workspace(void);", "lcrec_train_reduce_workspace"),
    ("int lcrec_trace_enable(int on);", "int lcrec_trace_enable(int on);\nstatic int lcrec_helper = 3;", "lcrec_helper"),
    ("#define LCREC_MAX_LAYERS 16", "#define LCREC_MAX_LAYERS (LCREC_MAX_LEVELS + 0)", "LCREC_MAX_LAYERS"),
    ("#define LCREC_MAX_LAYERS 16", "#pragma pack(4)", "pragma"),
])
def test_what_the_parser_cannot_type_is_an_error_naming_the_declaration(binding, header, old, new, named):
    with pytest.raises(binding.LcrecError) as err:
        binding.parse_header(damaged(header, old, new))
    assert named in str(err.value) and "lcrec.h" in str(err.value)


def test_the_result_follows_the_header(binding, header):
    """An extra parameter, a widened parameter and a field inserted mid-record each move exactly what they should."""
    _, structs, sigs = binding.parse_header(header)
    assert tuple(sigs) == binding.EXPORTS and len(sigs) >= 73
    res, args = sigs["lcrec_cast_rows"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    assert sigs["lcrec_last_error"] == (ctypes.c_char_p, []) and sigs["lcrec_context_create"] == (ctypes.c_int, [ctypes.c_void_p])
    assert sigs["lcrec_rq_assign_workspace"] == (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_int])
    assert sigs["lcrec_debug_encode_assign_workspace"] == (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                                             ctypes.c_int, ctypes.c_int64])
    assert sigs["lcrec_debug_encode_assign"][1] == sigs["lcrec_encode_assign"][1] + [ctypes.c_int64]
    assert [f for f, _ in structs["lcrec_encode_chunk"]._fields_] == ["row0", "rows", "pipeline", "first_act"]
    assert ctypes.sizeof(structs["lcrec_encode_plan"]) == 8 * (10 + binding.CONSTANTS["LCREC_ENC_ACT_BUFFERS"])

    more = binding.parse_header(damaged(header, "float *dst, void *hip_stream);", "float *dst, void *hip_stream, uint32_t flags);"))[2]
    assert more["lcrec_cast_rows"] == (res, args + [ctypes.c_uint32])
    wide = binding.parse_header(damaged(header, "int src_dtype", "int64_t src_dtype"))[2]
    assert wide["lcrec_cast_rows"] == (res, args[:1] + [ctypes.c_int64] + args[2:])
    assert all(more[n] == sigs[n] and wide[n] == sigs[n] for n in sigs if n != "lcrec_cast_rows")

    was = structs["lcrec_bn_plan"]
    now = binding.parse_header(damaged(header, "int rows_per_lane;", "int64_t inserted; int rows_per_lane;"))[1]["lcrec_bn_plan"]
    assert [f for f, _ in now._fields_] == ["float4", "cols", "inserted", "rows_per_lane", "cached", "grid", "xcd_order"]
    assert [(getattr(was, f).offset, getattr(now, f).offset) for f, _ in was._fields_] == [(0, 0), (4, 4), (8, 16), (12, 20), (16, 24), (20, 28)]
    assert (ctypes.sizeof(was), ctypes.sizeof(now)) == (24, 32)


def test_a_new_enumerator_without_a_name_is_refused_at_import(binding, header):
    """ops._check_names is what `import lcrec_amd.ops` runs on the header's constants."""
    from lcrec_amd import ops
    ops._check_names(binding.parse_header(header)[0])
    more = binding.parse_header(damaged(header, "LCREC_TAILK_CS_PER_LEVEL ", "LCREC_TAILK_CS_PER_LEVEL, LCREC_TAILK_NEW_FORM "))[0]
    assert more["LCREC_TAILK_NEW_FORM"] == len(ops.TAIL_FAMILIES)
    with pytest.raises(binding.LcrecError, match="TAIL_FAMILIES"):
        ops._check_names(more)
    with pytest.raises(binding.LcrecError, match="SK_TABLE_TRANSPORTS"):       # renumbered, not added
        ops._check_names(binding.parse_header(damaged(header, "LCREC_SK_TABLE_RING = 2", "LCREC_SK_TABLE_RING = 4"))[0])


def test_the_capturable_forms_refuse_a_wrong_counters_out_or_workspace_before_the_call(binding):
    """counters_out (finish / extend / spill_nearest_free) and workspace (spill_nearest_free, rq_audit_into) are checked by the two
    helpers below against the device of the call -- here the CPU stands in for it, so that no GPU is needed: wrong dtype, wrong
    shape, wrong device, not contiguous and a workspace one byte too small are each an LcrecError of the binding's own, raised
    before the library is called (its last-error text does not change)."""
    import inspect

    import torch

    from lcrec_amd import ops
    lib = binding.load()
    before = lib.lcrec_last_error()
    here, elsewhere = torch.device("cpu"), "meta"
    for f, names in ((ops.finish_nearest_free, ("counters_out",)), (ops.extend_nearest_free, ("counters_out",)),
                     (ops.spill_nearest_free, ("counters_out", "workspace")), (ops.rq_audit_into, ("workspace",)),
                     (ops.rq_beam_into, ("workspace",))):
        params = inspect.signature(f).parameters
        assert all(params[name].default is None for name in names), f.__name__
        assert all(name in f.__doc__ for name in names), f.__name__

    mine = torch.zeros(2, dtype=torch.int64)
    assert ops._counters_out(mine, here) is mine                                      # passed through as it is
    fresh = ops._counters_out(None, here)
    assert fresh.dtype == torch.int64 and tuple(fresh.shape) == (2,)
    for bad in (torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.float64), torch.zeros(3, dtype=torch.int64),
                torch.zeros((1, 2), dtype=torch.int64), torch.zeros(4, dtype=torch.int64)[::2],
                torch.zeros(2, dtype=torch.int64, device=elsewhere), [0, 0], 0):
        with pytest.raises(binding.LcrecError, match="counters_out must be a contiguous int64 \\[2\\] tensor"):
            ops._counters_out(bad, here)

    need = lib.lcrec_spill_nearest_free_workspace(218)
    assert need == 256 and lib.lcrec_rq_audit_workspace(257, 16, ops._ints([48, 100, 7]), 3) == 16640
    ws = torch.zeros(need, dtype=torch.uint8)
    assert ops._own_workspace(ws, here, need, "q") is ws and ops._own_workspace(ws, here, 0, "q") is ws
    for bad in (torch.zeros(need, dtype=torch.int8), torch.zeros(need // 4, dtype=torch.float32), torch.zeros(2 * need, dtype=torch.uint8)[::2],
                torch.zeros(need, dtype=torch.uint8, device=elsewhere), bytearray(need)):
        with pytest.raises(binding.LcrecError, match="workspace must be a contiguous uint8 tensor"):
            ops._own_workspace(bad, here, need, "q")
    with pytest.raises(binding.LcrecError, match=r"workspace of 255 bytes, 256 needed \(lcrec_spill_nearest_free_workspace\)"):
        ops._own_workspace(ws[:255], here, need, "lcrec_spill_nearest_free_workspace")
    # the entries themselves refuse what is not on a device before anything else
    idx, r, cb = torch.zeros((4, 2), dtype=torch.int64), torch.zeros((4, 16)), torch.zeros((8, 16))
    table = (torch.zeros(0, dtype=torch.int64), torch.zeros(1, dtype=torch.int64))
    for call in (lambda: ops.finish_nearest_free(idx, r, cb, [2, 8], *table, counters_out=mine),
                 lambda: ops.extend_nearest_free(idx, 0, r, cb, [2, 8], *table, counters_out=mine),
                 lambda: ops.spill_nearest_free(idx, 0, r, r, cb, cb, [8, 8], table, table, counters_out=mine, workspace=ws),
                 lambda: ops.rq_audit_into(r, cb, [8], idx[:, :1], {}, workspace=ws)):
        with pytest.raises(binding.LcrecError, match="device"):
            call()
    assert lib.lcrec_last_error() == before


def test_linear_bn_supported_answers_as_the_rule_it_restated(binding):
    """The Python expression linear_bn_supported was before it asked the library, as the reference, on a grid around every bound."""
    from lcrec_amd import ops
    binding.load()

    def rule(n, in_dim, out_dim):
        return (n >= 2 and in_dim % 32 == 0 and out_dim % 4 == 0 and out_dim <= 4096
                and ((n + 127) // 128) * ((out_dim + 127) // 128) < 512 and in_dim * 4 * (n + 128) < (1 << 31))

    grid = [(n, k, f) for n in (1, 2, 127, 128, 129, 2048, 65536, 131072) for k in (24, 32, 40, 768, 4096, 1 << 22)
            for f in (2, 4, 62, 64, 4096, 4100)]
    before = binding.load().lcrec_last_error()
    got = {p: ops.linear_bn_supported(*p) for p in grid}
    assert binding.load().lcrec_last_error() == before            # a refused question is no error of the asking thread's
    assert all(type(v) is bool for v in got.values())
    assert got == {p: rule(*p) for p in grid}
    assert 0 < sum(got.values()) < len(grid)
