"""ctypes binding of liblcrec_hip.so -- the C-ABI declared in include/lcrec.h.

The header is the only statement of that ABI: parse_header() derives every signature, plan record and constant from its
text, so an entry point or a field declared there needs nothing added here.

There is no CPU fallback: if the library has not been built (or cannot be
loaded) every entry point raises.  Build it with ``python -c "import
__graft_entry__ as g; g.build()"`` or ``make -C lc-rec_amd/csrc``.
"""
import ctypes
import os
import re

import torch  # noqa: F401  (first, so the HIP runtime torch ships is the one this library binds to)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LCREC_LIB_PATH") or os.path.join(_HERE, "csrc", "liblcrec_hip.so")   # override: diagnostic builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "lcrec.h")


class LcrecError(RuntimeError):
    code = None                      # the LCREC_E* code of a refused library call (check); None: raised by the binding itself


# ---- include/lcrec.h -> ctypes.  The header is plain C of a few forms (below); anything else is an error, never skipped.
_SCALARS = {"int": ctypes.c_int, "unsigned int": ctypes.c_uint, "unsigned char": ctypes.c_ubyte, "char": ctypes.c_char,
            "float": ctypes.c_float, "double": ctypes.c_double, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
            "size_t": ctypes.c_size_t}
_NOT_CODE = re.compile(r"/\*.*?\*/|^#ifdef __cplusplus$.*?^#endif$", re.S | re.M)     # comments, the two extern "C" brackets
_IGNORED_LINE = re.compile(r"#\s*(?:ifndef|endif|include)\b.*|#\s*define\s+\w+")        # the include guard, the includes
_DEFINE = re.compile(r"#\s*define\s+(LCREC_\w+)\s+\(?\s*(-?\w+)\s*\)?")
_FORMS = re.compile(r"\s*(?:enum\s*\{(?P<enum>[^{}]*)\}"
                    r"|typedef\s+struct\s*\{(?P<fields>[^{}]*)\}\s*(?P<struct>lcrec_\w+)"
                    r"|typedef\s+struct\s+(?P<opaque>lcrec_\w+)\s+(?P=opaque)"
                    r"|(?P<ret>[\w\s*]+?)\b(?P<fn>lcrec_\w+)\s*\((?P<params>[^()]*)\))\s*;")


def _integer(text, constants, what):
    try:
        return constants[text] if text in constants else int(text, 0)
    except ValueError:
        raise LcrecError(f"include/lcrec.h: {what}: `{text}` is neither a number nor a constant defined above it") from None


def _declarator(text, base, known, what):
    """`[const] type [*[const]]... name[[length]]`, the type being `base` after a comma -> (type, is pointer, name, length)."""
    m = re.fullmatch(r"(.*?)(\w+)\s*(?:\[\s*(\w+)\s*\])?", text.strip(), re.S)
    stem = " ".join(re.sub(r"\*|\bconst\b", " ", m.group(1)).split()) if m else ""
    if not m or not (stem or base) or (stem and stem not in known):
        raise LcrecError(f"include/lcrec.h: {what}: cannot type `{' '.join(text.split())}`")
    return stem or base, "*" in m.group(1), m.group(2), m.group(3)


def parse_header(text):
    """(constants, structs, signatures) of the text of include/lcrec.h: {LCREC_X: int} from the #defines and enumerators,
    {lcrec_x: ctypes.Structure subclass} in header order, {lcrec_fn: (restype, [argtypes])} in header order.  Every pointer
    is c_void_p, except that a `const char *` field or return is c_char_p.  Raises LcrecError naming the declaration for a
    type outside _SCALARS and the records declared above it, and for file-scope text that is no #define, enum, record or
    prototype."""
    constants, structs, signatures = {}, {}, {}
    known = dict(_SCALARS, void=None)
    lines = _NOT_CODE.sub(lambda m: " " + "\n" * m.group().count("\n"), text).split("\n")
    for i, line in enumerate(lines):
        line = line.strip()
        if line.startswith("#"):
            m = _DEFINE.fullmatch(line)
            if m:
                constants[m.group(1)] = _integer(m.group(2), constants, f"#define {m.group(1)}")
            elif not _IGNORED_LINE.fullmatch(line):
                raise LcrecError(f"include/lcrec.h line {i + 1}: `{line}` is not a form this binding reads")
            lines[i] = ""
    text, pos = "\n".join(lines).rstrip(), 0
    while pos < len(text):
        m = _FORMS.match(text, pos)
        if not m:
            raise LcrecError("include/lcrec.h: not a #define, enum, record or prototype (or its semicolon is missing): `"
                             + " ".join(text[pos:].split(";")[0].split())[:120] + "`")
        pos = m.end()
        if m.group("enum") is not None:
            value = -1
            for item in filter(None, (s.strip() for s in m.group("enum").split(","))):
                name, _, given = (s.strip() for s in item.partition("="))
                value = _integer(given, constants, f"enumerator {name}") if given else value + 1
                constants[name] = value
        elif m.group("struct"):
            name, fields = m.group("struct"), []
            for decl in filter(None, (s.strip() for s in m.group("fields").split(";"))):
                base = None
                for part in decl.split(","):
                    base, pointer, field, length = _declarator(part, base, known, f"{name}, field `{decl}`")
                    ctype = (ctypes.c_char_p if base == "char" else ctypes.c_void_p) if pointer else known[base]
                    if ctype is None:
                        raise LcrecError(f"include/lcrec.h: {name}, field `{decl}`: {base} has no size")
                    fields.append((field, ctype * _integer(length, constants, f"{name}.{field}") if length else ctype))
            structs[name] = known[name] = type(name, (ctypes.Structure,), {"_fields_": fields, "__doc__": f"{name} of include/lcrec.h"})
        elif m.group("opaque"):
            known[m.group("opaque")] = None
        else:
            name, params = m.group("fn"), m.group("params").strip()
            base, pointer, _, _ = _declarator(m.group("ret") + " result", None, known, f"{name}, return type")
            if base != "char" if pointer else base != "void" and base not in _SCALARS:
                raise LcrecError(f"include/lcrec.h: {name}: cannot return `{m.group('ret').strip()}`")
            argtypes = []
            for part in ([] if params == "void" else params.split(",")):
                kind, is_pointer, _, length = _declarator(part, None, known, name)
                if length or not (is_pointer or kind in _SCALARS):
                    raise LcrecError(f"include/lcrec.h: {name}: cannot pass `{' '.join(part.split())}`")
                argtypes.append(ctypes.c_void_p if is_pointer else _SCALARS[kind])
            signatures[name] = (ctypes.c_char_p if pointer else _SCALARS.get(base), argtypes)
    return constants, structs, signatures


try:
    with open(HEADER_PATH) as _f:
        CONSTANTS, STRUCTS, _SIGNATURES = parse_header(_f.read())
except OSError as exc:
    raise LcrecError(f"cannot read {HEADER_PATH}: {exc}") from exc

EXPORTS = tuple(_SIGNATURES)
ABI_VERSION = CONSTANTS["LCREC_ABI_VERSION"]
EUNSUPPORTED = CONSTANTS["LCREC_EUNSUPPORTED"]
MAX_LEVELS = CONSTANTS["LCREC_MAX_LEVELS"]
SK_GROUP_CLASSES = CONSTANTS["LCREC_SK_GROUP_CLASSES"]

DwProblem = STRUCTS["lcrec_dw_problem"]
SinkhornPlan = STRUCTS["lcrec_sinkhorn_plan"]
SinkhornClassPlan = STRUCTS["lcrec_sinkhorn_class_plan"]
SinkhornGroupsPlan = STRUCTS["lcrec_sinkhorn_groups_plan"]
SinkhornGroupRoute = STRUCTS["lcrec_sinkhorn_group_route"]
RqPlan = STRUCTS["lcrec_rq_plan"]
EncodePlan = STRUCTS["lcrec_encode_plan"]
EncodeChunk = STRUCTS["lcrec_encode_chunk"]
DecodePlan = STRUCTS["lcrec_decode_plan"]
BnPlan = STRUCTS["lcrec_bn_plan"]
StepTailPlan = STRUCTS["lcrec_step_tail_plan"]
OptimPlan = STRUCTS["lcrec_optim_plan"]
CollisionPlan = STRUCTS["lcrec_collision_plan"]
IndexTrie = STRUCTS["lcrec_index_trie"]
GemmLaunch = STRUCTS["lcrec_gemm_launch"]
TraceEntry = STRUCTS["lcrec_trace_entry"]

_lib = None


def load():
    """Return the loaded library; raise LcrecError (never fall back) if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LcrecError(
            f"{LIB_PATH} is not built: lcrec_amd has no CPU fallback. "
            "Run `make -C lc-rec_amd/csrc` (hipcc, --offload-arch=gfx950).")
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as exc:
        raise LcrecError(f"cannot load {LIB_PATH}: {exc}") from exc
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.lcrec_version() != ABI_VERSION:
        raise LcrecError(f"ABI version mismatch: library {lib.lcrec_version()}, binding {ABI_VERSION} "
                         "(rebuild: make -C lc-rec_amd/csrc)")
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().lcrec_last_error().decode("utf-8", "replace")
        err = LcrecError(f"{what} failed ({rc}): {msg}")
        err.code = rc
        raise err
