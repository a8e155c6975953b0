"""ctypes binding of liblcrec_hip.so -- the C-ABI declared in include/lcrec.h.

There is no CPU fallback: if the library has not been built (or cannot be
loaded) every entry point raises.  Build it with ``python -c "import
__graft_entry__ as g; g.build()"`` or ``make -C lc-rec_amd/csrc``.
"""
import ctypes
import os

import torch  # noqa: F401  (first, so the HIP runtime torch ships is the one this library binds to)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LCREC_LIB_PATH") or os.path.join(_HERE, "csrc", "liblcrec_hip.so")   # override: diagnostic builds

_f32p = ctypes.c_void_p
_vp = ctypes.c_void_p


class LcrecError(RuntimeError):
    code = None                      # the LCREC_E* code of a refused library call (check); None: raised by the binding itself


EUNSUPPORTED = -2                    # LCREC_EUNSUPPORTED of include/lcrec.h


_SIGNATURES = {
    "lcrec_version": (ctypes.c_int, []),
    "lcrec_last_error": (ctypes.c_char_p, []),
    "lcrec_linear_forward": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_int,
                                            ctypes.c_int, _vp, _vp]),
    "lcrec_linear_backward_splits": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    "lcrec_linear_backward_workspace": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    "lcrec_linear_backward": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp,
                                             ctypes.c_size_t, _vp]),
    "lcrec_linear_backward_weights_workspace": (ctypes.c_size_t, [_vp, ctypes.c_int]),
    "lcrec_linear_backward_weights": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_size_t, _vp]),
    "lcrec_rq_assign_workspace": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                                    ctypes.c_int]),
    "lcrec_context_create": (ctypes.c_int, [ctypes.POINTER(_vp)]),
    "lcrec_context_destroy": (ctypes.c_int, [_vp]),
    "lcrec_context_set_pipelines": (ctypes.c_int, [_vp, ctypes.c_int]),
    "lcrec_rq_assign": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int, _vp, ctypes.POINTER(ctypes.c_int),
                                       ctypes.c_int, _vp, ctypes.c_int64, _vp, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_float,
                                       _vp, ctypes.c_size_t, _vp, _vp]),
    "lcrec_encode_assign_workspace": (ctypes.c_size_t, [ctypes.c_int64, ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                                        ctypes.POINTER(ctypes.c_int), ctypes.c_int]),
    "lcrec_encode_assign_chunk_rows": (ctypes.c_int64, []),
    "lcrec_encode_assign": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                           ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                           ctypes.POINTER(_vp), _vp, ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                           _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_float, _vp, ctypes.c_size_t, _vp,
                                           _vp]),
    "lcrec_sinkhorn_assign_workspace": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int,
                                                          ctypes.POINTER(ctypes.c_int64), ctypes.c_int]),
    "lcrec_sinkhorn_assign": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int, _vp, ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.c_double,
                                             ctypes.c_int, _vp, ctypes.c_int64, _vp, ctypes.c_size_t, _vp, _vp, _vp]),
    "lcrec_rq_apply_level": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int, _vp, ctypes.c_int, _vp,
                                            ctypes.c_int64, _vp, ctypes.c_int, _vp, _vp, _vp, ctypes.c_size_t, _vp, _vp]),
    "lcrec_code_stats": (ctypes.c_int, [_vp, ctypes.c_int64, _vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int,
                                        _vp, _vp, _vp]),
    "lcrec_code_stats_levels": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                               ctypes.c_int, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                               ctypes.POINTER(_vp), ctypes.c_float, ctypes.c_float, _vp]),
    "lcrec_ema_update": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                        ctypes.c_float, ctypes.c_float, ctypes.c_float, _vp, _vp]),
    "lcrec_bn_relu_forward": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int, _vp, _vp, ctypes.c_float, ctypes.c_float, _vp,
                                             _vp, _vp, _vp, _vp, ctypes.c_int, _vp]),
    "lcrec_bn_relu_backward": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int64, ctypes.c_int, _vp, _vp, _vp, ctypes.c_int, _vp,
                                              _vp, _vp, _vp, _vp, _vp, _vp]),
    "lcrec_linear_bn_forward_workspace": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int]),
    "lcrec_linear_bn_forward": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp,
                                               ctypes.c_int, _vp, _vp, ctypes.c_float, ctypes.c_float, _vp, _vp, _vp, _vp, _vp, _vp,
                                               _vp, ctypes.c_size_t, _vp, _vp]),
    "lcrec_bn_stats": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int, _vp, _vp, _vp]),
    "lcrec_bn_relu_apply": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_int, _vp, _vp]),
    "lcrec_bn_backward_reduce": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int64, ctypes.c_int, _vp, _vp, ctypes.c_int, _vp, _vp, _vp, _vp,
                                                _vp]),
    "lcrec_bn_merge_stats": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, _vp, _vp, _vp, _vp, _vp]),
    "lcrec_bn_backward_apply": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int64, ctypes.c_int, _vp, _vp, _vp, ctypes.c_int, _vp, _vp,
                                               ctypes.c_float, _vp, _vp, _vp]),
    "lcrec_relu_bias_backward": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]),
    "lcrec_train_reduce_workspace": (ctypes.c_size_t, []),
    "lcrec_recon_loss_grad": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, _vp, _vp, _vp, ctypes.c_size_t, _vp,
                                             _vp]),
    "lcrec_grad_norm_clip": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_float, _vp, _vp, ctypes.c_size_t, _vp, _vp]),
    "lcrec_codebook_grad": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, _vp, _vp]),
    "lcrec_step_losses": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_float, _vp, _vp, _vp,
                                         _vp, _vp, _vp, _vp]),
    "lcrec_quantizer_input_grad": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_float,
                                                  ctypes.c_float, _vp, _vp, _vp]),
    "lcrec_quantizer_input_grad_bias": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.c_float,
                                                       ctypes.c_float, _vp, _vp, _vp, _vp]),
    "lcrec_adamw_step": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int64, _vp, _vp, ctypes.c_double, ctypes.c_double,
                                        ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int64, ctypes.c_int64, _vp, _vp, _vp, _vp]),
    "lcrec_sgd_step": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int64, _vp, _vp, ctypes.c_double, ctypes.c_double,
                                      ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int64, ctypes.c_int64,
                                      _vp, _vp, _vp, _vp]),
    "lcrec_adagrad_step": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int64, _vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                          ctypes.c_double, ctypes.c_int, ctypes.c_int64, ctypes.c_int64, _vp, _vp, _vp, _vp]),
    "lcrec_rmsprop_step": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_int64, _vp, _vp, ctypes.c_double, ctypes.c_double,
                                          ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int64,
                                          ctypes.c_int64, _vp, _vp, _vp, _vp]),
    "lcrec_dropout_apply": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, ctypes.c_uint32, ctypes.c_float, _vp, _vp, ctypes.c_int,
                                           ctypes.c_int64, _vp]),
    "lcrec_dropout_mask": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int, ctypes.c_uint32, _vp, _vp, ctypes.c_int, ctypes.c_int64, _vp]),
    "lcrec_cast_rows": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int64, _vp, _vp]),
    "lcrec_collision_groups_workspace": (ctypes.c_size_t, [ctypes.c_int64, ctypes.c_int]),
    "lcrec_collision_groups": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int), _vp,
                                              _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "lcrec_finish_nearest_free": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int), _vp, ctypes.c_int, _vp,
                                                 _vp, _vp, ctypes.c_int64, _vp, _vp]),
    "lcrec_extend_nearest_free": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int), _vp,
                                                 ctypes.c_int, _vp, _vp, _vp, ctypes.c_int64, _vp, _vp]),
    "lcrec_spill_nearest_free_workspace": (ctypes.c_size_t, [ctypes.c_int64]),
    "lcrec_spill_nearest_free": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int), _vp, _vp,
                                                ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_int64, _vp, _vp, ctypes.c_int64, _vp, _vp,
                                                ctypes.c_size_t, _vp]),
    "lcrec_index_json_bound": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int]),
    "lcrec_index_json_format": (ctypes.c_int64, [_vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int64, _vp, ctypes.c_int64]),
    "lcrec_index_json_parse": (ctypes.c_int64, [_vp, ctypes.c_int64, ctypes.c_int, _vp, ctypes.c_int64]),
    "lcrec_trace_enable": (ctypes.c_int, [ctypes.c_int]),
    "lcrec_trace_collect": (ctypes.c_int, [_vp, ctypes.c_int]),
    "lcrec_debug_sinkhorn_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp]),
    "lcrec_debug_sinkhorn_batch": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_double, ctypes.c_int,
                                                  _vp, ctypes.c_int64, _vp, ctypes.c_size_t, _vp, _vp, ctypes.c_int, _vp, _vp,
                                                  ctypes.POINTER(ctypes.c_int)]),
    "lcrec_debug_sinkhorn_groups_plan": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.c_int, _vp, _vp]),
    "lcrec_debug_sinkhorn_groups": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int, _vp, ctypes.c_int,
                                                   ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.c_double,
                                                   ctypes.c_int, _vp, ctypes.c_int64, _vp, ctypes.c_size_t, _vp, _vp, _vp, _vp, _vp]),
    "lcrec_debug_rq_assign_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int,
                                                  ctypes.c_int, ctypes.c_int, _vp]),
    "lcrec_debug_rq_assign": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int, _vp, ctypes.POINTER(ctypes.c_int),
                                             ctypes.c_int, _vp, ctypes.c_int64, _vp, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_float,
                                             _vp, ctypes.c_size_t, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "lcrec_debug_bn_plan": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, _vp]),
    "lcrec_debug_step_tail_plan": (ctypes.c_int, [ctypes.c_int, ctypes.c_int64, ctypes.c_int, ctypes.c_int, _vp]),
    "lcrec_debug_linear_forward_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int]),
    "lcrec_debug_linear_backward_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp,
                                                        ctypes.c_int]),
    "lcrec_debug_linear_backward_weights_plan": (ctypes.c_int, [_vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]),
    "lcrec_debug_linear_bn_forward_plan": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp]),
}


class DwProblem(ctypes.Structure):
    """lcrec_dw_problem of include/lcrec.h"""
    _fields_ = [("gy", ctypes.c_void_p), ("x", ctypes.c_void_p), ("gw", ctypes.c_void_p), ("n", ctypes.c_int64),
                ("in_dim", ctypes.c_int), ("out_dim", ctypes.c_int), ("x_scale", ctypes.c_void_p), ("x_shift", ctypes.c_void_p),
                ("x_relu", ctypes.c_int), ("splits", ctypes.c_int)]


class SinkhornPlan(ctypes.Structure):
    """lcrec_sinkhorn_plan of include/lcrec.h"""
    _fields_ = [("form", ctypes.c_int), ("cpl", ctypes.c_int), ("rw", ctypes.c_int), ("workgroups", ctypes.c_int),
                ("sets", ctypes.c_int), ("rows_per_workgroup", ctypes.c_int), ("padded_columns", ctypes.c_int),
                ("ragged_wave", ctypes.c_int), ("ragged_workgroup", ctypes.c_int), ("batch_route", ctypes.c_int),
                ("workspace_bytes", ctypes.c_int64)]


SK_GROUP_CLASSES = 5                 # LCREC_SK_GROUP_CLASSES of include/lcrec.h


class SinkhornClassPlan(ctypes.Structure):
    """lcrec_sinkhorn_class_plan of include/lcrec.h"""
    _fields_ = [("groups", ctypes.c_int), ("maxg", ctypes.c_int), ("lds_bytes", ctypes.c_int64), ("set_attribute", ctypes.c_int),
                ("threads", ctypes.c_int), ("table_first", ctypes.c_int), ("label", ctypes.c_char_p)]


class SinkhornGroupsPlan(ctypes.Structure):
    """lcrec_sinkhorn_groups_plan of include/lcrec.h"""
    _fields_ = [("cls", SinkhornClassPlan * SK_GROUP_CLASSES), ("slab_ok", ctypes.c_int), ("slab_doubles", ctypes.c_int64),
                ("batch_groups", ctypes.c_int), ("batch_biggest", ctypes.c_int64), ("table_groups", ctypes.c_int),
                ("transport", ctypes.c_int), ("fork_mask", ctypes.c_int), ("workspace_bytes", ctypes.c_int64)]


class SinkhornGroupRoute(ctypes.Structure):
    """lcrec_sinkhorn_group_route of include/lcrec.h"""
    _fields_ = [("cls", ctypes.c_int), ("position", ctypes.c_int), ("slab_offset", ctypes.c_int64)]


MAX_LEVELS = 16                      # LCREC_MAX_LEVELS of include/lcrec.h


class RqPlan(ctypes.Structure):
    """lcrec_rq_plan of include/lcrec.h"""
    _fields_ = [("split", ctypes.c_int), ("threads", ctypes.c_int), ("grid", ctypes.c_int), ("tiles", ctypes.c_int64),
                ("trips_max", ctypes.c_int64), ("trips_min", ctypes.c_int64), ("launches", ctypes.c_int),
                ("l0", ctypes.c_int * MAX_LEVELS), ("l1", ctypes.c_int * MAX_LEVELS), ("rows", ctypes.c_int * MAX_LEVELS),
                ("lds_bytes", ctypes.c_int64 * MAX_LEVELS), ("row_off", ctypes.c_int * MAX_LEVELS),
                ("blocks_per_wave", ctypes.c_int * MAX_LEVELS), ("idle_waves", ctypes.c_int * MAX_LEVELS),
                ("handover_reuse", ctypes.c_int)]


class BnPlan(ctypes.Structure):
    """lcrec_bn_plan of include/lcrec.h"""
    _fields_ = [("float4", ctypes.c_int), ("cols", ctypes.c_int), ("rows_per_lane", ctypes.c_int), ("cached", ctypes.c_int), ("grid", ctypes.c_int),
                ("xcd_order", ctypes.c_int)]


class StepTailPlan(ctypes.Structure):
    """lcrec_step_tail_plan of include/lcrec.h"""
    _fields_ = [("K", ctypes.c_int), ("family", ctypes.c_int), ("grid", ctypes.c_int), ("grid_sse", ctypes.c_int), ("cols", ctypes.c_int),
                ("xcd_order", ctypes.c_int), ("vec16", ctypes.c_int), ("second_launch", ctypes.c_int), ("tail", ctypes.c_int64)]


class GemmLaunch(ctypes.Structure):
    """lcrec_gemm_launch of include/lcrec.h"""
    _fields_ = [("label", ctypes.c_char_p), ("role", ctypes.c_int), ("family", ctypes.c_int), ("tile_rows", ctypes.c_int),
                ("tile_cols", ctypes.c_int), ("fast", ctypes.c_int), ("a_kmajor", ctypes.c_int), ("w_kmajor", ctypes.c_int),
                ("pro", ctypes.c_int), ("stats", ctypes.c_int), ("register_buffered", ctypes.c_int), ("m", ctypes.c_int64),
                ("n", ctypes.c_int), ("k", ctypes.c_int), ("k_tiles", ctypes.c_int), ("runs", ctypes.c_int),
                ("k_tiles_per_run", ctypes.c_int), ("k_tiles_last_run", ctypes.c_int), ("last_k_valid", ctypes.c_int),
                ("tiles", ctypes.c_int), ("virtual_tiles", ctypes.c_int), ("workgroups", ctypes.c_int), ("wg_start", ctypes.c_int),
                ("last_panel_rows", ctypes.c_int), ("last_tile_cols", ctypes.c_int), ("vector_stores", ctypes.c_int),
                ("chunk_row_tiles", ctypes.c_int), ("chunks", ctypes.c_int), ("total4", ctypes.c_int64), ("row0", ctypes.c_int64),
                ("form", ctypes.c_int), ("steady_iterations", ctypes.c_int), ("list_min", ctypes.c_int), ("list_max", ctypes.c_int),
                ("empty_workgroups", ctypes.c_int), ("single_tile_workgroups", ctypes.c_int), ("ragged_handed_over", ctypes.c_int)]


class TraceEntry(ctypes.Structure):
    _fields_ = [("kernel", ctypes.c_char_p), ("launches", ctypes.c_int64), ("total_ms", ctypes.c_double)]


EXPORTS = tuple(_SIGNATURES)
ABI_VERSION = 3                      # LCREC_ABI_VERSION of include/lcrec.h this binding was written against

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
