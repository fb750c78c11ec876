"""ctypes binding of libntt_mi355x.so -- the MI355X-native negacyclic NTT engine.

The product is the C-ABI shared library built from ``csrc/`` (HIP kernels for
gfx950 + a C host layer); this module is only a thin binding so that the Python
test-suite and ``bench.py`` can call it.  It mirrors the library's two surfaces:

* the batched, device-resident plan API of ``include/ntt_mi355x.h``
  (``Plan.fwd`` / ``Plan.inv`` / ``Plan.pointwise_mul`` / ``Plan.negacyclic_mul``);
* the reference's single-polynomial signatures on host arrays
  (``fwd_ntt_ref_harvey``, ``inv_ntt_ref_harvey``, ``fwd_ntt_radix4``,
  ``inv_ntt_radix4``, ``fwd_ntt_radix4x4``, ``fwd_ntt_ref_harvey_dbl``), which
  behave like reference include/ntt_reference.h:13-65, ntt_radix4.h:10-35 and
  ntt_radix4x4.h:10-28.

There is no CPU fallback: if the shared library is missing the import fails,
and without a HIP device every compute call raises ``NttError``.

The directory name contains hyphens (it is fixed by the project layout), so
import it with ``importlib`` -- see ``load()`` in the repository's ``ontt.py``.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NTT_LIB") or os.path.join(_HERE, "libntt_mi355x.so")  # NTT_LIB: A/B builds of the same library

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "libntt_mi355x.so is not built (run `make lib` or __graft_entry__.build()); "
        "there is no pure-Python or CPU fallback for the NTT kernels")

_lib = C.CDLL(LIB_PATH, mode=C.RTLD_LOCAL)

U64P = C.POINTER(C.c_uint64)
VOIDP = C.c_void_p

NTT_OK = 0
ARITH_AUTO, ARITH_U64, ARITH_F64, ARITH_U64_R4 = 0, 1, 2, 3
FLAG_INVERSE, FLAG_WIDE_IN, FLAG_LAZY_OUT = 1, 2, 4
MUL_LAZY_IN, MUL_B_BROADCAST, MUL_ACCUMULATE = 1, 2, 4
OPT_MAX_GRID, OPT_CHUNK_MIB, OPT_F64_CLASS, OPT_TWO_PHASE, OPT_FUSED_PRODUCT, OPT_BLOCK_LOG = 1, 2, 3, 4, 5, 6
OPT_XCD_LOCAL, OPT_XCD_LOCAL_LAG, OPT_XCD_LOCAL_WGS_PER_CU, OPT_INT_WIDE, OPT_BLOCK_OVERSUB = 7, 8, 9, 10, 11
OPT_RNS_LAUNCH, OPT_DOT_FUSED, OPT_MAX_BATCH_HINT, OPT_CTL_ALLOCATIONS, OPT_ONE_PASS = 12, 13, 14, 15, 16
OPT_RESCALE_FUSED = 17
OPT_MODUP_FUSED = 18
OPT_PAIR_FUSED = 19
OPT_MODDOWN_ADD_FUSED = 20
OPT_BGV_FUSED = 21
OPT_LIFT_FUSED = 22
OPT_SLOTS_FUSED = 23
OPT_SAMPLE_FUSED = 24
RESCALE_TRANSFORMED, RESCALE_FLOOR = 1, 2
MODUP_TRANSFORMED = 1
MODDOWN_TRANSFORMED, MODDOWN_FLOOR, MODDOWN_ACCUMULATE = 1, 2, 4
GALOIS_TRANSFORMED, GALOIS_ACCUMULATE, GALOIS_KEY_BROADCAST = 1, 2, 4
LINCOMB_ACCUMULATE, LINCOMB_M_BROADCAST, LINCOMB_LAZY_IN = 1, 2, 4
PLAIN_SCALE = 1
LIFT_SCALE, LIFT_TRANSFORMED, LIFT_ACCUMULATE = 1, 2, 4
SAMPLE_TERNARY, SAMPLE_CBD21, SAMPLE_UNIFORM = 0, 1, 2
SAMPLE_TRANSFORMED, SAMPLE_ACCUMULATE = 2, 4

#: every symbol include/ntt_mi355x.h and the reference-named headers declare
EXPORTED_SYMBOLS = [
    "ntt_last_error", "ntt_device_count", "ntt_version", "ntt_plan_create",
    "ntt_plan_create_from_tables", "ntt_plan_destroy", "ntt_plan_info", "ntt_plan_set_generic", "ntt_plan_set_option", "ntt_plan_get_option", "ntt_plan_reserve", "ntt_plan_export_table",
    "ntt_fwd_batch", "ntt_inv_batch", "ntt_fwd_batch_wide", "ntt_inv_batch_wide",
    "ntt_fwd_batch_lazy", "ntt_inv_batch_lazy", "ntt_transform_batch",
    "ntt_pointwise_mul_batch", "ntt_pointwise_mul_batch_lazy", "ntt_negacyclic_mul_batch", "ntt_rns_fwd_batch", "ntt_rns_inv_batch",
    "ntt_rns_negacyclic_mul_batch", "ntt_inv_product_batch", "ntt_inv_dot_batch", "ntt_mul_transformed_batch",
    "ntt_rns_inv_dot_batch", "ntt_rns_mul_transformed_batch", "ntt_fwd_mul_batch", "ntt_rns_fwd_mul_batch",
    "ntt_rns_fwd_batch_strided", "ntt_rns_inv_batch_strided", "ntt_rns_negacyclic_mul_batch_strided", "ntt_rns_inv_dot_batch_strided",
    "ntt_rns_mul_transformed_batch_strided", "ntt_rns_fwd_mul_batch_strided", "ntt_rns_rescale_batch", "ntt_rns_rescale_batch_strided",
    "ntt_rns_mod_up_batch", "ntt_rns_mod_up_batch_strided", "ntt_rns_mod_down_batch", "ntt_rns_mod_down_batch_strided",
    "ntt_rns_mod_up_mul_batch", "ntt_rns_mod_up_mul_batch_strided",
    "ntt_rns_fwd_mul_pair_batch", "ntt_rns_fwd_mul_pair_batch_strided", "ntt_rns_mod_up_mul_pair_batch", "ntt_rns_mod_up_mul_pair_batch_strided",
    "ntt_rns_galois_dot_pair_batch", "ntt_rns_galois_dot_pair_batch_strided",
    "ntt_rns_tensor_batch", "ntt_rns_tensor_batch_strided", "ntt_rns_mod_down_add_batch", "ntt_rns_mod_down_add_batch_strided",
    "ntt_rns_mod_up_exact_batch", "ntt_rns_mod_up_exact_batch_strided", "ntt_rns_mod_down_exact_batch", "ntt_rns_mod_down_exact_batch_strided",
    "ntt_rns_mod_down_bgv_batch", "ntt_rns_mod_down_bgv_batch_strided", "ntt_rns_mod_down_bgv_add_batch", "ntt_rns_mod_down_bgv_add_batch_strided",
    "ntt_galois_rotation", "ntt_galois_batch", "ntt_rns_galois_batch", "ntt_rns_galois_batch_strided", "ntt_rns_galois_dot_batch",
    "ntt_rns_galois_dot_batch_strided", "ntt_rns_lincomb_batch", "ntt_rns_lincomb_batch_strided",
    "ntt_rns_to_plain_batch", "ntt_rns_to_plain_batch_strided", "ntt_rns_to_double_batch", "ntt_rns_to_double_batch_strided",
    "ntt_rns_from_plain_batch", "ntt_rns_from_plain_batch_strided", "ntt_rns_from_double_batch", "ntt_rns_from_double_batch_strided",
    "ntt_rns_sample_batch", "ntt_rns_sample_batch_strided",
    "ntt_plan_enable_slots", "ntt_slot_position", "ntt_slots_encode_batch", "ntt_slots_encode_batch_strided", "ntt_slots_decode_batch",
    "ntt_slots_decode_batch_strided",
    "ntt_transform_batch_strided", "ntt_transform_ptrs", "ntt_rns_transform_ptrs", "ntt_transform_dev_ptrs", "ntt_rns_transform_dev_ptrs", "ntt_inv_dot_dev_ptrs", "ntt_fwd_mul_dev_ptrs", "ntt_negacyclic_mul_dev_ptrs",
    "ntt_rns_inv_dot_dev_ptrs", "ntt_rns_fwd_mul_dev_ptrs", "ntt_rns_negacyclic_mul_dev_ptrs", "ntt_dev_malloc", "ntt_dev_free", "ntt_dev_mem_info",
    "ntt_h2d", "ntt_d2h", "ntt_stream_create", "ntt_stream_destroy", "ntt_stream_sync",
    "ntt_event_create", "ntt_event_destroy", "ntt_event_record", "ntt_event_elapsed_ms",
    "ntt_fill_uniform", "ntt_poly_checksum", "ntt_rmw_probe", "ntt_shape_probe", "ntt_copy_probe", "ntt_batch_multi", "ntt_rns_mul_multi", "ntt_min_root", "ntt_find_prime",
    "ntt_compat_release", "ntt_compat_cached_plans",
    # reference signatures (include/ntt_reference.h, ntt_radix4.h, ntt_radix4x4.h, ntt_seal.h)
    "fwd_ntt_ref_harvey_lazy", "inv_ntt_ref_harvey", "fwd_ntt_ref_harvey_lazy_dbl",
    "fwd_ntt_radix4_lazy", "inv_ntt_radix4", "fwd_ntt_radix4x4_lazy", "fwd_ntt_seal_lazy",
    "inv_ntt_seal",
]


class NttError(RuntimeError):
    pass


class MulOp(C.Structure):
    """reference mul_op_t: two __uint128_t, passed by value (fast_mul_operators.h:10-13).

    __uint128_t is 16-byte aligned and ctypes has no 128-bit integer: the zero-length long double array
    contributes nothing but its 16-byte alignment, so libffi places the by-value copy where the C callee
    expects it even when other stack arguments precede it (tests/test_abi.py::test_mul_op_by_value_through_ctypes)."""
    _fields_ = [("_align16", C.c_longdouble * 0),
                ("op_lo", C.c_uint64), ("op_hi", C.c_uint64), ("con_lo", C.c_uint64), ("con_hi", C.c_uint64)]


def _sig(name, restype, *argtypes):
    if "NTT_LIB" in os.environ and not hasattr(_lib, name):
        return None   # an older build selected for a same-box A/B (tools/build_head.sh): entry points added since are simply absent
    f = getattr(_lib, name)
    f.restype = restype
    f.argtypes = list(argtypes)
    return f


_sig("ntt_last_error", C.c_char_p)
_sig("ntt_version", C.c_char_p)
_sig("ntt_device_count", C.c_int)
_sig("ntt_plan_create", C.c_int, C.POINTER(VOIDP), C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int)
_sig("ntt_plan_create_from_tables", C.c_int, C.POINTER(VOIDP), C.c_int, C.c_uint64, C.c_uint64, U64P, U64P, C.c_int)
_sig("ntt_plan_destroy", None, VOIDP)
_sig("ntt_plan_info", C.c_int, VOIDP, U64P)
_sig("ntt_plan_set_generic", C.c_int, VOIDP, C.c_int)
_sig("ntt_plan_set_option", C.c_int, VOIDP, C.c_int, C.c_int64)
_sig("ntt_plan_reserve", C.c_int, VOIDP, VOIDP, C.c_uint64)
_sig("ntt_plan_get_option", C.c_int, VOIDP, C.c_int, C.POINTER(C.c_int64))
_sig("ntt_plan_export_table", C.c_int, VOIDP, C.c_int, VOIDP, C.c_size_t)
_sig("ntt_plan_enable_slots", C.c_int, VOIDP)
_sig("ntt_slot_position", C.c_uint64, C.c_uint64, C.c_uint64)
for _n in ("ntt_slots_encode_batch", "ntt_slots_decode_batch"):
    _sig(_n, C.c_int, VOIDP, VOIDP, VOIDP, C.c_uint64, C.c_uint, VOIDP)
    _sig(_n + "_strided", C.c_int, VOIDP, VOIDP, VOIDP, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint, VOIDP)
for _n in ("ntt_fwd_batch", "ntt_inv_batch", "ntt_fwd_batch_wide", "ntt_inv_batch_wide", "ntt_fwd_batch_lazy",
           "ntt_inv_batch_lazy"):
    _sig(_n, C.c_int, VOIDP, VOIDP, C.c_uint64, VOIDP)
_sig("ntt_transform_batch", C.c_int, VOIDP, VOIDP, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_pointwise_mul_batch", C.c_int, VOIDP, VOIDP, VOIDP, VOIDP, C.c_uint64, VOIDP)
_sig("ntt_pointwise_mul_batch_lazy", C.c_int, VOIDP, VOIDP, VOIDP, VOIDP, C.c_uint64, VOIDP)
_sig("ntt_negacyclic_mul_batch", C.c_int, VOIDP, VOIDP, VOIDP, VOIDP, C.c_uint64, VOIDP)
_sig("ntt_rns_fwd_batch", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_uint64, VOIDP)
_sig("ntt_rns_inv_batch", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_uint64, VOIDP)
_sig("ntt_rns_negacyclic_mul_batch", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, VOIDP, C.c_uint64, VOIDP)
_sig("ntt_inv_product_batch", C.c_int, VOIDP, VOIDP, VOIDP, VOIDP, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_inv_dot_batch", C.c_int, VOIDP, VOIDP, C.c_int, C.POINTER(VOIDP), C.POINTER(VOIDP), C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_mul_transformed_batch", C.c_int, VOIDP, VOIDP, VOIDP, VOIDP, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_inv_dot_batch", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_int, C.POINTER(VOIDP), C.POINTER(VOIDP), C.c_uint64,
     C.c_uint, VOIDP)
_sig("ntt_rns_mul_transformed_batch", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, VOIDP, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_fwd_mul_batch", C.c_int, VOIDP, VOIDP, VOIDP, VOIDP, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_fwd_mul_batch", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, VOIDP, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_fwd_batch_strided", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_uint64, C.c_uint64, C.c_uint64, VOIDP)
_sig("ntt_rns_inv_batch_strided", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_uint64, C.c_uint64, C.c_uint64, VOIDP)
_sig("ntt_rns_negacyclic_mul_batch_strided", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, VOIDP, C.c_uint64, C.c_uint64, C.c_uint64, VOIDP)
_sig("ntt_rns_inv_dot_batch_strided", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_int, C.POINTER(VOIDP), C.POINTER(VOIDP), C.c_uint64,
     C.c_uint64, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_mul_transformed_batch_strided", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, VOIDP, C.c_uint64, C.c_uint64, C.c_uint64,
     C.c_uint, VOIDP)
_sig("ntt_rns_fwd_mul_batch_strided", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, VOIDP, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_rescale_batch", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_rescale_batch_strided", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_mod_up_batch", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_int, C.c_int, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_mod_up_batch_strided", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64,
     C.c_uint, VOIDP)
_sig("ntt_rns_mod_down_batch", C.c_int, C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_mod_down_batch_strided", C.c_int, C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint,
     VOIDP)
_sig("ntt_rns_mod_up_mul_batch", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, C.c_int, C.c_int, VOIDP, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_mod_up_mul_batch_strided", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, C.c_int, C.c_int, VOIDP, C.c_uint64, C.c_uint64,
     C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_fwd_mul_pair_batch", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, VOIDP, VOIDP, VOIDP, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_fwd_mul_pair_batch_strided", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, VOIDP, VOIDP, VOIDP, C.c_uint64, C.c_uint64,
     C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_mod_up_mul_pair_batch", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, VOIDP, C.c_int, C.c_int, VOIDP, VOIDP, C.c_uint64,
     C.c_uint, VOIDP)
_sig("ntt_rns_mod_up_mul_pair_batch_strided", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, VOIDP, C.c_int, C.c_int, VOIDP, VOIDP,
     C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_galois_dot_pair_batch", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, C.c_int, C.POINTER(VOIDP), C.POINTER(VOIDP),
     C.POINTER(VOIDP), C.c_uint64, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_galois_dot_pair_batch_strided", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, C.c_int, C.POINTER(VOIDP), C.POINTER(VOIDP),
     C.POINTER(VOIDP), C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_tensor_batch", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, VOIDP, VOIDP, VOIDP, VOIDP, VOIDP, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_tensor_batch_strided", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, VOIDP, VOIDP, VOIDP, VOIDP, VOIDP, C.c_uint64, C.c_uint64,
     C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_mod_down_add_batch", C.c_int, C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_mod_down_add_batch_strided", C.c_int, C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, C.c_uint64, C.c_uint64, C.c_uint64,
     C.c_uint64, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_mod_up_exact_batch", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_int, C.c_int, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_mod_up_exact_batch_strided", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64,
     C.c_uint, VOIDP)
_sig("ntt_rns_mod_down_exact_batch", C.c_int, C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_uint64, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_mod_down_exact_batch_strided", C.c_int, C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
     C.c_uint, VOIDP)
_sig("ntt_rns_mod_down_bgv_batch", C.c_int, C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_uint64, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_mod_down_bgv_batch_strided", C.c_int, C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
     C.c_uint, VOIDP)
_sig("ntt_rns_mod_down_bgv_add_batch", C.c_int, C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, C.c_uint64, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_mod_down_bgv_add_batch_strided", C.c_int, C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, C.c_uint64, C.c_uint64, C.c_uint64,
     C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_galois_rotation", C.c_uint64, C.c_uint64, C.c_int64)
_sig("ntt_galois_batch", C.c_int, VOIDP, VOIDP, VOIDP, C.c_uint64, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_galois_batch", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, C.c_uint64, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_galois_batch_strided", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
     C.c_uint, VOIDP)
_sig("ntt_rns_galois_dot_batch", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_int, C.POINTER(VOIDP), C.POINTER(VOIDP), C.c_uint64,
     C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_galois_dot_batch_strided", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_int, C.POINTER(VOIDP), C.POINTER(VOIDP), C.c_uint64,
     C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_lincomb_batch", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_int, C.POINTER(VOIDP), C.POINTER(VOIDP), U64P, U64P, U64P,
     C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_lincomb_batch_strided", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_int, C.POINTER(VOIDP), C.POINTER(VOIDP), U64P, U64P, U64P,
     C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_to_plain_batch", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, C.c_uint64, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_to_plain_batch_strided", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
     C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_to_double_batch", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, C.c_double, C.c_uint64, VOIDP)
_sig("ntt_rns_to_double_batch_strided", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, C.c_double, C.c_uint64, C.c_uint64, C.c_uint64,
     C.c_uint64, VOIDP)
_sig("ntt_rns_from_plain_batch", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, C.c_uint64, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_from_plain_batch_strided", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
     C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_from_double_batch", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, C.c_double, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_from_double_batch_strided", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, C.c_double, C.c_uint64, C.c_uint64, C.c_uint64,
     C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_sample_batch", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_sample_batch_strided", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
     C.c_uint64, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_transform_batch_strided", C.c_int, VOIDP, VOIDP, C.c_uint64, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_transform_ptrs", C.c_int, VOIDP, C.POINTER(VOIDP), C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_transform_ptrs", C.c_int, C.c_int, C.POINTER(VOIDP), C.POINTER(VOIDP), C.c_uint64, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_transform_dev_ptrs", C.c_int, VOIDP, VOIDP, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_transform_dev_ptrs", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_uint64, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_inv_dot_dev_ptrs", C.c_int, VOIDP, VOIDP, C.c_int, C.POINTER(VOIDP), C.POINTER(VOIDP), C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_fwd_mul_dev_ptrs", C.c_int, VOIDP, VOIDP, VOIDP, VOIDP, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_negacyclic_mul_dev_ptrs", C.c_int, VOIDP, VOIDP, VOIDP, VOIDP, C.c_uint64, VOIDP)
_sig("ntt_rns_inv_dot_dev_ptrs", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, C.c_int, C.POINTER(VOIDP), C.POINTER(VOIDP), C.c_uint64, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_fwd_mul_dev_ptrs", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, VOIDP, C.c_uint64, C.c_uint64, C.c_uint, VOIDP)
_sig("ntt_rns_negacyclic_mul_dev_ptrs", C.c_int, C.c_int, C.POINTER(VOIDP), VOIDP, VOIDP, VOIDP, C.c_uint64, C.c_uint64, VOIDP)
_sig("ntt_dev_malloc", C.c_int, C.c_int, C.POINTER(VOIDP), C.c_size_t)
_sig("ntt_dev_mem_info", C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t))
_sig("ntt_dev_free", C.c_int, C.c_int, VOIDP)
_sig("ntt_h2d", C.c_int, C.c_int, VOIDP, VOIDP, C.c_size_t)
_sig("ntt_d2h", C.c_int, C.c_int, VOIDP, VOIDP, C.c_size_t)
_sig("ntt_stream_create", C.c_int, C.c_int, C.POINTER(VOIDP))
_sig("ntt_stream_destroy", C.c_int, C.c_int, VOIDP)
_sig("ntt_stream_sync", C.c_int, C.c_int, VOIDP)
_sig("ntt_event_create", C.c_int, C.c_int, C.POINTER(VOIDP))
_sig("ntt_event_destroy", C.c_int, C.c_int, VOIDP)
_sig("ntt_event_record", C.c_int, C.c_int, VOIDP, VOIDP)
_sig("ntt_event_elapsed_ms", C.c_int, C.c_int, VOIDP, VOIDP, C.POINTER(C.c_float))
_sig("ntt_fill_uniform", C.c_int, C.c_int, VOIDP, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, VOIDP)
_sig("ntt_poly_checksum", C.c_int, C.c_int, VOIDP, VOIDP, C.c_uint64, C.c_uint64, VOIDP)
_sig("ntt_rmw_probe", C.c_int, C.c_int, VOIDP, C.c_uint64, C.c_uint64, VOIDP)
_sig("ntt_shape_probe", C.c_int, C.c_int, VOIDP, C.c_uint64, C.c_uint64, VOIDP)
_sig("ntt_copy_probe", C.c_int, C.c_int, VOIDP, VOIDP, C.c_uint64, VOIDP)
_sig("ntt_batch_multi", C.c_int, C.c_int, C.POINTER(VOIDP), C.POINTER(VOIDP), U64P, C.c_int)
_sig("ntt_rns_mul_multi", C.c_int, C.c_int, C.c_int, C.POINTER(VOIDP), C.POINTER(VOIDP), C.POINTER(VOIDP), C.POINTER(VOIDP), U64P)
_sig("ntt_compat_release", None)
_sig("ntt_compat_cached_plans", C.c_int)
_sig("ntt_min_root", C.c_uint64, C.c_uint64, C.c_uint64)
_sig("ntt_find_prime", C.c_uint64, C.c_uint, C.c_uint64, C.c_uint)
for _n in ("fwd_ntt_ref_harvey_lazy", "fwd_ntt_radix4_lazy", "fwd_ntt_radix4x4_lazy", "fwd_ntt_seal_lazy"):
    _sig(_n, None, U64P, C.c_uint64, C.c_uint64, U64P, U64P)
_sig("fwd_ntt_ref_harvey_lazy_dbl", None, U64P, U64P, C.c_uint64, C.c_uint64, U64P, U64P)
_sig("inv_ntt_ref_harvey", None, U64P, C.c_uint64, C.c_uint64, MulOp, C.c_uint64, U64P, U64P)
_sig("inv_ntt_radix4", None, U64P, C.c_uint64, C.c_uint64, MulOp, U64P, U64P)
_sig("inv_ntt_seal", None, U64P, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, U64P, U64P)


def last_error():
    return _lib.ntt_last_error().decode()


def _check(rc):
    # ntt_last_error is thread-local in the library and only read here, on the failing thread, immediately
    # after the failing call
    if rc != NTT_OK:
        raise NttError("ntt status %d: %s" % (rc, last_error()))


def version():
    return _lib.ntt_version().decode()


def device_count():
    n = _lib.ntt_device_count()
    if n < 0:
        raise NttError(last_error())
    return n


def compat_release():
    _lib.ntt_compat_release()


def compat_cached_plans():
    return int(_lib.ntt_compat_cached_plans())


def min_root(q, n):
    return int(_lib.ntt_min_root(q, n))


def find_prime(bits, n, skip=0):
    return int(_lib.ntt_find_prime(bits, n, skip))


def _ptr(a):
    assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(U64P)


# --------------------------------------------------------------------------
# device memory (library-owned HIP allocations; torch tensors work as well:
# pass tensor.data_ptr() wherever a device pointer is expected)
# --------------------------------------------------------------------------
class DeviceBuffer:
    def __init__(self, n_u64, device=0):
        self.device, self.n = device, int(n_u64)
        p = VOIDP()
        _check(_lib.ntt_dev_malloc(device, C.byref(p), self.n * 8))
        self.ptr = p.value

    def upload(self, host):
        host = np.ascontiguousarray(host, dtype=np.uint64)
        assert host.size <= self.n
        _check(_lib.ntt_h2d(self.device, self.ptr, host.ctypes.data, host.size * 8))
        return self

    def download(self, n=None, offset=0):
        n = self.n - offset if n is None else int(n)
        out = np.empty(n, dtype=np.uint64)
        _check(_lib.ntt_d2h(self.device, out.ctypes.data, self.ptr + 8 * offset, n * 8))
        return out

    def free(self):
        if self.ptr:
            _lib.ntt_dev_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def mem_info(device=0):
    """(free, total) bytes of device memory: hipMemGetInfo"""
    f, t = C.c_size_t(), C.c_size_t()
    _check(_lib.ntt_dev_mem_info(device, C.byref(f), C.byref(t)))
    return f.value, t.value


def fill_uniform(dptr, n, q, seed, offset=0, device=0, stream=None):
    _check(_lib.ntt_fill_uniform(device, dptr, n, q, seed, offset, stream))


def poly_checksum(dout, dptr, N, batch, device=0, stream=None):
    _check(_lib.ntt_poly_checksum(device, dout, dptr, N, batch, stream))


def rmw_probe(dptr, n, mask=0, device=0, stream=None):
    """in-place read-XOR-write of n words: the measured ceiling of the transform's memory shape"""
    _check(_lib.ntt_rmw_probe(device, dptr, n, mask, stream))


def shape_probe(dptr, n, mask=0, device=0, stream=None):
    """the same in the memory shape of the 2^14 block kernels (persistent workgroups, register prefetch, 16-byte accesses)"""
    _check(_lib.ntt_shape_probe(device, dptr, n, mask, stream))


def copy_probe(ddst, dsrc, n, device=0, stream=None):
    """out-of-place 16-byte-per-lane copy of n words (the guide's copy shape: 16 n bytes move)"""
    _check(_lib.ntt_copy_probe(device, ddst, dsrc, n, stream))


def stream_sync(device=0, stream=None):
    _check(_lib.ntt_stream_sync(device, stream))


class Event:
    def __init__(self, device=0):
        self.device = device
        e = VOIDP()
        _check(_lib.ntt_event_create(device, C.byref(e)))
        self.h = e.value

    def record(self, stream=None):
        _check(_lib.ntt_event_record(self.device, self.h, stream))

    def elapsed_ms_since(self, start):
        ms = C.c_float()
        _check(_lib.ntt_event_elapsed_ms(self.device, start.h, self.h, C.byref(ms)))
        return ms.value


# --------------------------------------------------------------------------
# plans
# --------------------------------------------------------------------------
class Plan:
    """Tables for one (device, N, q, root); see include/ntt_mi355x.h."""

    def __init__(self, N, q, root, device=0, arith=ARITH_AUTO):
        h = VOIDP()
        _check(_lib.ntt_plan_create(C.byref(h), device, N, q, root, arith))
        self.h, self.N, self.q, self.root, self.device = h.value, N, q, root, device

    def info(self):
        v = (C.c_uint64 * 8)()
        _check(_lib.ntt_plan_info(self.h, v))
        keys = ("N", "q", "log2N", "arith", "f64_class", "hbm_passes", "device", "root")
        return dict(zip(keys, [int(x) for x in v]))

    def set_generic(self, on):
        _check(_lib.ntt_plan_set_generic(self.h, int(on)))

    def export_table(self, which, n_records, dtype=np.uint64):
        """device table `which` (0 fwd, 1 inv, 2/3 compact fwd/inv) as an array of shape (n_records, 2) -- or
        (n_records,) for the compact tables -- of `dtype` (uint64 for the integer policies, float64 for FP64)"""
        width = 1 if which >= 2 else 2
        out = np.zeros(n_records * width, dtype=dtype)
        _check(_lib.ntt_plan_export_table(self.h, which, out.ctypes.data, out.nbytes))
        return out.reshape(n_records, width) if width == 2 else out

    def enable_slots(self):
        """ntt_plan_enable_slots: builds the slot tables pos / ipos on the device (idempotent; outside stream capture)"""
        _check(_lib.ntt_plan_enable_slots(self.h))
        return self

    def slot_table(self, inverse=False):
        """the device table pos (inverse: ipos) as N uint32"""
        out = np.zeros(self.N, dtype=np.uint32)
        _check(_lib.ntt_plan_export_table(self.h, 5 if inverse else 4, out.ctypes.data, out.nbytes))
        return out

    def set_option(self, option, value):
        _check(_lib.ntt_plan_set_option(self.h, option, value))

    def get_option(self, option):
        v = C.c_int64()
        _check(_lib.ntt_plan_get_option(self.h, option, C.byref(v)))
        return v.value

    def reserve(self, polys, stream=None):
        """ntt_plan_reserve: the control blocks of the XCD-local launches on `stream`, sized for `polys` polynomials x limbs"""
        _check(_lib.ntt_plan_reserve(self.h, stream, polys))

    def fwd(self, dptr, batch, stream=None, wide=False, lazy=False):
        if wide and lazy:
            _check(_lib.ntt_transform_batch(self.h, dptr, batch, FLAG_WIDE_IN | FLAG_LAZY_OUT, stream))
            return
        f = _lib.ntt_fwd_batch_lazy if lazy else (_lib.ntt_fwd_batch_wide if wide else _lib.ntt_fwd_batch)
        _check(f(self.h, dptr, batch, stream))

    def inv(self, dptr, batch, stream=None, wide=False, lazy=False):
        if wide and lazy:
            _check(_lib.ntt_transform_batch(self.h, dptr, batch, FLAG_INVERSE | FLAG_WIDE_IN | FLAG_LAZY_OUT, stream))
            return
        f = _lib.ntt_inv_batch_lazy if lazy else (_lib.ntt_inv_batch_wide if wide else _lib.ntt_inv_batch)
        _check(f(self.h, dptr, batch, stream))

    def transform_strided(self, dptr, poly_stride, batch, flags=0, stream=None):
        """`batch` polynomials poly_stride words apart (ntt_transform_batch_strided); flags = FLAG_*"""
        _check(_lib.ntt_transform_batch_strided(self.h, dptr, poly_stride, batch, flags, stream))

    def transform_ptrs(self, ptrs, flags=0, stream=None):
        """one device pointer per polynomial (ntt_transform_ptrs)"""
        k = len(ptrs)
        _check(_lib.ntt_transform_ptrs(self.h, (VOIDP * k)(*ptrs), k, flags, stream))

    def transform_dev_ptrs(self, d_table, count, flags=0, stream=None):
        """the same with the pointers already in DEVICE memory (ntt_transform_dev_ptrs): d_table = device address of `count` pointers"""
        _check(_lib.ntt_transform_dev_ptrs(self.h, d_table, count, flags, stream))

    def inv_dot_dev_ptrs(self, c_tab, a_tabs, b_tabs, count, flags=0, stream=None):
        """ntt_inv_dot_dev_ptrs: c_tab = device table of `count` pointers; a_tabs / b_tabs = lists of k device tables (a broadcast b: device pointers to ONE polynomial each)"""
        k = len(a_tabs)
        _check(_lib.ntt_inv_dot_dev_ptrs(self.h, c_tab, k, (VOIDP * k)(*a_tabs), (VOIDP * k)(*b_tabs), count, flags, stream))

    def fwd_mul_dev_ptrs(self, c_tab, a_tab, b_tab, count, flags=0, stream=None):
        _check(_lib.ntt_fwd_mul_dev_ptrs(self.h, c_tab, a_tab, b_tab, count, flags, stream))

    def negacyclic_mul_dev_ptrs(self, c_tab, a_tab, b_tab, count, stream=None):
        _check(_lib.ntt_negacyclic_mul_dev_ptrs(self.h, c_tab, a_tab, b_tab, count, stream))

    def pointwise_mul(self, dc, da, db, batch, stream=None, lazy_in=False):
        f = _lib.ntt_pointwise_mul_batch_lazy if lazy_in else _lib.ntt_pointwise_mul_batch
        _check(f(self.h, dc, da, db, batch, stream))

    def negacyclic_mul(self, dc, da, db, batch, stream=None):
        _check(_lib.ntt_negacyclic_mul_batch(self.h, dc, da, db, batch, stream))

    # operands in the NTT domain (include/ntt_mi355x.h): flags = MUL_LAZY_IN | MUL_B_BROADCAST
    def inv_product(self, dc, dahat, dbhat, batch, flags=0, stream=None):
        _check(_lib.ntt_inv_product_batch(self.h, dc, dahat, dbhat, batch, flags, stream))

    def inv_dot(self, dc, dahats, dbhats, batch, flags=0, stream=None):
        k = len(dahats)
        assert k == len(dbhats)
        _check(_lib.ntt_inv_dot_batch(self.h, dc, k, (VOIDP * k)(*dahats), (VOIDP * k)(*dbhats), batch, flags, stream))

    def mul_transformed(self, dc, da, dbhat, batch, flags=0, stream=None):
        _check(_lib.ntt_mul_transformed_batch(self.h, dc, da, dbhat, batch, flags, stream))

    def fwd_mul(self, dc, da, dbhat, batch, flags=0, stream=None):
        """c^ = fwd(a) (.) b^ (MUL_ACCUMULATE: c^ += ...): the result stays in the NTT domain"""
        _check(_lib.ntt_fwd_mul_batch(self.h, dc, da, dbhat, batch, flags, stream))

    def galois(self, dout, din, g, batch, flags=0, stream=None):
        """out = sigma_g(in): a(X) -> a(X^g), out of place (GALOIS_TRANSFORMED: both in the NTT domain, a permutation of words)"""
        _check(_lib.ntt_galois_batch(self.h, dout, din, g, batch, flags, stream))

    # host-array conveniences used by the parity tests
    def fwd_host(self, a, wide=False, lazy=False):
        a = np.ascontiguousarray(a, dtype=np.uint64)
        batch = a.size // self.N
        buf = DeviceBuffer(a.size, self.device).upload(a)
        self.fwd(buf.ptr, batch, wide=wide, lazy=lazy)
        out = buf.download()
        buf.free()
        return out

    def inv_host(self, a, wide=False, lazy=False):
        a = np.ascontiguousarray(a, dtype=np.uint64)
        batch = a.size // self.N
        buf = DeviceBuffer(a.size, self.device).upload(a)
        self.inv(buf.ptr, batch, wide=wide, lazy=lazy)
        out = buf.download()
        buf.free()
        return out

    def destroy(self):
        if self.h:
            _lib.ntt_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def _plan_array(plans):
    return (VOIDP * len(plans))(*[p.h for p in plans])


def set_rns_launch(plans, mode):
    """how ntt_rns_* launch a run of compatible limbs (NTT_OPT_RNS_LAUNCH on every plan): 0 / "0" = one launch over the run
    wherever built, 1 / "1" = one launch chain per limb, None = the library's choice"""
    v = -1 if mode is None else int(mode)
    for p in plans:
        p.set_option(OPT_RNS_LAUNCH, v)


def rns_transform_ptrs(plans, ptrs, limb_stride, flags=0, stream=None):
    """one device pointer per RNS polynomial (its limbs limb_stride words apart): ntt_rns_transform_ptrs"""
    k = len(ptrs)
    _check(_lib.ntt_rns_transform_ptrs(len(plans), _plan_array(plans), (VOIDP * k)(*ptrs), k, limb_stride, flags, stream))


def rns_transform_dev_ptrs(plans, d_table, count, limb_stride, flags=0, stream=None):
    """ntt_rns_transform_dev_ptrs: the pointers (limb 0 of every RNS polynomial) in a DEVICE array"""
    _check(_lib.ntt_rns_transform_dev_ptrs(len(plans), _plan_array(plans), d_table, count, limb_stride, flags, stream))


def rns_inv_dot_dev_ptrs(plans, c_tab, a_tabs, b_tabs, count, limb_stride, flags=0, stream=None):
    k = len(a_tabs)
    _check(_lib.ntt_rns_inv_dot_dev_ptrs(len(plans), _plan_array(plans), c_tab, k, (VOIDP * k)(*a_tabs), (VOIDP * k)(*b_tabs), count, limb_stride, flags, stream))


def rns_fwd_mul_dev_ptrs(plans, c_tab, a_tab, b_tab, count, limb_stride, flags=0, stream=None):
    _check(_lib.ntt_rns_fwd_mul_dev_ptrs(len(plans), _plan_array(plans), c_tab, a_tab, b_tab, count, limb_stride, flags, stream))


def rns_negacyclic_mul_dev_ptrs(plans, c_tab, a_tab, b_tab, count, limb_stride, stream=None):
    _check(_lib.ntt_rns_negacyclic_mul_dev_ptrs(len(plans), _plan_array(plans), c_tab, a_tab, b_tab, count, limb_stride, stream))


def batch_major(plans):
    """(limb_stride, poly_stride) of SURVEY 8(d)'s [batch][prime][N] layout for this limb list"""
    return (plans[0].N, len(plans) * plans[0].N)


def rns_fwd(plans, dptr, batch, stream=None, layout=None):
    """limbs laid out [limb][batch][N]; layout = (limb_stride, poly_stride) in words for any other placement"""
    if layout: _check(_lib.ntt_rns_fwd_batch_strided(len(plans), _plan_array(plans), dptr, layout[0], layout[1], batch, stream))
    else: _check(_lib.ntt_rns_fwd_batch(len(plans), _plan_array(plans), dptr, batch, stream))


def rns_inv(plans, dptr, batch, stream=None, layout=None):
    if layout: _check(_lib.ntt_rns_inv_batch_strided(len(plans), _plan_array(plans), dptr, layout[0], layout[1], batch, stream))
    else: _check(_lib.ntt_rns_inv_batch(len(plans), _plan_array(plans), dptr, batch, stream))


def rns_negacyclic_mul(plans, dc, da, db, batch, stream=None, layout=None):
    if layout: _check(_lib.ntt_rns_negacyclic_mul_batch_strided(len(plans), _plan_array(plans), dc, da, db, layout[0], layout[1], batch, stream))
    else: _check(_lib.ntt_rns_negacyclic_mul_batch(len(plans), _plan_array(plans), dc, da, db, batch, stream))


def rns_inv_dot(plans, dc, dahats, dbhats, batch, flags=0, stream=None, layout=None):
    """operands laid out [limb][batch][N] (a broadcast b^: [limb][N])"""
    k = len(dahats)
    if layout:
        _check(_lib.ntt_rns_inv_dot_batch_strided(len(plans), _plan_array(plans), dc, k, (VOIDP * k)(*dahats), (VOIDP * k)(*dbhats), layout[0],
                                                  layout[1], batch, flags, stream))
    else:
        _check(_lib.ntt_rns_inv_dot_batch(len(plans), _plan_array(plans), dc, k, (VOIDP * k)(*dahats), (VOIDP * k)(*dbhats), batch,
                                          flags, stream))


def rns_fwd_mul(plans, dc, da, dbhat, batch, flags=0, stream=None, layout=None):
    if layout: _check(_lib.ntt_rns_fwd_mul_batch_strided(len(plans), _plan_array(plans), dc, da, dbhat, layout[0], layout[1], batch, flags, stream))
    else: _check(_lib.ntt_rns_fwd_mul_batch(len(plans), _plan_array(plans), dc, da, dbhat, batch, flags, stream))


def rns_mul_transformed(plans, dc, da, dbhat, batch, flags=0, stream=None, layout=None):
    if layout:
        _check(_lib.ntt_rns_mul_transformed_batch_strided(len(plans), _plan_array(plans), dc, da, dbhat, layout[0], layout[1], batch, flags, stream))
    else:
        _check(_lib.ntt_rns_mul_transformed_batch(len(plans), _plan_array(plans), dc, da, dbhat, batch, flags, stream))


def rns_rescale(plans, dptr, batch, flags=0, stream=None, layout=None):
    """drop the last prime of plans (in place): limbs 0 .. L-1 become round(x / q_L) (RESCALE_FLOOR: floor), in the NTT domain with
    RESCALE_TRANSFORMED; limbs laid out [limb][batch][N], layout = (limb_stride, poly_stride) in words for any other placement"""
    if layout: _check(_lib.ntt_rns_rescale_batch_strided(len(plans), _plan_array(plans), dptr, layout[0], layout[1], batch, flags, stream))
    else: _check(_lib.ntt_rns_rescale_batch(len(plans), _plan_array(plans), dptr, batch, flags, stream))


def rns_mod_up(plans, dptr, first, count, batch, flags=0, stream=None, layout=None):
    """ModUp in place: every limb outside the digit [first, first + count) of plans gets FastBConv of the digit (MODUP_TRANSFORMED:
    the operand in the NTT domain); limbs laid out [limb][batch][N], layout = (limb_stride, poly_stride) in words otherwise"""
    if layout:
        _check(_lib.ntt_rns_mod_up_batch_strided(len(plans), _plan_array(plans), dptr, first, count, layout[0], layout[1], batch, flags,
                                                 stream))
    else: _check(_lib.ntt_rns_mod_up_batch(len(plans), _plan_array(plans), dptr, first, count, batch, flags, stream))


def rns_mod_up_mul(plans, dc, dext, first, count, dkeyhat, batch, flags=0, stream=None, layout=None):
    """c^ (+)= fwd(ModUp(digit)) (.) key^ on every limb: one digit's term of the key-switching inner product.  dext holds the digit's
    coefficients in limbs [first, first + count), its other slots are scratch (untouched where the fused kernel serves every run:
    OPT_MODUP_FUSED on plans[0]); flags: MUL_B_BROADCAST (the key is [limb][N]), MUL_ACCUMULATE, MUL_LAZY_IN (key words); limbs laid
    out [limb][batch][N], layout = (limb_stride, poly_stride) in words otherwise"""
    if layout:
        _check(_lib.ntt_rns_mod_up_mul_batch_strided(len(plans), _plan_array(plans), dc, dext, first, count, dkeyhat, layout[0], layout[1],
                                                     batch, flags, stream))
    else: _check(_lib.ntt_rns_mod_up_mul_batch(len(plans), _plan_array(plans), dc, dext, first, count, dkeyhat, batch, flags, stream))


def rns_fwd_mul_pair(plans, dc0, dc1, da, db0hat, db1hat, batch, flags=0, stream=None, layout=None):
    """c0^ (+)= fwd(a) (.) b0^ and c1^ (+)= fwd(a) (.) b1^ on every limb from ONE forward transform of a (a is scratch; untouched where
    the fused pair kernel serves every run: OPT_PAIR_FUSED on plans[0]); flags as rns_fwd_mul, one word for both components; limbs laid
    out [limb][batch][N], layout = (limb_stride, poly_stride) in words otherwise"""
    if layout:
        _check(_lib.ntt_rns_fwd_mul_pair_batch_strided(len(plans), _plan_array(plans), dc0, dc1, da, db0hat, db1hat, layout[0], layout[1],
                                                       batch, flags, stream))
    else: _check(_lib.ntt_rns_fwd_mul_pair_batch(len(plans), _plan_array(plans), dc0, dc1, da, db0hat, db1hat, batch, flags, stream))


def rns_mod_up_mul_pair(plans, dc0, dc1, dext, first, count, dkey0hat, dkey1hat, batch, flags=0, stream=None, layout=None):
    """c0^ (+)= fwd(ModUp(digit)) (.) key0^ and c1^ (+)= fwd(ModUp(digit)) (.) key1^ on every limb: one digit's term of both components
    of a key switch, the digit converted and transformed once.  dext as for rns_mod_up_mul (its other slots are scratch; untouched
    where the fused pair kernel serves every run: OPT_PAIR_FUSED on plans[0]); flags: MUL_B_BROADCAST, MUL_ACCUMULATE, MUL_LAZY_IN,
    one word for both components; limbs laid out [limb][batch][N], layout = (limb_stride, poly_stride) in words otherwise"""
    if layout:
        _check(_lib.ntt_rns_mod_up_mul_pair_batch_strided(len(plans), _plan_array(plans), dc0, dc1, dext, first, count, dkey0hat, dkey1hat,
                                                          layout[0], layout[1], batch, flags, stream))
    else:
        _check(_lib.ntt_rns_mod_up_mul_pair_batch(len(plans), _plan_array(plans), dc0, dc1, dext, first, count, dkey0hat, dkey1hat, batch,
                                                  flags, stream))


def rns_mod_down(plans, np_, dptr, batch, flags=0, stream=None, layout=None):
    """ModDown in place: the last np_ plans are P; the Q limbs become round(x / P) - v (MODDOWN_FLOOR: floor), in the NTT domain with
    MODDOWN_TRANSFORMED; limbs laid out [limb][batch][N], layout = (limb_stride, poly_stride) in words otherwise"""
    nq = len(plans) - np_
    if layout:
        _check(_lib.ntt_rns_mod_down_batch_strided(nq, np_, _plan_array(plans), dptr, layout[0], layout[1], batch, flags, stream))
    else: _check(_lib.ntt_rns_mod_down_batch(nq, np_, _plan_array(plans), dptr, batch, flags, stream))


def rns_tensor(plans, dc0, dc1, dc2, da0, da1, db0, db1, batch, flags=0, stream=None, layout=None):
    """the ciphertext tensor product per limb and word: c0 = a0 b0, c1 = a0 b1 + a1 b0, c2 = a1 b1, canonical (MUL_LAZY_IN: input words
    in [0, 4q)); db0 == da0 and db1 == da1 is a squaring (every input word loaded once); an output may be an input; all operands laid
    out [limb][batch][N], layout = (limb_stride, poly_stride) in words otherwise"""
    if layout:
        _check(_lib.ntt_rns_tensor_batch_strided(len(plans), _plan_array(plans), dc0, dc1, dc2, da0, da1, db0, db1, layout[0], layout[1],
                                                 batch, flags, stream))
    else: _check(_lib.ntt_rns_tensor_batch(len(plans), _plan_array(plans), dc0, dc1, dc2, da0, da1, db0, db1, batch, flags, stream))


def rns_mod_down_add(plans, np_, dc, da, batch, flags=0, stream=None, layout=None):
    """ModDown of the accumulator da (over Q u P, the last np_ plans are P) into the ciphertext dc (over Q): c = ModDown(a), or
    c += ModDown(a) with MODDOWN_ACCUMULATE; MODDOWN_TRANSFORMED / MODDOWN_FLOOR as rns_mod_down.  da's Q limbs are scratch afterwards
    (untouched where the fused kernel serves every run: OPT_MODDOWN_ADD_FUSED on plans[0]).  dc is [nq][batch][N] and da
    [nq + np_][batch][N]; layout = (c_limb_stride, c_poly_stride, a_limb_stride, a_poly_stride) in words otherwise"""
    nq = len(plans) - np_
    if layout:
        _check(_lib.ntt_rns_mod_down_add_batch_strided(nq, np_, _plan_array(plans), dc, da, layout[0], layout[1], layout[2], layout[3],
                                                       batch, flags, stream))
    else: _check(_lib.ntt_rns_mod_down_add_batch(nq, np_, _plan_array(plans), dc, da, batch, flags, stream))


def rns_mod_up_exact(plans, dptr, first, count, batch, flags=0, stream=None, layout=None):
    """exact ModUp in place: every limb outside the digit [first, first + count) of plans gets the CENTRED value of the digit (x, or
    x - B from B / 2 on: the HPS floating-point correction of FastBConv); flags and layout as rns_mod_up"""
    if layout:
        _check(_lib.ntt_rns_mod_up_exact_batch_strided(len(plans), _plan_array(plans), dptr, first, count, layout[0], layout[1], batch,
                                                       flags, stream))
    else: _check(_lib.ntt_rns_mod_up_exact_batch(len(plans), _plan_array(plans), dptr, first, count, batch, flags, stream))


def rns_mod_down_exact(plans, np_, dptr, mult, batch, flags=0, stream=None, layout=None):
    """exact scaled ModDown in place: the last np_ plans are P; the Q limbs become round(mult * x / P) exactly (1 <= mult < 2^61; BFV's
    round(t x / Q) with mult = t), in the NTT domain with MODDOWN_TRANSFORMED (the only flag); layout as rns_mod_down"""
    nq = len(plans) - np_
    if layout:
        _check(_lib.ntt_rns_mod_down_exact_batch_strided(nq, np_, _plan_array(plans), dptr, mult, layout[0], layout[1], batch, flags, stream))
    else: _check(_lib.ntt_rns_mod_down_exact_batch(nq, np_, _plan_array(plans), dptr, mult, batch, flags, stream))


def rns_mod_down_bgv(plans, np_, dptr, t, batch, flags=0, stream=None, layout=None):
    """BGV ModDown in place: the last np_ plans are P; the Q limbs become (x - t w) / P - v t, w the centred residue of x t^-1 mod P,
    0 <= v < np_: the plaintext mod t is multiplied by P^-1 mod t and nothing else (1 <= t < 2^61, no P prime divides t).  np_ = 1 is
    BGV's modulus switch.  MODDOWN_TRANSFORMED is the only flag; layout as rns_mod_down; OPT_BGV_FUSED on plans[0] selects the route"""
    nq = len(plans) - np_
    if layout:
        _check(_lib.ntt_rns_mod_down_bgv_batch_strided(nq, np_, _plan_array(plans), dptr, t, layout[0], layout[1], batch, flags, stream))
    else: _check(_lib.ntt_rns_mod_down_bgv_batch(nq, np_, _plan_array(plans), dptr, t, batch, flags, stream))


def rns_mod_down_bgv_add(plans, np_, dc, da, t, batch, flags=0, stream=None, layout=None):
    """BGV ModDown of the accumulator da (over Q u P) into the ciphertext dc (over Q): c = ModDown_t(a), or c += ModDown_t(a) with
    MODDOWN_ACCUMULATE (the last step of a BGV relinearisation or rotation); operands and layout as rns_mod_down_add, t as
    rns_mod_down_bgv.  da's Q limbs are scratch afterwards (untouched where the fused kernel serves every run)"""
    nq = len(plans) - np_
    if layout:
        _check(_lib.ntt_rns_mod_down_bgv_add_batch_strided(nq, np_, _plan_array(plans), dc, da, t, layout[0], layout[1], layout[2], layout[3],
                                                           batch, flags, stream))
    else: _check(_lib.ntt_rns_mod_down_bgv_add_batch(nq, np_, _plan_array(plans), dc, da, t, batch, flags, stream))


def galois_rotation(n, steps):
    """the Galois element 5^steps mod 2n of a rotation by `steps` slots (negative steps: the inverse power); 0 on a bad n"""
    return int(_lib.ntt_galois_rotation(n, steps))


def rns_galois(plans, dout, din, g, batch, flags=0, stream=None, layout=None):
    """out = sigma_g(in): a(X) -> a(X^g) on every limb, out of place (GALOIS_TRANSFORMED: both in the NTT domain); limbs laid out
    [limb][batch][N], layout = (limb_stride, poly_stride) in words otherwise"""
    if layout:
        _check(_lib.ntt_rns_galois_batch_strided(len(plans), _plan_array(plans), dout, din, g, layout[0], layout[1], batch, flags, stream))
    else: _check(_lib.ntt_rns_galois_batch(len(plans), _plan_array(plans), dout, din, g, batch, flags, stream))


def rns_galois_dot(plans, dc, dahats, dkeyhats, g, batch, flags=0, stream=None, layout=None):
    """c^ = sum_i sigma_g(a_i^) (.) key_i^ in the NTT domain (GALOIS_ACCUMULATE: c^ += ...; GALOIS_KEY_BROADCAST: every key is
    [limb][N], shared by the batch)"""
    k = len(dahats)
    assert k == len(dkeyhats)
    if layout:
        _check(_lib.ntt_rns_galois_dot_batch_strided(len(plans), _plan_array(plans), dc, k, (VOIDP * k)(*dahats), (VOIDP * k)(*dkeyhats), g,
                                                     layout[0], layout[1], batch, flags, stream))
    else:
        _check(_lib.ntt_rns_galois_dot_batch(len(plans), _plan_array(plans), dc, k, (VOIDP * k)(*dahats), (VOIDP * k)(*dkeyhats), g, batch,
                                             flags, stream))


def rns_galois_dot_pair(plans, dc0, dc1, dahats, dkey0hats, dkey1hats, g, batch, flags=0, stream=None, layout=None):
    """c_j^ = sum_i sigma_g(a_i^) (.) key_j,i^ for both components j of the rotation key in one launch per 16 limbs, every permuted
    digit read once (flags as rns_galois_dot, one word for both components)"""
    k = len(dahats)
    assert k == len(dkey0hats) == len(dkey1hats)
    arrs = ((VOIDP * k)(*dahats), (VOIDP * k)(*dkey0hats), (VOIDP * k)(*dkey1hats))
    if layout:
        _check(_lib.ntt_rns_galois_dot_pair_batch_strided(len(plans), _plan_array(plans), dc0, dc1, k, arrs[0], arrs[1], arrs[2], g,
                                                          layout[0], layout[1], batch, flags, stream))
    else:
        _check(_lib.ntt_rns_galois_dot_pair_batch(len(plans), _plan_array(plans), dc0, dc1, k, arrs[0], arrs[1], arrs[2], g, batch, flags,
                                                  stream))


def rns_lincomb(plans, dc, das, dms=None, scalars=None, gs=None, bias=None, batch=1, flags=0, stream=None, layout=None):
    """c (+)= bias + sum_i sigma_{g_i}(a_i) * mu_i per limb and word, mu_i the polynomial dms[i] or, where that is None, the per-limb
    scalars[i][l] (None: 1).  gs: one Galois element per term (None: 1), bias: one constant per limb (None: 0).  LINCOMB_ACCUMULATE:
    c += ...; LINCOMB_M_BROADCAST: every polynomial multiplier is [limb][N], shared by the batch; LINCOMB_LAZY_IN: a_i words in [0, 4q)"""
    k, nl = len(das), len(plans)
    a = (VOIDP * k)(*das)
    m = None
    if dms is not None:
        assert len(dms) == k
        m = (VOIDP * k)(*dms)
    s = None
    if scalars is not None:
        assert len(scalars) == k and all(len(row) == nl for row in scalars)
        s = (C.c_uint64 * (k * nl))(*[int(v) for row in scalars for v in row])
    g = None
    if gs is not None:
        assert len(gs) == k
        g = (C.c_uint64 * k)(*gs)
    b = None
    if bias is not None:
        assert len(bias) == nl
        b = (C.c_uint64 * nl)(*bias)
    if layout:
        _check(_lib.ntt_rns_lincomb_batch_strided(nl, _plan_array(plans), dc, k, a, m, s, g, b, layout[0], layout[1], batch, flags, stream))
    else: _check(_lib.ntt_rns_lincomb_batch(nl, _plan_array(plans), dc, k, a, m, s, g, b, batch, flags, stream))


def rns_add(plans, dc, da, db, batch, stream=None, layout=None):
    """c = a + b per limb and word (either domain); c may be a or b"""
    rns_lincomb(plans, dc, [da, db], batch=batch, stream=stream, layout=layout)


def rns_sub(plans, dc, da, db, batch, stream=None, layout=None):
    """c = a - b per limb and word (either domain); c may be a or b"""
    rns_lincomb(plans, dc, [da, db], scalars=[[1] * len(plans), [p.q - 1 for p in plans]], batch=batch, stream=stream, layout=layout)


def rns_neg(plans, dc, da, batch, stream=None, layout=None):
    """c = -a per limb and word (either domain); c may be a"""
    rns_lincomb(plans, dc, [da], scalars=[[p.q - 1 for p in plans]], batch=batch, stream=stream, layout=layout)


def rns_to_plain(plans, dm, da, t, batch, flags=0, stream=None, layout=None):
    """out of the RNS: dm ([batch][N]) = [x_c]_t of the coefficients da ([limb][batch][N], canonical), x_c the centred representative mod
    Q (BGV); PLAIN_SCALE: round(t x / Q) mod t (BFV; every prime coprime to t).  2 <= t < 2^61, up to 16 limbs.  layout =
    (a_limb_stride, a_poly_stride, m_poly_stride) in words for any other placement; dm may be da (limb 0's slots)"""
    if layout:
        _check(_lib.ntt_rns_to_plain_batch_strided(len(plans), _plan_array(plans), dm, da, t, layout[0], layout[1], layout[2], batch, flags,
                                                   stream))
    else: _check(_lib.ntt_rns_to_plain_batch(len(plans), _plan_array(plans), dm, da, t, batch, flags, stream))


def rns_to_double(plans, dy, da, scale, batch, stream=None, layout=None):
    """out of the RNS: dy ([batch][N] doubles) = fl(x_c) * scale for one or two limbs (CKKS, before the decoding FFT); layout =
    (a_limb_stride, a_poly_stride, y_poly_stride)"""
    if layout:
        _check(_lib.ntt_rns_to_double_batch_strided(len(plans), _plan_array(plans), dy, da, scale, layout[0], layout[1], layout[2], batch,
                                                    stream))
    else: _check(_lib.ntt_rns_to_double_batch(len(plans), _plan_array(plans), dy, da, scale, batch, stream))


def rns_from_plain(plans, dc, dm, t, batch, flags=0, stream=None, layout=None):
    """into the RNS: dc ([limb][batch][N], canonical) = the words dm ([batch][N], in [0, t)) lifted to every limb: [m_c]_q of the centred
    representative (BGV, plaintext operands); LIFT_SCALE: round(Q m / t) mod q (BFV; every prime coprime to t).  LIFT_TRANSFORMED: dc
    in the NTT domain; LIFT_ACCUMULATE: dc += the lift.  2 <= t < 2^61, any limb count.  layout = (c_limb_stride, c_poly_stride,
    m_poly_stride) in words for any other placement; OPT_LIFT_FUSED on plans[0] selects the NTT-domain route"""
    if layout:
        _check(_lib.ntt_rns_from_plain_batch_strided(len(plans), _plan_array(plans), dc, dm, t, layout[0], layout[1], layout[2], batch, flags,
                                                     stream))
    else: _check(_lib.ntt_rns_from_plain_batch(len(plans), _plan_array(plans), dc, dm, t, batch, flags, stream))


def rns_from_double(plans, dc, dy, scale, batch, flags=0, stream=None, layout=None):
    """into the RNS: dc = [rint(y * scale)]_q per limb for the doubles dy ([batch][N]) (CKKS, after the encoding FFT); 0 for NaN, inf and
    |y * scale| >= 2^127.  Flags and layout = (c_limb_stride, c_poly_stride, y_poly_stride) as rns_from_plain, without LIFT_SCALE"""
    if layout:
        _check(_lib.ntt_rns_from_double_batch_strided(len(plans), _plan_array(plans), dc, dy, scale, layout[0], layout[1], layout[2], batch,
                                                      flags, stream))
    else: _check(_lib.ntt_rns_from_double_batch(len(plans), _plan_array(plans), dc, dy, scale, batch, flags, stream))


def rns_sample(plans, dc, kind, seed, batch, first_poly=0, mult=1, flags=0, stream=None, layout=None):
    """random polynomials drawn on the device: dc ([limb][batch][N], canonical) = one word per limb and coefficient from the Philox4x32-10
    block of (seed, first_poly + polynomial, position) -- a statistical generator, not a cryptographic one.  SAMPLE_TERNARY / SAMPLE_CBD21:
    [mult v]_q of the same small v in every limb; SAMPLE_UNIFORM: the block mod q, independent per limb (mult = 1).  SAMPLE_TRANSFORMED:
    dc in the NTT domain; SAMPLE_ACCUMULATE: dc += the sample.  layout = (c_limb_stride, c_poly_stride) in words for any other
    placement; OPT_SAMPLE_FUSED on plans[0] selects the NTT-domain route"""
    a = (len(plans), _plan_array(plans), dc, kind, mult, seed & (2 ** 64 - 1), first_poly & (2 ** 64 - 1))
    if layout:
        _check(_lib.ntt_rns_sample_batch_strided(*a, layout[0], layout[1], batch, flags, stream))
    else: _check(_lib.ntt_rns_sample_batch(*a, batch, flags, stream))


def slot_position(n, i):
    """pos(i): the word of the forward transform that holds slot i = row * N/2 + column (None for a bad N or i)"""
    v = int(_lib.ntt_slot_position(n, i))
    return None if v == (1 << 64) - 1 else v


def slots_encode(plan, da, dv, batch, flags=0, stream=None, layout=None):
    """BFV / BGV: da ([batch][N] coefficients mod t) = the polynomial whose slots are dv ([batch][N], row-major 2 x N/2); dv is left
    untouched.  plan: a plan for (N, t, psi) with enable_slots().  layout = (v_poly_stride, a_poly_stride) in words for padded
    placements; OPT_SLOTS_FUSED on the plan selects the route"""
    if layout is not None: _check(_lib.ntt_slots_encode_batch_strided(plan.h, da, dv, layout[0], layout[1], batch, flags, stream))
    else: _check(_lib.ntt_slots_encode_batch(plan.h, da, dv, batch, flags, stream))


def slots_decode(plan, dv, da, batch, flags=0, stream=None, layout=None):
    """dv = the slots of the polynomials da; da is CONSUMED (its words are unspecified on return).  layout as slots_encode"""
    if layout is not None: _check(_lib.ntt_slots_decode_batch_strided(plan.h, dv, da, layout[0], layout[1], batch, flags, stream))
    else: _check(_lib.ntt_slots_decode_batch(plan.h, dv, da, batch, flags, stream))


def batch_multi(plans, dptrs, batches, inverse=False):
    n = len(plans)
    ph = (VOIDP * n)(*[p.h for p in plans])
    dp = (VOIDP * n)(*dptrs)
    bt = (C.c_uint64 * n)(*batches)
    _check(_lib.ntt_batch_multi(n, ph, dp, bt, int(inverse)))


def rns_mul_multi(plan_sets, dcs, das, dbs, batches):
    """RNS products across devices: plan_sets[g] = the limbs' plans on shard g's device"""
    ndev, nl = len(plan_sets), len(plan_sets[0])
    ph = (VOIDP * (ndev * nl))(*[p.h for ps in plan_sets for p in ps])
    _check(_lib.ntt_rns_mul_multi(ndev, nl, ph, (VOIDP * ndev)(*dcs), (VOIDP * ndev)(*das), (VOIDP * ndev)(*dbs),
                                  (C.c_uint64 * ndev)(*batches)))


# --------------------------------------------------------------------------
# reference-signature entry points on host numpy arrays (in place)
# --------------------------------------------------------------------------
def _mulop(op, con):
    m = MulOp()
    m.op_lo, m.op_hi, m.con_lo, m.con_hi = op & (2**64 - 1), op >> 64, con & (2**64 - 1), con >> 64
    return m


def _reduce(a, q, k):
    """the header-inline final reduction of the reference wrappers"""
    for m in ((4, 2, 1) if k == 8 else (2, 1)):
        np.subtract(a, np.uint64(m * q), out=a, where=a >= np.uint64(m * q))


def fwd_ntt_ref_harvey(a, N, q, w, w_con):
    _lib.fwd_ntt_ref_harvey_lazy(_ptr(a), N, q, _ptr(w), _ptr(w_con))
    _reduce(a, q, 4)


def fwd_ntt_ref_harvey_dbl(a1, a2, N, q, w, w_con):
    _lib.fwd_ntt_ref_harvey_lazy_dbl(_ptr(a1), _ptr(a2), N, q, _ptr(w), _ptr(w_con))
    _reduce(a1, q, 4)
    _reduce(a2, q, 4)


def inv_ntt_ref_harvey(a, N, q, n_inv, n_inv_con, word_size, w, w_con):
    _lib.inv_ntt_ref_harvey(_ptr(a), N, q, _mulop(n_inv, n_inv_con), word_size, _ptr(w), _ptr(w_con))


def fwd_ntt_radix4(a, N, q, w, w_con):
    _lib.fwd_ntt_radix4_lazy(_ptr(a), N, q, _ptr(w), _ptr(w_con))
    _reduce(a, q, 8)


def fwd_ntt_radix4x4(a, N, q, w, w_con):
    _lib.fwd_ntt_radix4x4_lazy(_ptr(a), N, q, _ptr(w), _ptr(w_con))
    _reduce(a, q, 8)


def inv_ntt_radix4(a, N, q, n_inv, n_inv_con, w, w_con):
    _lib.inv_ntt_radix4(_ptr(a), N, q, _mulop(n_inv, n_inv_con), _ptr(w), _ptr(w_con))


def fwd_ntt_seal(a, N, q, w, w_con):
    _lib.fwd_ntt_seal_lazy(_ptr(a), N, q, _ptr(w), _ptr(w_con))
    _reduce(a, q, 4)


def inv_ntt_seal(a, N, q, n_inv, n_inv_con, w, w_con):
    _lib.inv_ntt_seal(_ptr(a), N, q, n_inv, n_inv_con, _ptr(w), _ptr(w_con))
