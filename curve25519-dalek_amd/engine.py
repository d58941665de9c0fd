"""ctypes binding of libc25519hip.so (include/c25519_hip.h).

PyTorch is plumbing here: device buffers are torch uint8 CUDA tensors, the engine enqueues on
torch's current stream, and torch.distributed carries the multi-GPU exchange.  The arithmetic is
all in the HIP library; if it is missing this module raises -- it never falls back to a CPU path.
"""
import ctypes as C
import os

import numpy as np

OK, NONE, SCALAR_FORMAT, VERIFY, ARRAY_LENGTH, PREHASHED_CONTEXT_LENGTH = 0, 1, 2, 3, 4, 5
DOMAIN_SEPARATOR_LENGTH = 6      # hash-to-curve: a DST of 0 or more than 255 bytes
H2C_NU, H2C_RO = 0, 1            # c25519_edwards_hash_to_curve_batch mode: encode_to_curve / hash_to_curve
LIZARD_NONE, LIZARD_OK, LIZARD_BAD_ENCODING = 0, 1, 2      # per-item status of the Lizard decode
MONTGOMERY_MAX_BITS = 512        # C25519_MONTGOMERY_MAX_BITS: the longest bit string of montgomery_mul_bits_be
FMT_EDWARDS_Y, FMT_RISTRETTO, FMT_RAW160 = 0, 1, 2
POINT_DECODES, POINT_SMALL_ORDER, POINT_TORSION_FREE = 1, 2, 4      # flags of c25519_point_order_checks_batch
POINT_ADD, POINT_SUB = 0, 1                   # c25519_point_add_batch op
POINT_NEG, POINT_MUL_BY_COFACTOR = 0, 1       # c25519_point_map_batch op
Z_TRANSCRIPT, Z_DEVICE = 0, 1
FLAG_VARTIME_TABLES = 0x100      # c25519_ctx_create: fast secret-indexed tables for mul_base / mul_batch / sign / keygen (public scalars only)

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class EngineError(RuntimeError):
    pass


_LIB_OVERRIDE = None


def lib_path():
    """the library this process loads: lib/libc25519hip.so unless select_library() named another build.  Nothing here reads the environment."""
    return _LIB_OVERRIDE or os.path.join(_HERE, "lib", "libc25519hip.so")


def select_library(path):
    """Load another build of the same sources (the tuning build lib/libc25519hip_tune.so with its A/B knobs, the bound-checking debug build, a variant
    made by tools/build_variant.sh) instead of the release library.  An explicit call of the test harness / an A/B tool, before the first Engine; the
    package itself never looks at the environment for this (a crypto library must not be substitutable through a variable)."""
    global _LIB_OVERRIDE
    path = os.path.abspath(path)
    if _LIB is not None and os.path.abspath(lib_path()) != path:
        raise EngineError("select_library(%s): %s is already loaded in this process" % (path, lib_path()))
    _LIB_OVERRIDE = path


# every exported entry point of include/c25519_hip.h: name -> (restype, argtypes)
_vp, _u64, _i32 = C.c_void_p, C.c_uint64, C.c_int32
_SIGS = {
    "c25519_ctx_create": (_vp, [C.c_int, C.c_uint32]),
    "c25519_ctx_destroy": (None, [_vp]),
    "c25519_ctx_set_stream": (_i32, [_vp, _vp]),
    "c25519_ctx_synchronize": (_i32, [_vp]),
    "c25519_last_error": (C.c_char_p, [_vp]),
    "c25519_last_kernel_ms": (C.c_float, [_vp]),
    "c25519_phase_ms": (C.c_float, [_vp, C.c_uint32, C.c_int]),
    "c25519_last_call_phase_ms": (C.c_float, [_vp, C.c_int, _vp]),
    "c25519_debug_batch_zs": (_i32, [_vp, _vp, _vp, _vp, _vp, _u64, C.c_uint32, _vp]),
    "c25519_debug_sort": (_i32, [_vp, _vp, _u64, _u64, C.c_int32]),
    "c25519_mul_base_batch_dev": (_i32, [_vp, _vp, _u64, C.c_int, _vp]),
    "c25519_mul_base_batch": (_i32, [_vp, _vp, _u64, C.c_int, _vp]),
    "c25519_mul_base_batch_vartime_dev": (_i32, [_vp, _vp, _u64, C.c_int, _vp]),
    "c25519_mul_base_clamped_batch_dev": (_i32, [_vp, _vp, _u64, C.c_int, _vp]),
    "c25519_mul_base_clamped_batch": (_i32, [_vp, _vp, _u64, C.c_int, _vp]),
    "c25519_basetable_create": (_vp, [_vp, _vp, C.c_int]),
    "c25519_basetable_destroy": (None, [_vp, _vp]),
    "c25519_mul_table_batch_dev": (_i32, [_vp, _vp, _vp, _u64, C.c_int, _vp]),
    "c25519_mul_table_batch": (_i32, [_vp, _vp, _vp, _u64, C.c_int, _vp]),
    "c25519_x25519_contributory_batch_dev": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "c25519_x25519_contributory_batch": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "c25519_mul_clamped_batch_dev": (_i32, [_vp, _vp, _vp, _u64, C.c_int, C.c_int, _vp, _vp]),
    "c25519_mul_clamped_batch": (_i32, [_vp, _vp, _vp, _u64, C.c_int, C.c_int, _vp, _vp]),
    "c25519_point_order_checks_batch_dev": (_i32, [_vp, _vp, _u64, C.c_int, C.c_int, _vp]),
    "c25519_point_order_checks_batch": (_i32, [_vp, _vp, _u64, C.c_int, C.c_int, _vp]),
    "c25519_host_alloc": (_vp, [C.c_size_t]),
    "c25519_host_free": (None, [_vp]),
    "c25519_last_ffi_ms": (C.c_double, [_vp, _vp, _vp]),
    "c25519_ctx_trim": (_i32, [_vp]),
    "c25519_last_kernel_name": (C.c_char_p, [_vp, C.c_int]),
    "c25519_x25519_batch_dev": (_i32, [_vp, _vp, _vp, _u64, _vp]),
    "c25519_x25519_batch": (_i32, [_vp, _vp, _vp, _u64, _vp]),
    "c25519_x25519_base_batch_dev": (_i32, [_vp, _vp, _u64, _vp]),
    "c25519_x25519_base_batch": (_i32, [_vp, _vp, _u64, _vp]),
    "c25519_decompress_batch_dev": (_i32, [_vp, _vp, _u64, C.c_int, _vp, _vp]),
    "c25519_decompress_batch": (_i32, [_vp, _vp, _u64, C.c_int, _vp, _vp]),
    "c25519_compress_batch_dev": (_i32, [_vp, _vp, _u64, C.c_int, _vp]),
    "c25519_compress_batch": (_i32, [_vp, _vp, _u64, C.c_int, _vp]),
    "c25519_to_montgomery_batch_dev": (_i32, [_vp, _vp, _u64, _vp]),
    "c25519_to_montgomery_batch": (_i32, [_vp, _vp, _u64, _vp]),
    "c25519_msm_vartime_dev": (_i32, [_vp, _vp, _vp, _u64, C.c_int, C.c_int, _vp]),
    "c25519_msm_vartime": (_i32, [_vp, _vp, _vp, _u64, C.c_int, C.c_int, _vp]),
    "c25519_msm_partial_dev": (_i32, [_vp, _vp, _vp, _u64, C.c_int, _vp]),
    "c25519_fold_partials": (_i32, [_vp, _vp, _u64, C.c_int, _vp]),
    "c25519_msm_partial_record_dev": (_i32, [_vp, _vp, _vp, _u64, C.c_int, _vp]),
    "c25519_fold_partial_records": (_i32, [_vp, _vp, _u64, C.c_int, _vp]),
    "c25519_partial_record_pack": (_i32, [_vp, _i32, _vp, _vp]),
    "ed25519_batch_hram_dev": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp]),
    "ed25519_batch_transcript_zs": (_i32, [_vp, _vp, _u64, _vp]),
    "ed25519_verify_batch_record_dev": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp]),
    "ed25519_fold_verify_records": (_i32, [_vp, _vp, _u64]),
    "c25519_msm_vartime_multi": (_i32, [_vp, _i32, _vp, _vp, _u64, C.c_int, C.c_int, _vp]),
    "ed25519_verify_batch_multi": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _u64, C.c_uint32]),
    "ed25519_verify_batch_dev": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, C.c_uint32]),
    "ed25519_verify_batch": (_i32, [_vp, _vp, _vp, _vp, _vp, _u64, C.c_uint32]),
    "ed25519_verify_batch_keys_dev": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _u64, C.c_uint32]),
    "ed25519_verify_batch_keys": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _u64, C.c_uint32]),
    "c25519_mul_batch_dev": (_i32, [_vp, _vp, _vp, _u64, C.c_int, C.c_int, _vp, _vp]),
    "c25519_mul_batch": (_i32, [_vp, _vp, _vp, _u64, C.c_int, C.c_int, _vp, _vp]),
    "c25519_double_base_batch_dev": (_i32, [_vp, _vp, _vp, _vp, _u64, C.c_int, C.c_int, _vp, _vp]),
    "c25519_double_base_batch": (_i32, [_vp, _vp, _vp, _vp, _u64, C.c_int, C.c_int, _vp, _vp]),
    "c25519_last_call_host_us": (_i32, [_vp, _vp]),
    "c25519_ctx_counter": (_u64, [_vp, _i32]),
    "ed25519_verify_each_dev": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, C.c_int, _vp]),
    "ed25519_verify_each": (_i32, [_vp, _vp, _vp, _vp, _vp, _u64, C.c_int, _vp]),
    "ed25519_verify_each_prehashed_dev": (_i32, [_vp, _vp, C.c_char_p, C.c_uint32, _vp, _vp, _u64, C.c_int, _vp]),
    "ed25519_verify_each_prehashed": (_i32, [_vp, _vp, C.c_char_p, C.c_uint32, _vp, _vp, _u64, C.c_int, _vp]),
    "ed25519_sign_batch_prehashed_dev": (_i32, [_vp, _vp, _vp, C.c_char_p, C.c_uint32, _u64, _vp, _vp]),
    "ed25519_sign_batch_prehashed": (_i32, [_vp, _vp, _vp, C.c_char_p, C.c_uint32, _u64, _vp, _vp]),
    "ed25519_keygen_batch_dev": (_i32, [_vp, _vp, _u64, _vp]),
    "ed25519_sign_batch_dev": (_i32, [_vp, _vp, _vp, _vp, _u64, _u64, _vp, _vp]),
    "ed25519_sign_batch": (_i32, [_vp, _vp, _vp, _vp, _u64, _vp, _vp]),
    "c25519_precomp_create": (_vp, [_vp, _vp, _u64, C.c_int]),
    "c25519_precomp_destroy": (None, [_vp, _vp]),
    "c25519_precomp_len": (_u64, [_vp]),
    "c25519_precomp_msm_vartime": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, C.c_int, C.c_int, _vp]),
    "c25519_precomp_msm_vartime_rows_dev": (_i32, [_vp, _vp, _vp, _u64, _u64, _i32, C.c_int, _vp]),
    "c25519_precomp_msm_vartime_rows": (_i32, [_vp, _vp, _vp, _u64, _u64, _i32, C.c_int, _vp]),
    "c25519_precomp_msm_vartime_rows_plan": (_i32, [_u64, _u64, _vp]),
    "c25519_precomp_rows_table_bytes": (_u64, [_vp]),
    "c25519_precomp_msm_vartime_mixed_rows_dev": (_i32, [_vp, _vp, _vp, _u64, _u64, _vp, _vp, _u64, C.c_int, _vp, _i32, C.c_int, _vp, _vp]),
    "c25519_precomp_msm_vartime_mixed_rows": (_i32, [_vp, _vp, _vp, _u64, _u64, _vp, _vp, _u64, C.c_int, _vp, _i32, C.c_int, _vp, _vp]),
    "c25519_precomp_msm_vartime_mixed_rows_plan": (_i32, [_u64, _u64, _vp, _vp]),
    "c25519_precomp_msm_vartime_mixed_rows_fold_dev": (_i32, [_vp, _vp, _vp, _u64, _u64, _vp, _vp, _u64, C.c_int, _vp, _vp, _i32, C.c_int, _vp]),
    "c25519_precomp_msm_vartime_mixed_rows_fold": (_i32, [_vp, _vp, _vp, _u64, _u64, _vp, _vp, _u64, C.c_int, _vp, _vp, _i32, C.c_int, _vp]),
    "c25519_precomp_msm_vartime_mixed_rows_fold_plan": (_i32, [_u64, _u64, _vp, _i32, _vp]),
    "c25519_msm_consttime": (_i32, [_vp, _vp, _vp, _u64, C.c_int, C.c_int, _vp]),
    "c25519_double_and_compress_batch_dev": (_i32, [_vp, _vp, _u64, _vp]),
    "c25519_double_and_compress_batch": (_i32, [_vp, _vp, _u64, _vp]),
    "c25519_scalar_invert_batch": (_i32, [_vp, _vp, _u64, _vp]),
    "c25519_ristretto_from_uniform_bytes_batch_dev": (_i32, [_vp, _vp, _u64, C.c_int, _vp]),
    "c25519_ristretto_from_uniform_bytes_batch": (_i32, [_vp, _vp, _u64, C.c_int, _vp]),
    "c25519_ristretto_map_to_curve_batch_dev": (_i32, [_vp, _vp, _u64, C.c_int, _vp]),
    "c25519_ristretto_map_to_curve_batch": (_i32, [_vp, _vp, _u64, C.c_int, _vp]),
    "c25519_ristretto_hash_from_bytes_batch_dev": (_i32, [_vp, _vp, _vp, _u64, _u64, C.c_int, _vp]),
    "c25519_ristretto_hash_from_bytes_batch": (_i32, [_vp, _vp, _vp, _u64, C.c_int, _vp]),
    "c25519_edwards_hash_to_curve_batch_dev": (_i32, [_vp, _vp, _vp, _u64, _u64, C.c_char_p, C.c_uint32, C.c_int, C.c_int, _vp]),
    "c25519_edwards_hash_to_curve_batch": (_i32, [_vp, _vp, _vp, _u64, C.c_char_p, C.c_uint32, C.c_int, C.c_int, _vp]),
    "c25519_ristretto_lizard_encode_sha256_batch_dev": (_i32, [_vp, _vp, _u64, C.c_int, _vp]),
    "c25519_ristretto_lizard_encode_sha256_batch": (_i32, [_vp, _vp, _u64, C.c_int, _vp]),
    "c25519_ristretto_lizard_decode_sha256_batch_dev": (_i32, [_vp, _vp, _u64, C.c_int, _vp, _vp]),
    "c25519_ristretto_lizard_decode_sha256_batch": (_i32, [_vp, _vp, _u64, C.c_int, _vp, _vp]),
    "c25519_ristretto_map_to_curve_inverse_batch_dev": (_i32, [_vp, _vp, _u64, C.c_int, _vp, _vp, _vp]),
    "c25519_ristretto_map_to_curve_inverse_batch": (_i32, [_vp, _vp, _u64, C.c_int, _vp, _vp, _vp]),
    "c25519_montgomery_mul_batch_dev": (_i32, [_vp, _vp, _vp, _u64, _vp]),
    "c25519_montgomery_mul_batch": (_i32, [_vp, _vp, _vp, _u64, _vp]),
    "c25519_montgomery_mul_bits_be_batch_dev": (_i32, [_vp, _vp, C.c_uint32, _vp, _u64, _vp]),
    "c25519_montgomery_mul_bits_be_batch": (_i32, [_vp, _vp, C.c_uint32, _vp, _u64, _vp]),
    "c25519_montgomery_mul_base_batch_dev": (_i32, [_vp, _vp, _u64, _vp]),
    "c25519_montgomery_mul_base_batch": (_i32, [_vp, _vp, _u64, _vp]),
    "c25519_montgomery_to_edwards_batch_dev": (_i32, [_vp, _vp, _vp, _u64, C.c_int, _vp, _vp]),
    "c25519_montgomery_to_edwards_batch": (_i32, [_vp, _vp, _vp, _u64, C.c_int, _vp, _vp]),
    "c25519_point_add_batch_dev": (_i32, [_vp, _vp, _vp, _u64, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "c25519_point_add_batch": (_i32, [_vp, _vp, _vp, _u64, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "c25519_point_map_batch_dev": (_i32, [_vp, _vp, _u64, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "c25519_point_map_batch": (_i32, [_vp, _vp, _u64, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "c25519_point_eq_batch_dev": (_i32, [_vp, _vp, _vp, _u64, C.c_int, C.c_int, _vp, _vp]),
    "c25519_point_eq_batch": (_i32, [_vp, _vp, _vp, _u64, C.c_int, C.c_int, _vp, _vp]),
    "c25519_point_sum_segments_dev": (_i32, [_vp, _vp, _u64, C.c_int, _vp, _u64, C.c_int, _vp, _vp]),
    "c25519_point_sum_segments": (_i32, [_vp, _vp, _u64, C.c_int, _vp, _u64, C.c_int, _vp, _vp]),
    "c25519_msm_vartime_segments_dev": (_i32, [_vp, _vp, _vp, _u64, C.c_int, _vp, _u64, C.c_int, _vp, _vp]),
    "c25519_msm_vartime_segments": (_i32, [_vp, _vp, _vp, _u64, C.c_int, _vp, _u64, C.c_int, _vp, _vp]),
    "c25519_msm_vartime_segments_plan": (_i32, [_vp, _u64, _vp]),
    "c25519_msm_vartime_segments_routes": (_i32, [_vp, _u64, _vp]),
    "ed25519_verify_batch_segments_dev": (_i32, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _u64, _vp, _u64, C.c_uint32, _vp]),
    "ed25519_verify_batch_segments": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _u64, _vp, _u64, C.c_uint32, _vp]),
    "ed25519_verify_batch_segments_plan": (_i32, [_vp, _u64, _vp]),
    "ed25519_batch_transcript_zs_segments_dev": (_i32, [_vp, _vp, _vp, _u64, _vp, _u64, _vp]),
    "ed25519_batch_transcript_zs_segments": (_i32, [_vp, _vp, _vp, _u64, _vp, _u64, _vp]),
    "ed25519_batch_transcript_zs_segments_plan": (_i32, [_vp, _u64, _vp]),
    "c25519_microbench": (C.c_double, [_vp, C.c_int, C.c_int]),
    "c25519_selftest_field": (_i32, [_vp, C.c_int, C.c_int, _vp, _vp, _u64, _vp]),
    "c25519_selftest_scalar": (_i32, [_vp, C.c_int, _vp, _vp, _u64, _vp]),
    "c25519_selftest_point": (_i32, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _u64, _vp]),
    "c25519_debug_workspace_count": (_i32, [_vp]),
    "c25519_debug_workspace_info": (_i32, [_vp, C.c_int, _vp, _vp]),
    "c25519_debug_workspace_read": (_i32, [_vp, C.c_int, _u64, _u64, _vp]),
    "c25519_debug_workspace_zero": (_i32, [_vp]),
    "c25519_msm_geometry": (_i32, [_u64, _vp, _vp, _vp, _vp, _vp]),
    "c25519_msm_route": (_i32, [_i32, _u64, _i32, _i32, _vp]),
}
ABI_SYMBOLS = list(_SIGS)


def load_library():
    """Load the HIP library (after torch, so both share one HIP runtime).  Raises if absent."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise EngineError("HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback)" % path)
    try:
        import torch  # noqa: F401  (loads libamdhip64 first; our library binds to the same runtime)
    except Exception:  # pragma: no cover
        pass
    lib = C.CDLL(path)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)  # AttributeError here = the library does not export the ABI
        fn.restype, fn.argtypes = res, args
    _LIB = lib
    return lib


_PT = {FMT_EDWARDS_Y: 32, FMT_RISTRETTO: 32, FMT_RAW160: 160}
PARTIAL_RECORD_BYTES = 9024      # C25519_PARTIAL_RECORD_BYTES
MSM_SEGMENT_DIRECT_MAX = 64      # C25519_MSM_SEGMENT_DIRECT_MAX: the longest segment msm_vartime_segments runs one per lane
MSM_SEGMENT_WAVE_MAX = 2048      # C25519_MSM_SEGMENT_WAVE_MAX: the longest segment it runs one per wave
MSM_SEGMENT_PASS_TERMS = 1 << 18     # C25519_MSM_SEGMENT_PASS_TERMS: most terms whose tables are resident at once
MSM_SEGMENT_BUCKET_MAX = 32768  # C25519_MSM_SEGMENT_BUCKET_MAX: the longest segment on its bucket route; longer ones take the single-MSM path
MSM_SEGMENT_BUCKET_PASS_TERMS = 1 << 20      # C25519_MSM_SEGMENT_BUCKET_PASS_TERMS: most terms of one pass of the bucket route
# what msm_vartime_segments_routes reports per segment (C25519_MSM_SEGMENT_ROUTE_*)
MSM_SEGMENT_ROUTE_LANE, MSM_SEGMENT_ROUTE_WAVE, MSM_SEGMENT_ROUTE_BUCKET, MSM_SEGMENT_ROUTE_SINGLE = 0, 1, 2, 3
VERIFY_SEGMENT_MAX = 1023        # ED25519_VERIFY_SEGMENT_MAX: the longest segment verify_batch_segments runs through the segmented MSM
TRANSCRIPT_SEGMENT_DEVICE_MAX = 256      # ED25519_TRANSCRIPT_SEGMENT_DEVICE_MAX: the longest segment whose Merlin transcript verify_batch_segments runs on the device
PRECOMP_ROWS_MAX_POINTS = 4096   # C25519_PRECOMP_ROWS_MAX_POINTS: the largest handle precomp_msm_vartime_rows serves (64 KB of comb table per point)
PRECOMP_ROWS_AUTO, PRECOMP_ROWS_LANE, PRECOMP_ROWS_WAVE = 0, 1, 2      # C25519_PRECOMP_ROWS_*: its route argument (one lane / one wave per row)
PRECOMP_ROWS_LANE_WIDTH = 16     # C25519_PRECOMP_ROWS_LANE_WIDTH: AUTO takes the lane route only for rows narrower than this ...
PRECOMP_ROWS_LANE_MIN_ROWS = 32768       # C25519_PRECOMP_ROWS_LANE_MIN_ROWS: ... and only from this many rows
PRECOMP_MIXED_LANE_DYN_MAX = 16  # C25519_PRECOMP_MIXED_LANE_DYN_MAX: precomp_msm_vartime_mixed_rows AUTO takes the lane route only if no row has more dynamic terms ...
PRECOMP_MIXED_LANE_BASE_ROWS = 1024      # C25519_PRECOMP_MIXED_LANE_BASE_ROWS: ... and only from BASE_ROWS + ROWS_PER_TERM * (w + the longest row's dynamic terms) rows
PRECOMP_MIXED_LANE_ROWS_PER_TERM = 320   # C25519_PRECOMP_MIXED_LANE_ROWS_PER_TERM


def _seg_off_host(seg_off):
    """m + 1 segment offsets as a contiguous uint64 array on the host (a sequence, an array or a CPU tensor)"""
    if hasattr(seg_off, "is_cuda"):
        assert not seg_off.is_cuda, "seg_off stays on the host"
        seg_off = seg_off.numpy()
    off = np.ascontiguousarray(np.asarray(seg_off, dtype=np.uint64).reshape(-1))
    assert off.shape[0] >= 1
    return off


def _np8(x, width):
    a = np.ascontiguousarray(np.frombuffer(x, dtype=np.uint8) if isinstance(x, (bytes, bytearray)) else x, dtype=np.uint8)
    return a.reshape(-1, width)


class Engine:
    """One engine = one GPU + one stream (`c25519_ctx`).  Tensor methods (`*_t`) take/return torch
    uint8 CUDA tensors already resident in HBM; the plain methods take/return numpy arrays / bytes
    and go through the host-pointer entry points (PCIe copies included)."""

    def __init__(self, device=0, window=0, flags=0):
        """window: fixed-base table algorithm (c25519_ctx_create flags & 0x1f); flags: FLAG_VARTIME_TABLES or 0"""
        import torch
        self.torch = torch
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise EngineError("no GPU visible to PyTorch-ROCm: the engine has no CPU fallback")
        self.device = torch.device("cuda", device)
        # (round 5 let C25519_DEFAULT_WINDOW / C25519_DEFAULT_VARTIME_TABLES steer these two from the environment: a default context could be talked out of
        #  its constant-time tables by a variable.  The arguments are the only way now; tests pass them.)
        self.ctx = self.lib.c25519_ctx_create(device, (window & 0x1f) | flags)
        if not self.ctx:
            raise EngineError("c25519_ctx_create(%d) failed" % device)
        self._bind_stream()

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.c25519_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- plumbing ----------------------------------------------------------------------------
    def _bind_stream(self):
        if not self.ctx:
            raise EngineError("this Engine has been closed")
        st = self.torch.cuda.current_stream(self.device).cuda_stream
        self.lib.c25519_ctx_set_stream(self.ctx, C.c_void_p(st))

    def _chk(self, st, allowed=(OK,)):
        if st < 0:
            raise EngineError("HIP error %d: %s" % (-st, self.lib.c25519_last_error(self.ctx).decode()))
        if st not in allowed:
            raise EngineError("unexpected status %d" % st)
        return st

    def _t(self, t, width):
        torch = self.torch
        assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous(), "need a contiguous uint8 CUDA tensor"
        assert t.numel() % width == 0
        assert t.data_ptr() % 16 == 0, "device buffers must be 16-byte aligned"
        return t.numel() // width

    def last_call_host_us(self):
        """host clock of the latest synchronous MSM / verify_batch call, microseconds since its entry: (upload enqueued, kernels enqueued, results on the host, folded)"""
        out = (C.c_double * 4)()
        self._chk(self.lib.c25519_last_call_host_us(self.ctx, out))
        return tuple(out)

    def counter(self, which):
        """event counters of the context (c25519_ctx_counter): 0 publications that blocked on the stream, 1 lost publications (re-run), 2 directly published calls"""
        return int(self.lib.c25519_ctx_counter(self.ctx, which))

    def synchronize(self):
        self._chk(self.lib.c25519_ctx_synchronize(self.ctx))

    def last_kernel_ms(self):
        return float(self.lib.c25519_last_kernel_ms(self.ctx))

    def phase_ms(self, back=0, phase=0):
        return float(self.lib.c25519_phase_ms(self.ctx, back, phase))

    def last_call_phase_ms(self, phase=0):
        """-> (ms summed over the passes of the latest MSM / verify_batch call, number of passes)"""
        passes = C.c_uint32(0)
        ms = float(self.lib.c25519_last_call_phase_ms(self.ctx, phase, C.byref(passes)))
        return ms, int(passes.value)

    def selftest_field(self, op, a_limbs, b_limbs=None, chain=0):
        """one field operation per row on the GPU: (n, 10) uint32 limbs in -> (n, 32) canonical bytes (c25519_selftest_field)"""
        a = np.ascontiguousarray(a_limbs, dtype=np.uint32).reshape(-1, 10); n = a.shape[0]
        b = None if b_limbs is None else np.ascontiguousarray(b_limbs, dtype=np.uint32).reshape(-1, 10)
        assert b is None or b.shape[0] == n
        out = np.empty((n, 32), dtype=np.uint8)
        self._bind_stream()
        self._chk(self.lib.c25519_selftest_field(self.ctx, op, chain, a.ctypes.data, b.ctypes.data if b is not None else None, n, out.ctypes.data))
        return out

    def selftest_point(self, op, p, q=None, aux=None, chain=0):
        """one point formula per row on the GPU: (n, 40) uint32 limbs X Y Z T, q (n, 40) and aux (n,) as the op takes them -> (n, 128) canonical X Y Z T (c25519_selftest_point)"""
        p = np.ascontiguousarray(p, dtype=np.uint32).reshape(-1, 40); n = p.shape[0]
        q = None if q is None else np.ascontiguousarray(q, dtype=np.uint32).reshape(-1, 40)
        aux = None if aux is None else np.ascontiguousarray(aux, dtype=np.uint32).reshape(-1)
        assert (q is None or q.shape[0] == n) and (aux is None or aux.shape[0] == n)
        out = np.empty((n, 128), dtype=np.uint8)
        self._bind_stream()
        self._chk(self.lib.c25519_selftest_point(self.ctx, op, chain, p.ctypes.data, q.ctypes.data if q is not None else None, aux.ctypes.data if aux is not None else None, n, out.ctypes.data))
        return out

    def selftest_scalar(self, op, a_words, b_words=None):
        """one sc28.h operation per row on the GPU: (n, 16) uint32 per operand -> (n, 32) bytes (c25519_selftest_scalar)"""
        a = np.ascontiguousarray(a_words, dtype=np.uint32).reshape(-1, 16); n = a.shape[0]
        b = None if b_words is None else np.ascontiguousarray(b_words, dtype=np.uint32).reshape(-1, 16)
        assert b is None or b.shape[0] == n
        out = np.empty((n, 32), dtype=np.uint8)
        self._bind_stream()
        self._chk(self.lib.c25519_selftest_scalar(self.ctx, op, a.ctypes.data, b.ctypes.data if b is not None else None, n, out.ctypes.data))
        return out

    def workspaces(self):
        """-> {name: bytes} of every device workspace of the context and its peer, read back after all its streams have drained (c25519_debug_workspace_*)"""
        out = {}
        for i in range(self.lib.c25519_debug_workspace_count(self.ctx)):
            name, cap = C.c_char_p(), C.c_uint64(0)
            self._chk(self.lib.c25519_debug_workspace_info(self.ctx, i, C.byref(name), C.byref(cap)))
            buf = np.zeros(cap.value, dtype=np.uint8)
            if cap.value:
                self._chk(self.lib.c25519_debug_workspace_read(self.ctx, i, 0, cap.value, buf.ctypes.data))
            out[name.value.decode()] = buf
        return out

    def workspace_zero(self):
        """zero every device workspace over its whole capacity (c25519_debug_workspace_zero: the one write of the debug window)"""
        self._chk(self.lib.c25519_debug_workspace_zero(self.ctx))

    def microbench(self, which, iters=2000):
        self._bind_stream()
        return float(self.lib.c25519_microbench(self.ctx, which, iters))

    # -- device-tensor API -------------------------------------------------------------------
    def mul_base_batch_t(self, scalars, out_fmt=FMT_EDWARDS_Y, out=None):
        n = self._t(scalars, 32)
        if out is None:
            out = self.torch.empty((n, _PT[out_fmt]), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        self._chk(self.lib.c25519_mul_base_batch_dev(self.ctx, scalars.data_ptr(), n, out_fmt, out.data_ptr()))
        return out

    def mul_base_batch_vartime_t(self, scalars, out_fmt=FMT_EDWARDS_Y, out=None):
        """scalars declared PUBLIC: the fast tables whatever the context's flags"""
        n = self._t(scalars, 32)
        if out is None:
            out = self.torch.empty((n, _PT[out_fmt]), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        self._chk(self.lib.c25519_mul_base_batch_vartime_dev(self.ctx, scalars.data_ptr(), n, out_fmt, out.data_ptr()))
        return out

    def x25519_base_batch_t(self, k, out=None):
        n = self._t(k, 32)
        if out is None:
            out = self.torch.empty((n, 32), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        self._chk(self.lib.c25519_x25519_base_batch_dev(self.ctx, k.data_ptr(), n, out.data_ptr()))
        return out

    def x25519_batch_t(self, k, u, out=None):
        n = self._t(k, 32)
        assert self._t(u, 32) == n
        if out is None:
            out = self.torch.empty((n, 32), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        self._chk(self.lib.c25519_x25519_batch_dev(self.ctx, k.data_ptr(), u.data_ptr(), n, out.data_ptr()))
        return out

    def decompress_batch_t(self, enc, in_fmt=FMT_EDWARDS_Y):
        n = self._t(enc, 32)
        pts = self.torch.empty((n, 160), dtype=self.torch.uint8, device=self.device)
        ok = self.torch.empty((n,), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        st = self._chk(self.lib.c25519_decompress_batch_dev(self.ctx, enc.data_ptr(), n, in_fmt, pts.data_ptr(), ok.data_ptr()), (OK, NONE))
        return st, pts, ok

    def compress_batch_t(self, pts, out_fmt=FMT_EDWARDS_Y):
        n = self._t(pts, 160)
        out = self.torch.empty((n, 32), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        self._chk(self.lib.c25519_compress_batch_dev(self.ctx, pts.data_ptr(), n, out_fmt, out.data_ptr()))
        return out

    def msm_vartime_t(self, scalars, points, in_fmt=FMT_RAW160, out_fmt=FMT_EDWARDS_Y):
        """-> (status, bytes).  status NONE mirrors Option::None of the reference."""
        n = self._t(scalars, 32)
        assert self._t(points, _PT[in_fmt]) == n
        out = C.create_string_buffer(_PT[out_fmt])
        self._bind_stream()
        st = self._chk(self.lib.c25519_msm_vartime_dev(self.ctx, scalars.data_ptr(), points.data_ptr(), n, in_fmt, out_fmt, out), (OK, NONE))
        return st, out.raw

    def msm_partial_t(self, scalars, points, in_fmt=FMT_RAW160):
        n = self._t(scalars, 32)
        assert self._t(points, _PT[in_fmt]) == n
        out = C.create_string_buffer(160)
        self._bind_stream()
        st = self._chk(self.lib.c25519_msm_partial_dev(self.ctx, scalars.data_ptr(), points.data_ptr(), n, in_fmt, out), (OK, NONE))
        return st, out.raw

    def msm_partial_record_t(self, scalars, points, in_fmt=FMT_RAW160, out=None):
        """This rank's share of a sharded MSM as a partial-result RECORD in device memory (uint8 tensor of
        PARTIAL_RECORD_BYTES).  Enqueue only: nothing has waited for the host when this returns."""
        n = self._t(scalars, 32)
        assert self._t(points, _PT[in_fmt]) == n
        if out is None:
            out = self.torch.empty((PARTIAL_RECORD_BYTES,), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        self._chk(self.lib.c25519_msm_partial_record_dev(self.ctx, scalars.data_ptr(), points.data_ptr(), n, in_fmt, out.data_ptr()))
        return out

    def batch_hram_t(self, msgs, msg_off, sigs, pks):
        """H(R_i || A_i || M_i) of this shard: uint8 device tensor of n * 64 + 64 bytes (the trailer holds the counters of
        ed25519_batch_hram_dev).  Enqueue only."""
        n = self._t(sigs, 64)
        assert self._t(pks, 32) == n and msg_off.numel() == n + 1
        out = self.torch.empty((n * 64 + 64,), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        self._chk(self.lib.ed25519_batch_hram_dev(self.ctx, msgs.data_ptr(), msg_off.data_ptr(), msgs.numel(), sigs.data_ptr(), pks.data_ptr(), n, out.data_ptr()))
        return out

    def verify_batch_record_t(self, sigs, pks, hram, z16, pk_points=None):
        """This shard's share of the batch equation with GIVEN z_i (n x 16 device tensor) and its hram buffer from
        batch_hram_t, as a partial-result record in device memory.  Enqueue only."""
        n = self._t(sigs, 64)
        assert self._t(pks, 32) == n and hram.numel() == n * 64 + 64 and z16.numel() == n * 16
        assert hram.is_cuda and z16.is_cuda and z16.is_contiguous() and (n == 0 or z16.data_ptr() % 16 == 0)
        if pk_points is not None:
            assert self._t(pk_points, 160) == n
        out = self.torch.empty((PARTIAL_RECORD_BYTES,), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        self._chk(self.lib.ed25519_verify_batch_record_dev(self.ctx, sigs.data_ptr(), pks.data_ptr(), pk_points.data_ptr() if pk_points is not None else None,
                                                           hram.data_ptr(), z16.data_ptr(), n, out.data_ptr()))
        return out

    def fold_partials(self, partials, out_fmt=FMT_EDWARDS_Y):
        blob = b"".join(partials)
        out = C.create_string_buffer(_PT[out_fmt])
        self._chk(self.lib.c25519_fold_partials(self.ctx, blob, len(partials), out_fmt, out))
        return out.raw

    def verify_batch_t(self, msgs, msg_off, sigs, pks, z_mode=Z_TRANSCRIPT, pk_points=None):
        """msgs: uint8 CUDA tensor of the concatenated messages; msg_off: int64/uint64 CUDA tensor (n+1);
        pk_points: optional (n, 160) raw points of the keys (VerifyingKey.point), skips their decompression."""
        n = self._t(sigs, 64)
        assert self._t(pks, 32) == n and msg_off.numel() == n + 1
        if pk_points is not None:
            assert self._t(pk_points, 160) == n
        self._bind_stream()
        return self._chk(self.lib.ed25519_verify_batch_keys_dev(self.ctx, msgs.data_ptr(), msg_off.data_ptr(), msgs.numel(),
                                                                sigs.data_ptr(), pks.data_ptr(), pk_points.data_ptr() if pk_points is not None else None,
                                                                n, z_mode),
                         (OK, NONE, SCALAR_FORMAT, VERIFY))

    def mul_batch_t(self, scalars, points, in_fmt=FMT_RAW160, out_fmt=FMT_EDWARDS_Y):
        n = self._t(scalars, 32)
        assert self._t(points, _PT[in_fmt]) == n
        out = self.torch.empty((n, _PT[out_fmt]), dtype=self.torch.uint8, device=self.device)
        ok = self.torch.empty((n,), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        self._chk(self.lib.c25519_mul_batch_dev(self.ctx, scalars.data_ptr(), points.data_ptr(), n, in_fmt, out_fmt, out.data_ptr(), ok.data_ptr()))
        return out, ok

    def double_base_batch_t(self, a, A, b, in_fmt=FMT_RAW160, out_fmt=FMT_EDWARDS_Y):
        n = self._t(a, 32)
        assert self._t(A, _PT[in_fmt]) == n and self._t(b, 32) == n
        out = self.torch.empty((n, _PT[out_fmt]), dtype=self.torch.uint8, device=self.device)
        ok = self.torch.empty((n,), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        self._chk(self.lib.c25519_double_base_batch_dev(self.ctx, a.data_ptr(), A.data_ptr(), b.data_ptr(), n, in_fmt, out_fmt, out.data_ptr(), ok.data_ptr()))
        return out, ok

    def verify_each_t(self, msgs, msg_off, sigs, pks, strict=False):
        n = self._t(sigs, 64)
        assert self._t(pks, 32) == n and msg_off.numel() == n + 1
        status = self.torch.empty((n,), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        self._chk(self.lib.ed25519_verify_each_dev(self.ctx, msgs.data_ptr(), msg_off.data_ptr(), msgs.numel(), sigs.data_ptr(), pks.data_ptr(),
                                                   n, 1 if strict else 0, status.data_ptr()))
        return status

    def verify_each_prehashed_t(self, prehashes, sigs, pks, context=b"", strict=False):
        """Ed25519ph on device tensors (prehashes: n x 64 bytes).  -> status tensor, or PREHASHED_CONTEXT_LENGTH for a context beyond 255 bytes"""
        n = self._t(sigs, 64)
        assert self._t(pks, 32) == n and self._t(prehashes, 64) == n
        status = self.torch.empty((n,), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        st = self._chk(self.lib.ed25519_verify_each_prehashed_dev(self.ctx, prehashes.data_ptr(), bytes(context), len(context), sigs.data_ptr(), pks.data_ptr(),
                                                                  n, 1 if strict else 0, status.data_ptr()), (OK, PREHASHED_CONTEXT_LENGTH))
        return status if st == OK else st

    def sign_batch_prehashed_t(self, seeds, prehashes, context=b""):
        n = self._t(seeds, 32)
        assert self._t(prehashes, 64) == n
        pks = self.torch.empty((n, 32), dtype=self.torch.uint8, device=self.device)
        sigs = self.torch.empty((n, 64), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        st = self._chk(self.lib.ed25519_sign_batch_prehashed_dev(self.ctx, seeds.data_ptr(), prehashes.data_ptr(), bytes(context), len(context), n, pks.data_ptr(), sigs.data_ptr()),
                       (OK, PREHASHED_CONTEXT_LENGTH))
        return (pks, sigs) if st == OK else st

    def keygen_batch_t(self, seeds):
        n = self._t(seeds, 32)
        pks = self.torch.empty((n, 32), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        self._chk(self.lib.ed25519_keygen_batch_dev(self.ctx, seeds.data_ptr(), n, pks.data_ptr()))
        return pks

    def sign_batch_t(self, seeds, msgs, msg_off):
        n = self._t(seeds, 32)
        assert msg_off.numel() == n + 1
        pks = self.torch.empty((n, 32), dtype=self.torch.uint8, device=self.device)
        sigs = self.torch.empty((n, 64), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        self._chk(self.lib.ed25519_sign_batch_dev(self.ctx, seeds.data_ptr(), msgs.data_ptr(), msg_off.data_ptr(), msgs.numel(), n, pks.data_ptr(), sigs.data_ptr()))
        return pks, sigs

    # -- hash-to-group on device tensors: -> (n, 32) or (n, 160) uint8 tensor, or DOMAIN_SEPARATOR_LENGTH (an int) for a bad DST
    def _h2c_out_t(self, n, out_fmt):
        return self.torch.empty((n, _PT[out_fmt]), dtype=self.torch.uint8, device=self.device)

    def ristretto_from_uniform_bytes_batch_t(self, in64, out_fmt=FMT_RISTRETTO):
        n = self._t(in64, 64)
        out = self._h2c_out_t(n, out_fmt)
        self._bind_stream()
        self._chk(self.lib.c25519_ristretto_from_uniform_bytes_batch_dev(self.ctx, in64.data_ptr(), n, out_fmt, out.data_ptr()))
        return out

    def ristretto_map_to_curve_batch_t(self, in32, out_fmt=FMT_RISTRETTO):
        n = self._t(in32, 32)
        out = self._h2c_out_t(n, out_fmt)
        self._bind_stream()
        self._chk(self.lib.c25519_ristretto_map_to_curve_batch_dev(self.ctx, in32.data_ptr(), n, out_fmt, out.data_ptr()))
        return out

    def ristretto_hash_from_bytes_batch_t(self, msgs, msg_off, out_fmt=FMT_RISTRETTO):
        """msgs: uint8 CUDA tensor of the concatenated messages; msg_off: int64/uint64 CUDA tensor (n+1)"""
        n = msg_off.numel() - 1
        out = self._h2c_out_t(n, out_fmt)
        self._bind_stream()
        self._chk(self.lib.c25519_ristretto_hash_from_bytes_batch_dev(self.ctx, msgs.data_ptr(), msg_off.data_ptr(), msgs.numel(), n, out_fmt, out.data_ptr()))
        return out

    def edwards_hash_to_curve_batch_t(self, msgs, msg_off, dst, mode=H2C_RO, out_fmt=FMT_EDWARDS_Y):
        n = msg_off.numel() - 1
        out = self._h2c_out_t(n, out_fmt)
        self._bind_stream()
        dst = bytes(dst)
        st = self._chk(self.lib.c25519_edwards_hash_to_curve_batch_dev(self.ctx, msgs.data_ptr(), msg_off.data_ptr(), msgs.numel(), n, dst, len(dst), mode, out_fmt,
                                                                       out.data_ptr()), (OK, DOMAIN_SEPARATOR_LENGTH))
        return out if st == OK else st

    # -- Lizard on device tensors (D = Sha256) --------------------------------------------------------------------------
    def ristretto_lizard_encode_batch_t(self, data16, out_fmt=FMT_RISTRETTO):
        """(n, 16) uint8 payloads -> (n, 32) CompressedRistretto or (n, 160) RAW160 uint8 tensor"""
        n = self._t(data16, 16)
        out = self._h2c_out_t(n, out_fmt)
        self._bind_stream()
        self._chk(self.lib.c25519_ristretto_lizard_encode_sha256_batch_dev(self.ctx, data16.data_ptr(), n, out_fmt, out.data_ptr()))
        return out

    def ristretto_lizard_decode_batch_t(self, points, in_fmt=FMT_RISTRETTO):
        """-> (payloads (n, 16) uint8 tensor, zero unless OK; status (n,) uint8 tensor of LIZARD_*)"""
        n = self._t(points, _PT[in_fmt]) if in_fmt in (FMT_RISTRETTO, FMT_RAW160) else points.shape[0]
        out = self.torch.empty((n, 16), dtype=self.torch.uint8, device=self.device)
        st = self.torch.empty((n,), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        self._chk(self.lib.c25519_ristretto_lizard_decode_sha256_batch_dev(self.ctx, points.data_ptr(), n, in_fmt, out.data_ptr(), st.data_ptr()))
        return out, st

    def ristretto_map_to_curve_inverse_batch_t(self, points, in_fmt=FMT_RISTRETTO):
        """-> (preimages (n, 16, 32) uint8 tensor, an undefined slot zero; mask (n,) int16 tensor, bit j = slot j defined;
        ok (n,) uint8 tensor, 1 = valid encoding (all ones for RAW160 input))"""
        n = self._t(points, _PT[in_fmt]) if in_fmt in (FMT_RISTRETTO, FMT_RAW160) else points.shape[0]
        out = self.torch.empty((n, 16, 32), dtype=self.torch.uint8, device=self.device)
        mask = self.torch.empty((n,), dtype=self.torch.int16, device=self.device)
        ok = self.torch.ones((n,), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        self._chk(self.lib.c25519_ristretto_map_to_curve_inverse_batch_dev(self.ctx, points.data_ptr(), n, in_fmt, out.data_ptr(), mask.data_ptr(), ok.data_ptr()))
        return out, mask, ok

    # -- MontgomeryPoint on device tensors (montgomery.rs) ------------------------------------------------------------
    def montgomery_mul_batch_t(self, k, u, out=None):
        """u(k_i * P_i), the unclamped ladder over bits 254..0 of k_i (Mul<&Scalar>, montgomery.rs:484-492): (n, 32) uint8 tensors"""
        n = self._t(k, 32)
        assert self._t(u, 32) == n
        if out is None:
            out = self.torch.empty((n, 32), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        self._chk(self.lib.c25519_montgomery_mul_batch_dev(self.ctx, k.data_ptr(), u.data_ptr(), n, out.data_ptr()))
        return out

    def montgomery_mul_bits_be_batch_t(self, bits, nbits, u, out=None):
        """mul_bits_be (montgomery.rs:183-211): bits (n, ceil(nbits/8)) uint8 tensor, MSB first; u (n, 32) -> (n, 32)"""
        n = self._t(u, 32)
        nb = (nbits + 7) // 8
        if nb:
            assert bits.is_cuda and bits.dtype == self.torch.uint8 and bits.is_contiguous() and bits.numel() == n * nb
        if out is None:
            out = self.torch.empty((n, 32), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        self._chk(self.lib.c25519_montgomery_mul_bits_be_batch_dev(self.ctx, bits.data_ptr() if nb else None, nbits, u.data_ptr(), n, out.data_ptr()))
        return out

    def montgomery_mul_base_batch_t(self, scalars, out=None):
        """MontgomeryPoint::mul_base (montgomery.rs:144-146), unclamped: (n, 32) -> (n, 32)"""
        n = self._t(scalars, 32)
        if out is None:
            out = self.torch.empty((n, 32), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        self._chk(self.lib.c25519_montgomery_mul_base_batch_dev(self.ctx, scalars.data_ptr(), n, out.data_ptr()))
        return out

    def montgomery_to_edwards_batch_t(self, u, signs, out_fmt=FMT_EDWARDS_Y):
        """to_edwards(sign) (montgomery.rs:239-268): u (n, 32), signs (n,) uint8 -> (points (n, 32) or (n, 160), zero where None;
        status (n,) uint8, 1 = Some)"""
        n = self._t(u, 32)
        assert signs.is_cuda and signs.dtype == self.torch.uint8 and signs.is_contiguous() and signs.numel() == n
        out = self.torch.empty((n, _PT.get(out_fmt, 32)), dtype=self.torch.uint8, device=self.device)
        st = self.torch.empty((n,), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        self._chk(self.lib.c25519_montgomery_to_edwards_batch_dev(self.ctx, u.data_ptr(), signs.data_ptr(), n, out_fmt, out.data_ptr(), st.data_ptr()))
        return out, st

    # -- the group law on device tensors (edwards.rs / ristretto.rs Add, Sub, Neg, mul_by_cofactor, ConstantTimeEq, Sum) -----------
    # Each returns (status, result, ok): status OK, or NONE when a compressed input does not decode (ok[i] = 0 there).
    def point_add_batch_t(self, p, q, op=POINT_ADD, in_fmt=FMT_RAW160, out_fmt=FMT_RAW160):
        """p[i] + q[i] (op POINT_ADD) or p[i] - q[i] (POINT_SUB): (n, 32|160) uint8 tensors -> (status, (n, 32|160), ok (n,))"""
        n = self._t(p, _PT[in_fmt])
        assert self._t(q, _PT[in_fmt]) == n
        out = self.torch.empty((n, _PT.get(out_fmt, 32)), dtype=self.torch.uint8, device=self.device)
        ok = self.torch.empty((n,), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        st = self._chk(self.lib.c25519_point_add_batch_dev(self.ctx, p.data_ptr(), q.data_ptr(), n, op, in_fmt, out_fmt, out.data_ptr(), ok.data_ptr()), (OK, NONE))
        return st, out, ok

    def point_map_batch_t(self, p, op=POINT_NEG, in_fmt=FMT_RAW160, out_fmt=FMT_RAW160):
        """-p[i] (op POINT_NEG) or [8] p[i] (POINT_MUL_BY_COFACTOR, Edwards only) -> (status, (n, 32|160), ok (n,))"""
        n = self._t(p, _PT[in_fmt])
        out = self.torch.empty((n, _PT.get(out_fmt, 32)), dtype=self.torch.uint8, device=self.device)
        ok = self.torch.empty((n,), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        st = self._chk(self.lib.c25519_point_map_batch_dev(self.ctx, p.data_ptr(), n, op, in_fmt, out_fmt, out.data_ptr(), ok.data_ptr()), (OK, NONE))
        return st, out, ok

    def point_eq_batch_t(self, p, q=None, in_fmt=FMT_RAW160, group=FMT_EDWARDS_Y):
        """p[i] == q[i] in `group` (FMT_EDWARDS_Y or FMT_RISTRETTO), or p[i] == identity with q None -> (status, eq (n,), ok (n,))"""
        n = self._t(p, _PT[in_fmt])
        if q is not None:
            assert self._t(q, _PT[in_fmt]) == n
        eq = self.torch.empty((n,), dtype=self.torch.uint8, device=self.device)
        ok = self.torch.empty((n,), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        st = self._chk(self.lib.c25519_point_eq_batch_dev(self.ctx, p.data_ptr(), q.data_ptr() if q is not None else None, n, in_fmt, group,
                                                          eq.data_ptr(), ok.data_ptr()), (OK, NONE))
        return st, eq, ok

    def point_sum_segments_t(self, points, seg_off, in_fmt=FMT_RAW160, out_fmt=FMT_RAW160):
        """sums of points[seg_off[s] .. seg_off[s+1]): points (n, 32|160) uint8, seg_off (m + 1,) int64 CUDA tensor, trusted (monotone, 0 .. n;
        it stays on the device) -> (status, (m, 32|160), ok (m,))"""
        n = self._t(points, _PT[in_fmt])
        assert seg_off.is_cuda and seg_off.dtype in (self.torch.int64, self.torch.uint64) and seg_off.is_contiguous() and seg_off.numel() >= 1
        m = seg_off.numel() - 1
        out = self.torch.empty((m, _PT.get(out_fmt, 32)), dtype=self.torch.uint8, device=self.device)
        ok = self.torch.empty((m,), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        st = self._chk(self.lib.c25519_point_sum_segments_dev(self.ctx, points.data_ptr(), n, in_fmt, seg_off.data_ptr(), m, out_fmt,
                                                              out.data_ptr(), ok.data_ptr()), (OK, NONE))
        return st, out, ok

    def msm_vartime_segments_t(self, scalars, points, seg_off, in_fmt=FMT_RAW160, out_fmt=FMT_EDWARDS_Y):
        """many independent vartime MSMs: out[s] = sum scalars[i] * points[i] over [seg_off[s], seg_off[s+1]).  scalars (n, 32), points
        (n, 32|160) uint8 CUDA tensors; seg_off m + 1 offsets on the HOST (a sequence or a CPU tensor: the lengths are public and the host
        routes by them) -> (status OK | NONE, (m, 32|160), ok (m,))"""
        n = self._t(scalars, 32)
        assert self._t(points, _PT.get(in_fmt, 32)) == n
        if hasattr(seg_off, "is_cuda"):
            assert not seg_off.is_cuda, "seg_off stays on the host"
            seg_off = seg_off.numpy()
        off = np.ascontiguousarray(np.asarray(seg_off, dtype=np.uint64).reshape(-1))
        assert off.shape[0] >= 1
        m = off.shape[0] - 1
        out = self.torch.empty((m, _PT.get(out_fmt, 32)), dtype=self.torch.uint8, device=self.device)
        ok = self.torch.empty((m,), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        st = self._chk(self.lib.c25519_msm_vartime_segments_dev(self.ctx, scalars.data_ptr(), points.data_ptr(), n, in_fmt, off.ctypes.data, m, out_fmt,
                                                                out.data_ptr(), ok.data_ptr()), (OK, NONE))
        return st, out, ok

    def precomp_msm_vartime_rows_t(self, h, scalars, route=PRECOMP_ROWS_AUTO, out_fmt=FMT_EDWARDS_Y):
        """many multiscalar muls over one precomputation: out[r] = sum_j scalars[r][j] * S_j over the first w static points of the handle h.
        scalars (m, w, 32) uint8 CUDA tensor -> (m, 32|160) CUDA tensor, on torch's current stream (the call synchronises it once)"""
        assert scalars.dim() == 3 and scalars.shape[2] == 32, "scalars must have shape (m, w, 32)"
        m, w = int(scalars.shape[0]), int(scalars.shape[1])
        if scalars.numel():
            self._t(scalars, 32)
        out = self.torch.empty((m, _PT.get(out_fmt, 32)), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        self._chk(self.lib.c25519_precomp_msm_vartime_rows_dev(self.ctx, h, scalars.data_ptr(), m, w, route, out_fmt, out.data_ptr()))
        return out

    def precomp_msm_vartime_mixed_rows_t(self, h, static_scalars, dyn_scalars, dyn_points, dyn_off, in_fmt=FMT_RAW160, route=PRECOMP_ROWS_AUTO, out_fmt=FMT_EDWARDS_Y):
        """many mixed multiscalar muls over one precomputation: out[r] = sum_j static_scalars[r][j] * S_j + sum dyn_scalars[i] * dyn_points[i] over
        i in [dyn_off[r], dyn_off[r+1]).  static_scalars (m, w, 32), dyn_scalars (n_dyn, 32), dyn_points (n_dyn, 32|160) uint8 CUDA tensors; dyn_off
        m + 1 offsets on the HOST (a sequence or a CPU tensor: the lengths are public and the host cuts the passes by them) -> (status OK | NONE,
        (m, 32|160), ok (m,)), on torch's current stream (the call synchronises it once)"""
        assert static_scalars.dim() == 3 and static_scalars.shape[2] == 32, "static_scalars must have shape (m, w, 32)"
        m, w = int(static_scalars.shape[0]), int(static_scalars.shape[1])
        if static_scalars.numel():
            self._t(static_scalars, 32)
        n = self._t(dyn_scalars, 32)
        assert self._t(dyn_points, _PT.get(in_fmt, 32)) == n
        if hasattr(dyn_off, "is_cuda"):
            assert not dyn_off.is_cuda, "dyn_off stays on the host"
            dyn_off = dyn_off.numpy()
        off = np.ascontiguousarray(np.asarray(dyn_off, dtype=np.uint64).reshape(-1))
        assert off.shape[0] == m + 1, "dyn_off must hold m + 1 offsets"
        out = self.torch.empty((m, _PT.get(out_fmt, 32)), dtype=self.torch.uint8, device=self.device)
        ok = self.torch.empty((m,), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        st = self._chk(self.lib.c25519_precomp_msm_vartime_mixed_rows_dev(self.ctx, h, static_scalars.data_ptr(), m, w, dyn_scalars.data_ptr(), dyn_points.data_ptr(), n,
                                                                          in_fmt, off.ctypes.data, route, out_fmt, out.data_ptr(), ok.data_ptr()), (OK, NONE))
        return st, out, ok

    def precomp_msm_vartime_mixed_rows_fold_t(self, h, static_scalars, dyn_scalars, dyn_points, dyn_off, weights, in_fmt=FMT_RAW160, out_fmt=FMT_EDWARDS_Y):
        """precomp_msm_vartime_mixed_rows_fold on device inputs: static_scalars (m, w, 32), dyn_scalars (n_dyn, 32), dyn_points (n_dyn, 32|160),
        weights (m, 16) or (m, 32) uint8 CUDA tensors; dyn_off m + 1 offsets on the HOST (a sequence or a CPU tensor); h may be None iff w == 0
        -> (status OK | NONE, 32|160 bytes on the host), on torch's current stream (the call synchronises it)"""
        assert static_scalars.dim() == 3 and static_scalars.shape[2] == 32, "static_scalars must have shape (m, w, 32)"
        m, w = int(static_scalars.shape[0]), int(static_scalars.shape[1])
        if static_scalars.numel():
            self._t(static_scalars, 32)
        n = self._t(dyn_scalars, 32)
        assert self._t(dyn_points, _PT.get(in_fmt, 32)) == n
        assert weights.dim() == 2 and int(weights.shape[0]) == m, "weights must have shape (m, 16) or (m, 32)"
        wb = int(weights.shape[1])
        if weights.numel():
            self._t(weights, wb)
        off = _seg_off_host(dyn_off)
        assert off.shape[0] == m + 1, "dyn_off must hold m + 1 offsets"
        out = C.create_string_buffer(_PT.get(out_fmt, 32))
        self._bind_stream()
        st = self._chk(self.lib.c25519_precomp_msm_vartime_mixed_rows_fold_dev(self.ctx, h, static_scalars.data_ptr(), m, w, dyn_scalars.data_ptr(), dyn_points.data_ptr(), n,
                                                                               in_fmt, off.ctypes.data, weights.data_ptr(), wb, out_fmt, out), (OK, NONE))
        return st, out.raw

    def verify_batch_segments_t(self, msgs, msg_off, sigs, pks, seg_off, z_mode=Z_TRANSCRIPT, pk_points=None):
        """many independent verify_batch calls in one: status[s] is what verify_batch_t returns for signatures [seg_off[s], seg_off[s+1]) alone.
        msgs, msg_off, sigs, pks, pk_points as for verify_batch_t (CUDA tensors); seg_off m + 1 offsets on the HOST -> (m,) uint8 CUDA tensor"""
        n = self._t(sigs, 64)
        assert self._t(pks, 32) == n and msg_off.numel() == n + 1
        if pk_points is not None:
            assert self._t(pk_points, 160) == n
        off = _seg_off_host(seg_off)
        m = off.shape[0] - 1
        status = self.torch.empty((m,), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        self._chk(self.lib.ed25519_verify_batch_segments_dev(self.ctx, msgs.data_ptr(), msg_off.data_ptr(), msgs.numel(), sigs.data_ptr(), pks.data_ptr(),
                                                             pk_points.data_ptr() if pk_points is not None else None, n, off.ctypes.data, m, z_mode,
                                                             status.data_ptr()))
        return status

    def batch_transcript_zs_segments_t(self, hram, sigs, seg_off, out=None):
        """the reference's z_i (batch.rs:168-222) of many independent batches, one Merlin transcript per segment on the GPU: rows [seg_off[s],
        seg_off[s+1]) are batch_transcript_zs of that segment alone.  hram: n x 64 bytes (the tensor of batch_hram_t with its trailer will do),
        sigs (n, 64): uint8 CUDA tensors; seg_off m + 1 offsets on the HOST; out: an (n, 16) uint8 CUDA tensor to write into (rows of no segment
        stay as they are).  -> (n, 16) uint8 CUDA tensor.  Enqueue only; every segment runs on the device whatever its length."""
        n = self._t(sigs, 64)
        assert hram.is_cuda and hram.dtype == self.torch.uint8 and hram.is_contiguous() and hram.numel() in (n * 64, n * 64 + 64)
        assert n == 0 or hram.data_ptr() % 16 == 0, "device buffers must be 16-byte aligned"
        off = _seg_off_host(seg_off)
        m = off.shape[0] - 1
        if out is None:
            out = self.torch.empty((n, 16), dtype=self.torch.uint8, device=self.device)
        assert self._t(out, 16) == n
        self._bind_stream()
        self._chk(self.lib.ed25519_batch_transcript_zs_segments_dev(self.ctx, hram.data_ptr(), sigs.data_ptr(), n, off.ctypes.data, m, out.data_ptr()))
        return out

    # -- host-buffer API (numpy in / numpy out) ---------------------------------------------------
    @staticmethod
    def _out(out, n, width):
        """the caller's output buffer (reuse it: a fresh allocation pays first-touch page faults inside the copy) or a new one"""
        if out is None:
            return np.empty((n, width) if width > 1 else (n,), dtype=np.uint8)
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.size == n * width
        return out

    def mul_base_batch(self, scalars, out_fmt=FMT_EDWARDS_Y, out=None):
        s = _np8(scalars, 32); n = s.shape[0]
        out = self._out(out, n, _PT[out_fmt])
        self._bind_stream()
        self._chk(self.lib.c25519_mul_base_batch(self.ctx, s.ctypes.data, n, out_fmt, out.ctypes.data))
        return out

    def mul_base_clamped_batch(self, raw, out_fmt=FMT_EDWARDS_Y, out=None):
        """EdwardsPoint::mul_base_clamped (edwards.rs:948): clamp_integer(raw_i) * B, not reduced mod l"""
        s = _np8(raw, 32); n = s.shape[0]
        out = self._out(out, n, _PT[out_fmt])
        self._bind_stream()
        self._chk(self.lib.c25519_mul_base_clamped_batch(self.ctx, s.ctypes.data, n, out_fmt, out.ctypes.data))
        return out

    def mul_clamped_batch(self, raw, points, in_fmt=FMT_RAW160, out_fmt=FMT_EDWARDS_Y):
        """EdwardsPoint::mul_clamped (edwards.rs:932): clamp_integer(raw_i) * P_i"""
        s = _np8(raw, 32); p = _np8(points, _PT[in_fmt]); n = s.shape[0]
        assert p.shape[0] == n
        out = np.empty((n, _PT[out_fmt]), dtype=np.uint8); ok = np.empty((n,), dtype=np.uint8)
        self._bind_stream()
        self._chk(self.lib.c25519_mul_clamped_batch(self.ctx, s.ctypes.data, p.ctypes.data, n, in_fmt, out_fmt, out.ctypes.data, ok.ctypes.data))
        return out, ok

    def point_order_checks(self, points, in_fmt=FMT_EDWARDS_Y, which=POINT_SMALL_ORDER | POINT_TORSION_FREE):
        """EdwardsPoint::is_small_order / is_torsion_free (edwards.rs:1405 / :1435) -> (n,) uint8 flags: POINT_DECODES | POINT_SMALL_ORDER | POINT_TORSION_FREE"""
        p = _np8(points, _PT[in_fmt]); n = p.shape[0]
        fl = np.empty((n,), dtype=np.uint8)
        self._bind_stream()
        self._chk(self.lib.c25519_point_order_checks_batch(self.ctx, p.ctypes.data, n, in_fmt, which, fl.ctypes.data))
        return fl

    def point_order_checks_t(self, points, in_fmt=FMT_EDWARDS_Y, which=POINT_SMALL_ORDER | POINT_TORSION_FREE):
        n = self._t(points, _PT[in_fmt])
        fl = self.torch.empty((n,), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        self._chk(self.lib.c25519_point_order_checks_batch_dev(self.ctx, points.data_ptr(), n, in_fmt, which, fl.data_ptr()))
        return fl

    # -- constant-time fixed-base tables for a caller's point (EdwardsBasepointTable::create / RistrettoBasepointTable::create)
    def basetable_create(self, point, in_fmt=FMT_EDWARDS_Y):
        b = bytes(point)
        assert len(b) == _PT[in_fmt]
        self._bind_stream()
        h = self.lib.c25519_basetable_create(self.ctx, b, in_fmt)
        if not h:
            raise EngineError("basetable_create failed: %s" % self.lib.c25519_last_error(self.ctx).decode())
        return h

    def basetable_destroy(self, h):
        self.lib.c25519_basetable_destroy(self.ctx, h)

    def mul_table_batch(self, h, scalars, out_fmt=FMT_EDWARDS_Y, out=None):
        s = _np8(scalars, 32); n = s.shape[0]
        out = self._out(out, n, _PT[out_fmt])
        self._bind_stream()
        self._chk(self.lib.c25519_mul_table_batch(self.ctx, h, s.ctypes.data, n, out_fmt, out.ctypes.data))
        return out

    def mul_table_batch_t(self, h, scalars, out_fmt=FMT_EDWARDS_Y, out=None):
        n = self._t(scalars, 32)
        if out is None:
            out = self.torch.empty((n, _PT[out_fmt]), dtype=self.torch.uint8, device=self.device)
        self._bind_stream()
        self._chk(self.lib.c25519_mul_table_batch_dev(self.ctx, h, scalars.data_ptr(), n, out_fmt, out.data_ptr()))
        return out

    def last_ffi(self):
        """-> (wall-clock ms, bytes up, bytes down) of the latest host-pointer call"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        ms = float(self.lib.c25519_last_ffi_ms(self.ctx, C.byref(a), C.byref(b)))
        return ms, int(a.value), int(b.value)

    def trim(self):
        self._chk(self.lib.c25519_ctx_trim(self.ctx))

    def x25519_base_batch(self, k, out=None):
        """X25519 public keys x25519(k_i, 9) through the fixed-base path (x25519.rs:105-109)."""
        k = _np8(k, 32); n = k.shape[0]
        out = self._out(out, n, 32)
        self._bind_stream()
        self._chk(self.lib.c25519_x25519_base_batch(self.ctx, k.ctypes.data, n, out.ctypes.data))
        return out

    def x25519_batch(self, k, u, out=None):
        k = _np8(k, 32); u = _np8(u, 32); n = k.shape[0]
        assert u.shape[0] == n
        out = self._out(out, n, 32)
        self._bind_stream()
        self._chk(self.lib.c25519_x25519_batch(self.ctx, k.ctypes.data, u.ctypes.data, n, out.ctypes.data))
        return out

    def x25519_contributory_batch(self, k, u):
        """-> (shared secrets (n, 32), was_contributory (n,)): x25519.rs:335 as a batched flag"""
        k = _np8(k, 32); u = _np8(u, 32); n = k.shape[0]
        assert u.shape[0] == n
        out = np.empty((n, 32), dtype=np.uint8); fl = np.empty((n,), dtype=np.uint8)
        self._bind_stream()
        self._chk(self.lib.c25519_x25519_contributory_batch(self.ctx, k.ctypes.data, u.ctypes.data, n, out.ctypes.data, fl.ctypes.data))
        return out, fl

    def decompress_batch(self, enc, in_fmt=FMT_EDWARDS_Y):
        e = _np8(enc, 32); n = e.shape[0]
        pts = np.empty((n, 160), dtype=np.uint8); ok = np.empty((n,), dtype=np.uint8)
        self._bind_stream()
        st = self._chk(self.lib.c25519_decompress_batch(self.ctx, e.ctypes.data, n, in_fmt, pts.ctypes.data, ok.ctypes.data), (OK, NONE))
        return st, pts, ok

    def compress_batch(self, pts, out_fmt=FMT_EDWARDS_Y):
        p = _np8(pts, 160); n = p.shape[0]
        out = np.empty((n, 32), dtype=np.uint8)
        self._bind_stream()
        self._chk(self.lib.c25519_compress_batch(self.ctx, p.ctypes.data, n, out_fmt, out.ctypes.data))
        return out

    def msm_vartime(self, scalars, points, in_fmt=FMT_RAW160, out_fmt=FMT_EDWARDS_Y):
        s = _np8(scalars, 32); p = _np8(points, _PT[in_fmt]); n = s.shape[0]
        assert p.shape[0] == n
        out = C.create_string_buffer(_PT[out_fmt])
        self._bind_stream()
        st = self._chk(self.lib.c25519_msm_vartime(self.ctx, s.ctypes.data, p.ctypes.data, n, in_fmt, out_fmt, out), (OK, NONE))
        return st, out.raw

    def verify_batch(self, msgs, sigs, pks, z_mode=Z_TRANSCRIPT, pk_points=None):
        """msgs: list of bytes; sigs: list of 64-byte; pks: list of 32-byte; pk_points: optional (n, 160) uint8
        array of the keys' decompressed points (VerifyingKey.point).  Status code out."""
        if not (len(msgs) == len(sigs) == len(pks)):
            return ARRAY_LENGTH  # batch.rs:152-165
        n = len(msgs)
        self._check_items(sigs, 64, "signature"); self._check_items(pks, 32, "public key")
        off = np.zeros(n + 1, dtype=np.uint64)
        for i, m in enumerate(msgs):
            off[i + 1] = off[i] + len(m)
        blob = np.frombuffer(b"".join(msgs) + b"\0" * 16, dtype=np.uint8)
        s = _np8(b"".join(sigs) if n else b"", 64) if n else np.zeros((0, 64), np.uint8)
        p = _np8(b"".join(pks) if n else b"", 32) if n else np.zeros((0, 32), np.uint8)
        self._bind_stream()
        pp = None
        if pk_points is not None:
            pp = _np8(pk_points, 160)
            assert pp.shape[0] == n
        return self._chk(self.lib.ed25519_verify_batch_keys(self.ctx, blob.ctypes.data, off.ctypes.data, s.ctypes.data, p.ctypes.data,
                                                            pp.ctypes.data if pp is not None else None, n, z_mode),
                         (OK, NONE, SCALAR_FORMAT, VERIFY))

    def verify_batch_segments(self, msgs, sigs, pks, seg_off, z_mode=Z_TRANSCRIPT, pk_points=None):
        """many independent batches in one call.  msgs / sigs / pks: lists over ALL signatures; seg_off: m + 1 offsets into them; pk_points:
        optional (n, 160) uint8 array of the keys' decompressed points.  -> numpy uint8 status per segment, each what verify_batch returns
        for that segment alone (0 OK, 1 bad key, 2 ScalarFormat, 3 Verify; an empty segment is 0)."""
        n = len(msgs)
        assert len(sigs) == n and len(pks) == n
        self._check_items(sigs, 64, "signature"); self._check_items(pks, 32, "public key")
        off = _seg_off_host(seg_off)
        m = off.shape[0] - 1
        status = np.zeros((m,), dtype=np.uint8)
        blob, moff = self._pack(list(msgs))
        s = _np8(b"".join(sigs), 64) if n else np.zeros((0, 64), np.uint8)
        p = _np8(b"".join(pks), 32) if n else np.zeros((0, 32), np.uint8)
        pp = None
        if pk_points is not None:
            pp = _np8(pk_points, 160)
            assert pp.shape[0] == n
        self._bind_stream()
        self._chk(self.lib.ed25519_verify_batch_segments(self.ctx, blob.ctypes.data, moff.ctypes.data, s.ctypes.data, p.ctypes.data,
                                                         pp.ctypes.data if pp is not None else None, n, off.ctypes.data, m, z_mode, status.ctypes.data))
        return status

    @staticmethod
    def verify_batch_segments_plan(seg_off):
        """how verify_batch_segments routes these m + 1 offsets -> (segments on the segmented route, segments run as single batches, passes,
        most terms in one pass).  Host arithmetic: no engine, no GPU."""
        off = _seg_off_host(seg_off)
        plan = np.zeros(4, dtype=np.uint64)
        st = load_library().ed25519_verify_batch_segments_plan(off.ctypes.data, off.shape[0] - 1, plan.ctypes.data)
        if st:
            raise EngineError("HIP error %d: verify_batch_segments_plan: seg_off must be m + 1 non-decreasing values from 0, below 2^40" % -st)
        return tuple(int(v) for v in plan)

    def batch_transcript_zs_segments(self, hram, sigs, seg_off, out=None):
        """batch_transcript_zs of many independent batches on the GPU: hram (n, 64), sigs (n, 64) uint8 arrays or bytes, seg_off m + 1 offsets
        -> (n, 16) uint8 array (`out`, when given, is written in place: rows of no segment stay as they are)"""
        h = _np8(hram, 64); g = _np8(sigs, 64); n = h.shape[0]
        assert g.shape[0] == n
        off = _seg_off_host(seg_off)
        z = np.zeros((n, 16), dtype=np.uint8) if out is None else out
        assert z.dtype == np.uint8 and z.flags["C_CONTIGUOUS"] and z.shape == (n, 16)
        self._bind_stream()
        self._chk(self.lib.ed25519_batch_transcript_zs_segments(self.ctx, h.ctypes.data, g.ctypes.data, n, off.ctypes.data, off.shape[0] - 1, z.ctypes.data))
        return z

    @staticmethod
    def batch_transcript_zs_segments_plan(seg_off):
        """how verify_batch_segments routes the transcripts of these m + 1 offsets in Z_TRANSCRIPT -> (segments whose transcript runs on the device:
        at most TRANSCRIPT_SEGMENT_DEVICE_MAX signatures; segments whose transcript runs on the host: longer, up to VERIFY_SEGMENT_MAX).  Host
        arithmetic: no engine, no GPU."""
        off = _seg_off_host(seg_off)
        plan = np.zeros(2, dtype=np.uint64)
        st = load_library().ed25519_batch_transcript_zs_segments_plan(off.ctypes.data, off.shape[0] - 1, plan.ctypes.data)
        if st:
            raise EngineError("HIP error %d: batch_transcript_zs_segments_plan: seg_off must be m + 1 non-decreasing values from 0, below 2^40" % -st)
        return tuple(int(v) for v in plan)

    def debug_batch_zs(self, msgs, sigs, pks, z_mode=Z_DEVICE):
        """The z_i of a batch as an (n, 16) uint8 array (diagnostics, see c25519_debug_batch_zs)."""
        n = len(msgs)
        assert len(sigs) == n and len(pks) == n
        self._check_items(sigs, 64, "signature"); self._check_items(pks, 32, "public key")
        out = np.zeros((n, 16), dtype=np.uint8)
        if n == 0:
            return out
        blob, off = self._pack(list(msgs))
        s = _np8(b"".join(sigs), 64); p = _np8(b"".join(pks), 32)
        self._bind_stream()
        self._chk(self.lib.c25519_debug_batch_zs(self.ctx, blob.ctypes.data, off.ctypes.data, s.ctypes.data, p.ctypes.data, n, z_mode, out.ctypes.data))
        return out

    def mul_batch(self, scalars, points, in_fmt=FMT_RAW160, out_fmt=FMT_EDWARDS_Y):
        s = _np8(scalars, 32); p = _np8(points, _PT[in_fmt]); n = s.shape[0]
        assert p.shape[0] == n
        out = np.empty((n, _PT[out_fmt]), dtype=np.uint8); ok = np.empty((n,), dtype=np.uint8)
        self._bind_stream()
        self._chk(self.lib.c25519_mul_batch(self.ctx, s.ctypes.data, p.ctypes.data, n, in_fmt, out_fmt, out.ctypes.data, ok.ctypes.data))
        return out, ok

    def double_base_batch(self, a, A, b, in_fmt=FMT_RAW160, out_fmt=FMT_EDWARDS_Y):
        """out[i] = a[i]*A[i] + b[i]*B (vartime_double_scalar_mul_basepoint, edwards.rs:1099)."""
        sa = _np8(a, 32); p = _np8(A, _PT[in_fmt]); sb = _np8(b, 32); n = sa.shape[0]
        assert p.shape[0] == n and sb.shape[0] == n
        out = np.empty((n, _PT[out_fmt]), dtype=np.uint8); ok = np.empty((n,), dtype=np.uint8)
        self._bind_stream()
        self._chk(self.lib.c25519_double_base_batch(self.ctx, sa.ctypes.data, p.ctypes.data, sb.ctypes.data, n, in_fmt, out_fmt, out.ctypes.data, ok.ctypes.data))
        return out, ok

    @staticmethod
    def _check_items(items, width, what):
        for i, it in enumerate(items):
            if len(it) != width:
                raise ValueError("%s %d has %d bytes, expected %d" % (what, i, len(it), width))

    @staticmethod
    def _pack(msgs):
        n = len(msgs)
        off = np.zeros(n + 1, dtype=np.uint64)
        for i, m in enumerate(msgs):
            off[i + 1] = off[i] + len(m)
        return np.frombuffer(b"".join(msgs) + b"\0" * 16, dtype=np.uint8), off

    def verify_each(self, msgs, sigs, pks, strict=False):
        """-> numpy uint8 status per signature (0 OK, 1 bad key, 2 ScalarFormat, 3 Verify)."""
        n = len(msgs)
        assert len(sigs) == n and len(pks) == n
        status = np.empty((n,), dtype=np.uint8)
        if n == 0:
            return status
        self._check_items(sigs, 64, "signature"); self._check_items(pks, 32, "public key")
        blob, off = self._pack(list(msgs))
        s = _np8(b"".join(sigs), 64); p = _np8(b"".join(pks), 32)
        self._bind_stream()
        self._chk(self.lib.ed25519_verify_each(self.ctx, blob.ctypes.data, off.ctypes.data, s.ctypes.data, p.ctypes.data, n, 1 if strict else 0, status.ctypes.data))
        return status

    def verify_each_prehashed(self, prehashes, sigs, pks, context=b"", strict=False):
        """Ed25519ph / Ed25519ctx per signature (verifying.rs:284 / :424): prehashes = the 64-byte SHA-512 of each message.
        -> numpy uint8 status per signature, or PREHASHED_CONTEXT_LENGTH (an int) when the context exceeds 255 bytes."""
        n = len(prehashes)
        assert len(sigs) == n and len(pks) == n
        status = np.empty((n,), dtype=np.uint8)
        self._check_items(sigs, 64, "signature"); self._check_items(pks, 32, "public key"); self._check_items(prehashes, 64, "prehash")
        ph = _np8(b"".join(prehashes), 64) if n else np.empty((0, 64), np.uint8)
        s = _np8(b"".join(sigs), 64) if n else np.empty((0, 64), np.uint8); p = _np8(b"".join(pks), 32) if n else np.empty((0, 32), np.uint8)
        self._bind_stream()
        st = self._chk(self.lib.ed25519_verify_each_prehashed(self.ctx, ph.ctypes.data, bytes(context), len(context), s.ctypes.data, p.ctypes.data, n, 1 if strict else 0,
                                                              status.ctypes.data), (OK, PREHASHED_CONTEXT_LENGTH))
        return status if st == OK else st

    def sign_batch_prehashed(self, seeds, prehashes, context=b""):
        """Ed25519ph signing (signing.rs:312): -> (pks, sigs) numpy arrays, or PREHASHED_CONTEXT_LENGTH (an int)."""
        n = len(seeds)
        assert len(prehashes) == n
        pks = np.empty((n, 32), dtype=np.uint8); sigs = np.empty((n, 64), dtype=np.uint8)
        self._check_items(seeds, 32, "seed"); self._check_items(prehashes, 64, "prehash")
        sd = _np8(b"".join(seeds), 32) if n else np.empty((0, 32), np.uint8); ph = _np8(b"".join(prehashes), 64) if n else np.empty((0, 64), np.uint8)
        self._bind_stream()
        st = self._chk(self.lib.ed25519_sign_batch_prehashed(self.ctx, sd.ctypes.data, ph.ctypes.data, bytes(context), len(context), n, pks.ctypes.data, sigs.ctypes.data),
                       (OK, PREHASHED_CONTEXT_LENGTH))
        return (pks, sigs) if st == OK else st

    def sign_batch(self, seeds, msgs):
        """-> (pks (n,32), sigs (n,64)) numpy arrays; seeds: list of 32-byte secret keys."""
        n = len(seeds)
        assert len(msgs) == n
        pks = np.empty((n, 32), dtype=np.uint8); sigs = np.empty((n, 64), dtype=np.uint8)
        if n == 0:
            return pks, sigs
        self._check_items(seeds, 32, "seed")
        blob, off = self._pack(list(msgs))
        sd = _np8(b"".join(seeds), 32)
        self._bind_stream()
        self._chk(self.lib.ed25519_sign_batch(self.ctx, sd.ctypes.data, blob.ctypes.data, off.ctypes.data, n, pks.ctypes.data, sigs.ctypes.data))
        return pks, sigs

    def to_montgomery_batch(self, pts):
        p = _np8(pts, 160); n = p.shape[0]
        out = np.empty((n, 32), dtype=np.uint8)
        self._bind_stream()
        self._chk(self.lib.c25519_to_montgomery_batch(self.ctx, p.ctypes.data, n, out.ctypes.data))
        return out

    # -- §8f widening ------------------------------------------------------------------------------------
    def precomp_create(self, static_points, in_fmt=FMT_RAW160):
        p = _np8(static_points, _PT[in_fmt])
        self._bind_stream()
        h = self.lib.c25519_precomp_create(self.ctx, p.ctypes.data, p.shape[0], in_fmt)
        if not h:
            raise EngineError("precomp_create failed: %s" % self.lib.c25519_last_error(self.ctx).decode())
        return h

    def precomp_destroy(self, h):
        self.lib.c25519_precomp_destroy(self.ctx, h)

    def precomp_len(self, h):
        return int(self.lib.c25519_precomp_len(h))

    def precomp_msm_vartime(self, h, static_scalars, dyn_scalars, dyn_points, in_fmt=FMT_RAW160, out_fmt=FMT_EDWARDS_Y):
        ss = _np8(static_scalars, 32); ds = _np8(dyn_scalars, 32); dp = _np8(dyn_points, _PT[in_fmt])
        assert ds.shape[0] == dp.shape[0]
        out = C.create_string_buffer(_PT[out_fmt])
        self._bind_stream()
        st = self._chk(self.lib.c25519_precomp_msm_vartime(self.ctx, h, ss.ctypes.data, ss.shape[0], ds.ctypes.data, dp.ctypes.data, ds.shape[0],
                                                           in_fmt, out_fmt, out), (OK, NONE))
        return st, out.raw

    def precomp_msm_vartime_rows(self, h, scalars, route=PRECOMP_ROWS_AUTO, out_fmt=FMT_EDWARDS_Y):
        """many multiscalar muls over one precomputation in one call (VartimePrecomputedMultiscalarMul::vartime_multiscalar_mul per row,
        traits.rs:304-419): out[r] = sum_j scalars[r][j] * S_j over the first w static points of the handle h.  scalars (m, w, 32) uint8 ->
        (m, 32|160); every row in format 0 or 1 is byte for byte what precomp_msm_vartime returns for it alone.  route: PRECOMP_ROWS_AUTO
        (precomp_msm_vartime_rows_plan tells which), or PRECOMP_ROWS_LANE / PRECOMP_ROWS_WAVE to force one.  The first call on a handle
        builds its comb table (precomp_rows_table_bytes)."""
        s = np.ascontiguousarray(scalars, dtype=np.uint8)
        assert s.ndim == 3 and s.shape[2] == 32, "scalars must have shape (m, w, 32)"
        m, w = s.shape[0], s.shape[1]
        out = np.empty((m, _PT.get(out_fmt, 32)), np.uint8)
        self._bind_stream()
        self._chk(self.lib.c25519_precomp_msm_vartime_rows(self.ctx, h, s.ctypes.data, m, w, route, out_fmt, out.ctypes.data))
        return out

    @staticmethod
    def precomp_msm_vartime_rows_plan(m, w):
        """how PRECOMP_ROWS_AUTO routes m rows of w terms -> (route, waves launched): the lane route iff w < PRECOMP_ROWS_LANE_WIDTH and
        m >= PRECOMP_ROWS_LANE_MIN_ROWS.  Host arithmetic: needs no GPU and no context (a static method); a shape the call would reject raises."""
        plan = np.zeros(2, np.uint64)
        st = load_library().c25519_precomp_msm_vartime_rows_plan(m, w, plan.ctypes.data)
        if st < 0:
            raise EngineError("HIP error %d: precomp_msm_vartime_rows_plan: m must be below 2^32 - 1 and m * w must not overflow" % -st)
        return int(plan[0]), int(plan[1])

    def precomp_rows_table_bytes(self, h):
        """bytes of the handle's comb table: 0 until the first precomp_msm_vartime_rows call has built it, 65536 per static point afterwards"""
        return int(self.lib.c25519_precomp_rows_table_bytes(h))

    def precomp_msm_vartime_mixed_rows(self, h, static_scalars, dyn_scalars, dyn_points, dyn_off, in_fmt=FMT_RAW160, route=PRECOMP_ROWS_AUTO, out_fmt=FMT_EDWARDS_Y):
        """many mixed multiscalar muls over one precomputation in one call (VartimePrecomputedMultiscalarMul::vartime_mixed_multiscalar_mul per
        row, traits.rs:304-419, precomputed_straus.rs:29-127): out[r] = sum_j static_scalars[r][j] * S_j over the first w static points of the
        handle h + sum dyn_scalars[i] * dyn_points[i] over i in [dyn_off[r], dyn_off[r+1]).  static_scalars (m, w, 32), dyn_scalars (n_dyn, 32),
        dyn_points (n_dyn, 32|160) uint8, dyn_off m + 1 offsets -> (status OK | NONE, (m, 32|160), ok (m,)); ok[r] = 0 where a dynamic point of
        row r does not decode.  Every row with ok = 1 in format 0 or 1 is byte for byte what precomp_msm_vartime returns for it alone; a row
        may have at most MSM_SEGMENT_WAVE_MAX dynamic terms.  route: PRECOMP_ROWS_AUTO (precomp_msm_vartime_mixed_rows_plan tells which),
        or PRECOMP_ROWS_LANE / PRECOMP_ROWS_WAVE to force one.  The comb table is the rows call's (precomp_rows_table_bytes)."""
        ss = np.ascontiguousarray(static_scalars, dtype=np.uint8)
        assert ss.ndim == 3 and ss.shape[2] == 32, "static_scalars must have shape (m, w, 32)"
        m, w = ss.shape[0], ss.shape[1]
        ds = _np8(dyn_scalars, 32) if len(dyn_scalars) else np.zeros((0, 32), np.uint8)
        dp = _np8(dyn_points, _PT.get(in_fmt, 32)) if len(dyn_points) else np.zeros((0, _PT.get(in_fmt, 32)), np.uint8)
        assert ds.shape[0] == dp.shape[0]
        off = np.ascontiguousarray(np.asarray(dyn_off, dtype=np.uint64).reshape(-1))
        assert off.shape[0] == m + 1, "dyn_off must hold m + 1 offsets"
        out = np.empty((m, _PT.get(out_fmt, 32)), np.uint8); ok = np.empty((m,), np.uint8)
        self._bind_stream()
        st = self._chk(self.lib.c25519_precomp_msm_vartime_mixed_rows(self.ctx, h, ss.ctypes.data, m, w, ds.ctypes.data, dp.ctypes.data, ds.shape[0], in_fmt,
                                                                      off.ctypes.data, route, out_fmt, out.ctypes.data, ok.ctypes.data), (OK, NONE))
        return st, out, ok

    @staticmethod
    def precomp_msm_vartime_mixed_rows_plan(m, w, dyn_off):
        """how precomp_msm_vartime_mixed_rows treats m rows of w static scalars with these m + 1 dynamic offsets -> (the route PRECOMP_ROWS_AUTO
        takes, waves of its row launches, passes, most dynamic terms in one pass): for w < PRECOMP_ROWS_LANE_WIDTH the lane route iff no row has more
        than PRECOMP_MIXED_LANE_DYN_MAX dynamic terms and m >= PRECOMP_MIXED_LANE_BASE_ROWS + PRECOMP_MIXED_LANE_ROWS_PER_TERM * (w + the longest
        row's dynamic terms) -- without any dynamic term the rule of precomp_msm_vartime_rows_plan; a pass holds at most MSM_SEGMENT_PASS_TERMS
        dynamic terms.  Host arithmetic: needs no GPU and no context (a static method); a shape the call would
        reject raises."""
        off = np.ascontiguousarray(np.asarray(dyn_off, dtype=np.uint64).reshape(-1))
        assert m == 0 or off.shape[0] == m + 1, "dyn_off must hold m + 1 offsets"
        plan = np.zeros(4, np.uint64)
        st = load_library().c25519_precomp_msm_vartime_mixed_rows_plan(m, w, off.ctypes.data if off.size else None, plan.ctypes.data)
        if st < 0:
            raise EngineError("HIP error %d: precomp_msm_vartime_mixed_rows_plan: m must be below 2^32 - 1, m * w must not overflow, dyn_off must be m + 1 "
                              "non-decreasing values from 0, below 2^40, and no row may have more than MSM_SEGMENT_WAVE_MAX dynamic terms" % -st)
        return tuple(int(x) for x in plan)

    def precomp_msm_vartime_mixed_rows_fold(self, h, static_scalars, dyn_scalars, dyn_points, dyn_off, weights, in_fmt=FMT_RAW160, out_fmt=FMT_EDWARDS_Y):
        """the rows of precomp_msm_vartime_mixed_rows folded into ONE multiscalar mul by a random linear combination (the fold of
        ed25519-dalek/src/batch.rs:207-233 for the equations of vartime_mixed_multiscalar_mul): with a weight c_r per row, on integers mod l,
        t_j = sum_r c_r * static_scalars[r][j], d'_i = c_row(i) * dyn_scalars[i], out = sum_j t_j * S_j + sum_i d'_i * dyn_points[i].
        static_scalars (m, w, 32), dyn_scalars (n_dyn, 32), dyn_points (n_dyn, 32|160) uint8, dyn_off m + 1 offsets, weights (m, 16) or (m, 32)
        uint8 -> (status OK | NONE, 32|160 bytes).  Scalars and weights are any little-endian integers (reduced by the product: no bit-255
        refusal); a row may have any number of dynamic terms; h may be None iff w == 0.  The result in format 0 or 1 is byte for byte
        precomp_msm_vartime(h, t, d', dyn_points); exact in the Ristretto group and for torsion-free Edwards points (a point with torsion
        changes it by a small-order point, as in verify_batch).  No comb table is built (precomp_rows_table_bytes is unchanged)."""
        ss = np.ascontiguousarray(static_scalars, dtype=np.uint8)
        assert ss.ndim == 3 and ss.shape[2] == 32, "static_scalars must have shape (m, w, 32)"
        m, w = ss.shape[0], ss.shape[1]
        ds = _np8(dyn_scalars, 32) if len(dyn_scalars) else np.zeros((0, 32), np.uint8)
        dp = _np8(dyn_points, _PT.get(in_fmt, 32)) if len(dyn_points) else np.zeros((0, _PT.get(in_fmt, 32)), np.uint8)
        assert ds.shape[0] == dp.shape[0]
        off = np.ascontiguousarray(np.asarray(dyn_off, dtype=np.uint64).reshape(-1))
        assert off.shape[0] == m + 1, "dyn_off must hold m + 1 offsets"
        wt = np.ascontiguousarray(weights, dtype=np.uint8)
        assert wt.ndim == 2 and wt.shape[0] == m, "weights must have shape (m, 16) or (m, 32)"
        out = C.create_string_buffer(_PT.get(out_fmt, 32))
        self._bind_stream()
        st = self._chk(self.lib.c25519_precomp_msm_vartime_mixed_rows_fold(self.ctx, h, ss.ctypes.data, m, w, ds.ctypes.data, dp.ctypes.data, ds.shape[0], in_fmt,
                                                                           off.ctypes.data, wt.ctypes.data, wt.shape[1], out_fmt, out), (OK, NONE))
        return st, out.raw

    @staticmethod
    def precomp_msm_vartime_mixed_rows_fold_plan(m, w, dyn_off, weight_bytes=16):
        """the MSM precomp_msm_vartime_mixed_rows_fold leaves behind and how its column fold is cut -> (static terms of the final MSM, its dynamic
        terms, row slices of the column fold, rows per slice).  Host arithmetic: needs no GPU and no context (a static method); a shape the
        call would reject raises."""
        off = np.ascontiguousarray(np.asarray(dyn_off, dtype=np.uint64).reshape(-1))
        assert m == 0 or off.shape[0] == m + 1, "dyn_off must hold m + 1 offsets"
        plan = np.zeros(4, np.uint64)
        st = load_library().c25519_precomp_msm_vartime_mixed_rows_fold_plan(m, w, off.ctypes.data if off.size else None, weight_bytes, plan.ctypes.data)
        if st < 0:
            raise EngineError("HIP error %d: precomp_msm_vartime_mixed_rows_fold_plan: weight_bytes must be 16 or 32, m below 2^32 - 1, m * w must not overflow, "
                              "dyn_off must be m + 1 non-decreasing values from 0, below 2^40" % -st)
        return tuple(int(x) for x in plan)

    def msm_consttime(self, scalars, points, in_fmt=FMT_RAW160, out_fmt=FMT_EDWARDS_Y):
        s = _np8(scalars, 32); p = _np8(points, _PT[in_fmt])
        assert s.shape[0] == p.shape[0]
        out = C.create_string_buffer(_PT[out_fmt])
        self._bind_stream()
        st = self._chk(self.lib.c25519_msm_consttime(self.ctx, s.ctypes.data, p.ctypes.data, s.shape[0], in_fmt, out_fmt, out), (OK, NONE))
        return st, out.raw

    def double_and_compress_batch(self, pts):
        p = _np8(pts, 160); n = p.shape[0]
        out = np.empty((n, 32), dtype=np.uint8)
        self._bind_stream()
        self._chk(self.lib.c25519_double_and_compress_batch(self.ctx, p.ctypes.data, n, out.ctypes.data))
        return out

    # -- hash-to-group, host buffers: -> numpy (n, 32) or (n, 160) uint8
    def ristretto_from_uniform_bytes_batch(self, in64, out_fmt=FMT_RISTRETTO, out=None):
        a = _np8(in64, 64) if len(in64) else np.empty((0, 64), np.uint8); n = a.shape[0]
        out = self._out(out, n, _PT[out_fmt])
        self._bind_stream()
        self._chk(self.lib.c25519_ristretto_from_uniform_bytes_batch(self.ctx, a.ctypes.data, n, out_fmt, out.ctypes.data))
        return out

    def ristretto_map_to_curve_batch(self, in32, out_fmt=FMT_RISTRETTO, out=None):
        a = _np8(in32, 32) if len(in32) else np.empty((0, 32), np.uint8); n = a.shape[0]
        out = self._out(out, n, _PT[out_fmt])
        self._bind_stream()
        self._chk(self.lib.c25519_ristretto_map_to_curve_batch(self.ctx, a.ctypes.data, n, out_fmt, out.ctypes.data))
        return out

    @staticmethod
    def _pack_off(msgs, msg_off):
        """msgs: a list of byte strings, or (blob, offsets) already packed"""
        if msg_off is None:
            return Engine._pack(list(msgs))
        return np.ascontiguousarray(np.frombuffer(bytes(msgs), dtype=np.uint8)), np.ascontiguousarray(msg_off, dtype=np.uint64)

    def ristretto_hash_from_bytes_batch(self, msgs, out_fmt=FMT_RISTRETTO, msg_off=None, out=None):
        blob, off = self._pack_off(msgs, msg_off)
        n = off.shape[0] - 1
        out = self._out(out, n, _PT[out_fmt])
        self._bind_stream()
        self._chk(self.lib.c25519_ristretto_hash_from_bytes_batch(self.ctx, blob.ctypes.data, off.ctypes.data, n, out_fmt, out.ctypes.data))
        return out

    def edwards_hash_to_curve_batch(self, msgs, dst, mode=H2C_RO, out_fmt=FMT_EDWARDS_Y, msg_off=None, out=None):
        """RFC 9380 edwards25519_XMD:SHA-512_ELL2_RO_ (mode H2C_RO) / _NU_ (H2C_NU) with one DST for the batch.
        -> numpy array, or DOMAIN_SEPARATOR_LENGTH (an int) when the DST is empty or longer than 255 bytes."""
        blob, off = self._pack_off(msgs, msg_off)
        n = off.shape[0] - 1
        out = self._out(out, n, _PT[out_fmt])
        dst = bytes(dst)
        self._bind_stream()
        st = self._chk(self.lib.c25519_edwards_hash_to_curve_batch(self.ctx, blob.ctypes.data, off.ctypes.data, n, dst, len(dst), mode, out_fmt, out.ctypes.data),
                       (OK, DOMAIN_SEPARATOR_LENGTH))
        return out if st == OK else st

    # -- Lizard, host buffers (D = Sha256)
    def ristretto_lizard_encode_batch(self, data16, out_fmt=FMT_RISTRETTO, out=None):
        """(n, 16) payloads -> numpy (n, 32) CompressedRistretto or (n, 160) RAW160"""
        a = _np8(data16, 16) if len(data16) else np.empty((0, 16), np.uint8); n = a.shape[0]
        out = self._out(out, n, _PT.get(out_fmt, 32))
        self._bind_stream()
        self._chk(self.lib.c25519_ristretto_lizard_encode_sha256_batch(self.ctx, a.ctypes.data, n, out_fmt, out.ctypes.data))
        return out

    def ristretto_lizard_decode_batch(self, points, in_fmt=FMT_RISTRETTO, out=None, status=None):
        """-> (payloads numpy (n, 16), zero unless OK; status numpy (n,) uint8 of LIZARD_*).  out / status: buffers to reuse"""
        a = _np8(points, _PT.get(in_fmt, 32)) if len(points) else np.empty((0, _PT.get(in_fmt, 32)), np.uint8); n = a.shape[0]
        out = self._out(out, n, 16)
        st = self._out(status, n, 1)
        self._bind_stream()
        self._chk(self.lib.c25519_ristretto_lizard_decode_sha256_batch(self.ctx, a.ctypes.data, n, in_fmt, out.ctypes.data, st.ctypes.data))
        return out, st

    def ristretto_map_to_curve_inverse_batch(self, points, in_fmt=FMT_RISTRETTO, out=None):
        """-> (preimages numpy (n, 16, 32), an undefined slot zero; mask numpy (n,) uint16, bit j = slot j defined;
        ok numpy (n,) uint8, 1 = valid encoding (all ones for RAW160 input)).  out: an (n, 16, 32) uint8 buffer to reuse"""
        a = _np8(points, _PT.get(in_fmt, 32)) if len(points) else np.empty((0, _PT.get(in_fmt, 32)), np.uint8); n = a.shape[0]
        out = self._out(out, n, 512).reshape(n, 16, 32)
        mask = np.empty((n,), np.uint16)
        ok = np.ones((n,), np.uint8)
        self._bind_stream()
        self._chk(self.lib.c25519_ristretto_map_to_curve_inverse_batch(self.ctx, a.ctypes.data, n, in_fmt, out.ctypes.data, mask.ctypes.data, ok.ctypes.data))
        return out, mask, ok

    # -- MontgomeryPoint, host buffers
    def montgomery_mul_batch(self, k, u, out=None):
        """u(k_i * P_i), unclamped (Mul<&Scalar>, montgomery.rs:484-492) -> numpy (n, 32)"""
        k = _np8(k, 32); u = _np8(u, 32); n = k.shape[0]
        assert u.shape[0] == n
        out = self._out(out, n, 32)
        self._bind_stream()
        self._chk(self.lib.c25519_montgomery_mul_batch(self.ctx, k.ctypes.data, u.ctypes.data, n, out.ctypes.data))
        return out

    def montgomery_mul_bits_be_batch(self, bits, nbits, u, out=None):
        """mul_bits_be (montgomery.rs:183-211): bits (n, ceil(nbits/8)) MSB first, one nbits for all items -> numpy (n, 32)"""
        u = _np8(u, 32); n = u.shape[0]
        nb = (nbits + 7) // 8
        b = _np8(bits, nb) if nb else np.empty((n, 0), np.uint8)
        assert b.shape[0] == n
        out = self._out(out, n, 32)
        self._bind_stream()
        self._chk(self.lib.c25519_montgomery_mul_bits_be_batch(self.ctx, b.ctypes.data if nb else None, nbits, u.ctypes.data, n, out.ctypes.data))
        return out

    def montgomery_mul_base_batch(self, scalars, out=None):
        """MontgomeryPoint::mul_base (montgomery.rs:144-146), unclamped -> numpy (n, 32)"""
        s = _np8(scalars, 32); n = s.shape[0]
        out = self._out(out, n, 32)
        self._bind_stream()
        self._chk(self.lib.c25519_montgomery_mul_base_batch(self.ctx, s.ctypes.data, n, out.ctypes.data))
        return out

    def montgomery_to_edwards_batch(self, u, signs, out_fmt=FMT_EDWARDS_Y, out=None):
        """to_edwards(sign) (montgomery.rs:239-268) -> (points numpy (n, 32) or (n, 160), zero where None; status numpy (n,) uint8, 1 = Some)"""
        u = _np8(u, 32); n = u.shape[0]
        sg = np.ascontiguousarray(np.asarray(signs, dtype=np.uint8).reshape(-1))
        assert sg.shape[0] == n
        out = self._out(out, n, _PT.get(out_fmt, 32))
        st = np.empty((n,), np.uint8)
        self._bind_stream()
        self._chk(self.lib.c25519_montgomery_to_edwards_batch(self.ctx, u.ctypes.data, sg.ctypes.data, n, out_fmt, out.ctypes.data, st.ctypes.data))
        return out, st

    # -- the group law, host buffers: each returns (status OK | NONE, result numpy, ok numpy (n,) uint8)
    def point_add_batch(self, p, q, op=POINT_ADD, in_fmt=FMT_RAW160, out_fmt=FMT_RAW160):
        """p[i] + q[i] (POINT_ADD) or p[i] - q[i] (POINT_SUB) (edwards.rs:808-835, ristretto.rs:852-880)"""
        a = _np8(p, _PT.get(in_fmt, 32)); b = _np8(q, _PT.get(in_fmt, 32)); n = a.shape[0]
        assert b.shape[0] == n
        out = np.empty((n, _PT.get(out_fmt, 32)), np.uint8); ok = np.empty((n,), np.uint8)
        self._bind_stream()
        st = self._chk(self.lib.c25519_point_add_batch(self.ctx, a.ctypes.data, b.ctypes.data, n, op, in_fmt, out_fmt, out.ctypes.data, ok.ctypes.data), (OK, NONE))
        return st, out, ok

    def point_map_batch(self, p, op=POINT_NEG, in_fmt=FMT_RAW160, out_fmt=FMT_RAW160):
        """-p[i] (POINT_NEG) or [8] p[i] (POINT_MUL_BY_COFACTOR, edwards.rs:1365; Edwards only)"""
        a = _np8(p, _PT.get(in_fmt, 32)); n = a.shape[0]
        out = np.empty((n, _PT.get(out_fmt, 32)), np.uint8); ok = np.empty((n,), np.uint8)
        self._bind_stream()
        st = self._chk(self.lib.c25519_point_map_batch(self.ctx, a.ctypes.data, n, op, in_fmt, out_fmt, out.ctypes.data, ok.ctypes.data), (OK, NONE))
        return st, out, ok

    def point_eq_batch(self, p, q=None, in_fmt=FMT_RAW160, group=FMT_EDWARDS_Y):
        """p[i] == q[i] in `group`, or p[i] == identity with q None -> (status, eq (n,), ok (n,))"""
        a = _np8(p, _PT.get(in_fmt, 32)); n = a.shape[0]
        b = None
        if q is not None:
            b = _np8(q, _PT.get(in_fmt, 32))
            assert b.shape[0] == n
        eq = np.empty((n,), np.uint8); ok = np.empty((n,), np.uint8)
        self._bind_stream()
        st = self._chk(self.lib.c25519_point_eq_batch(self.ctx, a.ctypes.data, b.ctypes.data if b is not None else None, n, in_fmt, group,
                                                      eq.ctypes.data, ok.ctypes.data), (OK, NONE))
        return st, eq, ok

    def point_sum_segments(self, points, seg_off, in_fmt=FMT_RAW160, out_fmt=FMT_RAW160):
        """sums of points[seg_off[s] .. seg_off[s+1]) (impl Sum, edwards.rs:837-851): seg_off m + 1 offsets, checked here -> (status, (m, 32|160), ok (m,))"""
        a = _np8(points, _PT.get(in_fmt, 32)) if len(points) else np.zeros((0, _PT.get(in_fmt, 32)), np.uint8)
        off = np.ascontiguousarray(np.asarray(seg_off, dtype=np.uint64).reshape(-1))
        assert off.shape[0] >= 1
        m = off.shape[0] - 1
        out = np.empty((m, _PT.get(out_fmt, 32)), np.uint8); ok = np.empty((m,), np.uint8)
        self._bind_stream()
        st = self._chk(self.lib.c25519_point_sum_segments(self.ctx, a.ctypes.data, a.shape[0], in_fmt, off.ctypes.data, m, out_fmt, out.ctypes.data,
                                                          ok.ctypes.data), (OK, NONE))
        return st, out, ok

    def msm_vartime_segments(self, scalars, points, seg_off, in_fmt=FMT_RAW160, out_fmt=FMT_EDWARDS_Y):
        """many independent vartime MSMs in one call (optional_multiscalar_mul per segment, edwards.rs:1002-1031 / ristretto.rs:984):
        out[s] = sum scalars[i] * points[i] over [seg_off[s], seg_off[s+1]) -> (status OK | NONE, (m, 32|160), ok (m,)); ok[s] = 0 where a
        point of segment s does not decode.  Routed by length (msm_vartime_segments_routes): one lane per segment up to MSM_SEGMENT_DIRECT_MAX terms,
        one wave up to MSM_SEGMENT_WAVE_MAX, the bucket method for all such segments side by side up to MSM_SEGMENT_BUCKET_MAX, a single-MSM call
        per segment beyond"""
        s = _np8(scalars, 32) if len(scalars) else np.zeros((0, 32), np.uint8)
        a = _np8(points, _PT.get(in_fmt, 32)) if len(points) else np.zeros((0, _PT.get(in_fmt, 32)), np.uint8)
        assert s.shape[0] == a.shape[0]
        off = np.ascontiguousarray(np.asarray(seg_off, dtype=np.uint64).reshape(-1))
        assert off.shape[0] >= 1
        m = off.shape[0] - 1
        out = np.empty((m, _PT.get(out_fmt, 32)), np.uint8); ok = np.empty((m,), np.uint8)
        self._bind_stream()
        st = self._chk(self.lib.c25519_msm_vartime_segments(self.ctx, s.ctypes.data, a.ctypes.data, s.shape[0], in_fmt, off.ctypes.data, m, out_fmt,
                                                            out.ctypes.data, ok.ctypes.data), (OK, NONE))
        return st, out, ok

    @staticmethod
    def msm_vartime_segments_plan(seg_off):
        """how msm_vartime_segments routes these m + 1 offsets -> (lane segments, wave segments, segments longer than the wave maximum, passes
        of the lane and wave segments, most terms resident in one such pass): at most MSM_SEGMENT_DIRECT_MAX terms run one per lane, at most
        MSM_SEGMENT_WAVE_MAX one per wave, longer ones on the bucket route or through the single-MSM path (msm_vartime_segments_routes tells
        which).  Host arithmetic: needs no GPU and no context (a static method); offsets the call would reject raise."""
        off = np.ascontiguousarray(np.asarray(seg_off, dtype=np.uint64).reshape(-1))
        assert off.shape[0] >= 1
        plan = np.zeros(5, np.uint64)
        st = load_library().c25519_msm_vartime_segments_plan(off.ctypes.data, off.shape[0] - 1, plan.ctypes.data)
        if st < 0:
            raise EngineError("HIP error %d: msm_vartime_segments_plan: seg_off must be m + 1 non-decreasing values from 0, below 2^40" % -st)
        return tuple(int(x) for x in plan)

    @staticmethod
    def msm_vartime_segments_routes(seg_off):
        """the route of every segment of these m + 1 offsets -> (m,) uint8 of MSM_SEGMENT_ROUTE_LANE / _WAVE / _BUCKET / _SINGLE, by its length
        alone.  Host arithmetic: needs no GPU and no context (a static method); offsets the call would reject raise."""
        off = np.ascontiguousarray(np.asarray(seg_off, dtype=np.uint64).reshape(-1))
        assert off.shape[0] >= 1
        route = np.zeros(off.shape[0] - 1, np.uint8)
        st = load_library().c25519_msm_vartime_segments_routes(off.ctypes.data, off.shape[0] - 1, route.ctypes.data)
        if st < 0:
            raise EngineError("HIP error %d: msm_vartime_segments_routes: seg_off must be m + 1 non-decreasing values from 0, below 2^40" % -st)
        return route

    @staticmethod
    def msm_route(kind, n, in_fmt=FMT_RAW160, host_pointers=False):
        """which path serves a call (c25519_msm_route) -> dict: kind 0 = msm_vartime over n points of in_fmt, 1 = verify_batch of n signatures (device z-mode).
        path: "empty" | "small" | "mid" | "pipeline"; c: window width; passes; per: terms (signatures) per pass; publish: the last kernel publishes the
        record itself; prep_points: records are made first; layout_terms.  Host arithmetic: needs no GPU and no context (a static method)."""
        r = np.zeros(7, np.int64)
        st = load_library().c25519_msm_route(kind, n, in_fmt, 1 if host_pointers else 0, r.ctypes.data)
        if st < 0:
            raise EngineError("HIP error %d: msm_route: kind must be 0 or 1, in_fmt a point format, n below 2^40" % -st)
        return {"path": ("empty", "small", "mid", "pipeline")[int(r[0])], "c": int(r[1]), "passes": int(r[2]), "per": int(r[3]), "publish": bool(r[4]),
                "prep_points": bool(r[5]), "layout_terms": int(r[6])}

    def scalar_invert_batch(self, scalars):
        """-> (inverses (n,32), product of all inverses (32 bytes)); inputs must be canonical and non-zero."""
        s = _np8(scalars, 32).copy(); n = s.shape[0]
        prod = C.create_string_buffer(32)
        self._bind_stream()
        self._chk(self.lib.c25519_scalar_invert_batch(self.ctx, s.ctypes.data, n, prod))
        return s, prod.raw


def fold_partial_records(records, out_fmt=FMT_EDWARDS_Y):
    """records: (count, PARTIAL_RECORD_BYTES) uint8 array on the HOST -> (status, bytes | None).  Host arithmetic in the C
    library (c25519_fold_partial_records); needs no GPU."""
    lib = load_library()
    r = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, PARTIAL_RECORD_BYTES)
    out = C.create_string_buffer(_PT[out_fmt])
    st = lib.c25519_fold_partial_records(None, r.ctypes.data, r.shape[0], out_fmt, out)
    if st < 0:
        raise EngineError("c25519_fold_partial_records failed with status %d" % st)
    return (st, out.raw if st == OK else None)


def fold_verify_records(records):
    """records of every rank's share of ONE batch equation -> the reference's verdict (status code)."""
    lib = load_library()
    r = np.ascontiguousarray(records, dtype=np.uint8).reshape(-1, PARTIAL_RECORD_BYTES)
    st = lib.ed25519_fold_verify_records(None, r.ctypes.data, r.shape[0])
    if st < 0:
        raise EngineError("ed25519_fold_verify_records failed with status %d" % st)
    return st


def partial_record_pack(point160, status=OK, counters=None):
    """A record holding a given 160-byte point (c25519_partial_record_pack) -> bytes."""
    lib = load_library()
    out = C.create_string_buffer(PARTIAL_RECORD_BYTES)
    cnt = None
    if counters is not None:
        cnt = (C.c_uint32 * 8)(*[int(c) for c in counters])
    st = lib.c25519_partial_record_pack(bytes(point160), status, cnt, out)
    if st != 0:
        raise EngineError("c25519_partial_record_pack failed with status %d" % st)
    return out.raw


def batch_transcript_zs(hram, sigs):
    """The reference's z_i (batch.rs:168-222) from every H(R||A||M) (n, 64) and every signature (n, 64; s = bytes 32..63)
    of the batch, on the host: -> (n, 16) uint8."""
    lib = load_library()
    h = _np8(hram, 64); g = _np8(sigs, 64); n = h.shape[0]
    assert g.shape[0] == n
    z = np.zeros((n, 16), dtype=np.uint8)
    lib.ed25519_batch_transcript_zs(h.ctypes.data, g.ctypes.data, n, z.ctypes.data)
    return z


def msm_vartime_multi(engines, scalars, points, in_fmt=FMT_RAW160, out_fmt=FMT_EDWARDS_Y):
    """c25519_msm_vartime_multi: one process, several contexts (GPUs); -> (status, bytes)"""
    s = _np8(scalars, 32); p = _np8(points, _PT[in_fmt]); n = s.shape[0]
    assert p.shape[0] == n and len(engines) >= 1
    arr = (C.c_void_p * len(engines))(*[e.ctx for e in engines])
    out = C.create_string_buffer(_PT[out_fmt])
    st = engines[0]._chk(engines[0].lib.c25519_msm_vartime_multi(arr, len(engines), s.ctypes.data, p.ctypes.data, n, in_fmt, out_fmt, out), (OK, NONE))
    return st, out.raw


def verify_batch_multi(engines, msgs, sigs, pks, z_mode=Z_TRANSCRIPT):
    """ed25519_verify_batch_multi: one process, several contexts (GPUs); -> status"""
    if not (len(msgs) == len(sigs) == len(pks)):
        return ARRAY_LENGTH
    n = len(msgs)
    if n == 0:
        return OK
    Engine._check_items(sigs, 64, "signature"); Engine._check_items(pks, 32, "public key")
    blob, off = Engine._pack(list(msgs))
    s = _np8(b"".join(sigs), 64); p = _np8(b"".join(pks), 32)
    arr = (C.c_void_p * len(engines))(*[e.ctx for e in engines])
    return engines[0]._chk(engines[0].lib.ed25519_verify_batch_multi(arr, len(engines), blob.ctypes.data, off.ctypes.data, s.ctypes.data, p.ctypes.data, n, z_mode),
                           (OK, NONE, SCALAR_FORMAT, VERIFY))
