"""ctypes binding of include/mispmm_attn_fp8_decode.h (libmispmm_attn_fp8_decode.so: decode attention on a paged fp8 e4m3 KV
cache with the query heads of a KV group packed into one MFMA tile, a seventeenth library beside libmispmm.so).

Loaded through capi.SideLibrary, which says why check() and last_kernel() go through the library's own handle.
MISPMM_ATTN_FP8_DECODE_LIB points at another build."""
import ctypes

from . import capi

_c = ctypes
_vp, _u32, _u64 = _c.c_void_p, _c.c_uint32, _c.c_uint64

# name -> (restype, argtypes); every symbol include/mispmm_attn_fp8_decode.h declares
SIGNATURES = {
    "mispmm_attn_decode_fp8_workspace": (_u64, [_u32, _u32, _u32, _u32, _u32]),           # B, H, kv_group, Dv, splits
    "mispmm_attn_decode_fp8": (_c.c_int, [_vp, _u32, _u32, _u32, _u32, _u32,                # stream, B, H, K, bS, numPages
                                          _vp, _vp, _vp,                                    # pagePtrs, pageIdxs, seqLens
                                          _vp, _u32, _u64, _vp, _u32, _u64, _vp, _u32, _u64,  # Q, K, V with row and head strides
                                          _u32, _u32, _c.c_float, _vp, _vp, _vp,            # D, Dv, scale, q_scale, k_scale, v_scale
                                          _vp, _u32, _u64, _c.c_int, _vp,                   # out, ldo, o_head, out_bf16, lse
                                          _u32, _u32, _vp, _u64]),                          # kv_group, splits, workspace, workspace_bytes
}

_side = capi.SideLibrary("libmispmm_attn_fp8_decode.so", "MISPMM_ATTN_FP8_DECODE_LIB", SIGNATURES)
LIB_PATH = _side.path
lib, check, last_error, last_kernel = _side.lib, _side.check, _side.last_error, _side.last_kernel
