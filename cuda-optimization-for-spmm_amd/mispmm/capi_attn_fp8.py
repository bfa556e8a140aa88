"""ctypes binding of include/mispmm_attn_fp8.h (libmispmm_attn_fp8.so: the fused block-sparse attention forward with Q, K and
V in fp8 e4m3 on MFMA, a fifteenth library beside libmispmm.so).

Loaded through capi.SideLibrary, which says why check() and last_kernel() go through the library's own handle.
MISPMM_ATTN_FP8_LIB points at another build."""
import ctypes

from . import capi

_c = ctypes
_vp, _u32, _u64, _i = _c.c_void_p, _c.c_uint32, _c.c_uint64, _c.c_int

# name -> (restype, argtypes); every symbol include/mispmm_attn_fp8.h declares
SIGNATURES = {
    "mispmm_attn_bsr_fp8": (_i, [_vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _u32, _u64, _vp, _u32, _u64, _vp, _u32, _u64, _u32, _u32,
                                 _vp, _c.c_float, _vp, _vp, _vp, _vp, _u32, _u64, _i, _vp]),
}

_side = capi.SideLibrary("libmispmm_attn_fp8.so", "MISPMM_ATTN_FP8_LIB", SIGNATURES)
LIB_PATH = _side.path
lib, check, last_error, last_kernel = _side.lib, _side.check, _side.last_error, _side.last_kernel
