"""ctypes binding of include/mispmm_attn_bwd.h (libmispmm_attn_bwd.so: the fused attention backward, a third library beside
libmispmm.so and libmispmm_attn.so).

Loaded through capi.SideLibrary, which says why check() and last_kernel() go through the library's own handle.
MISPMM_ATTN_BWD_LIB points at another build."""
import ctypes

from . import capi

_c = ctypes
_vp, _u32, _u64, _i = _c.c_void_p, _c.c_uint32, _c.c_uint64, _c.c_int

# name -> (restype, argtypes); every symbol include/mispmm_attn_bwd.h declares
SIGNATURES = {
    "mispmm_attn_bsr_bwd_bf16": (_i, [_vp, _u32, _u32, _u32, _u32, _u32,           # stream, H, numBlockRows, K, bS, numBlocks
                                      _vp, _vp, _vp, _vp, _vp,                      # A's and A^T's index arrays, perm
                                      _vp, _u32, _u64, _vp, _u32, _u64, _vp, _u32, _u64, _vp, _u32, _u64,   # Q, K, V, dO
                                      _vp, _u32, _u64, _i, _vp, _vp,                # out, its strides and type, lse, delta
                                      _u32, _u32, _vp, _c.c_float,                  # D, Dv, mask, scale
                                      _vp, _u32, _u64, _vp, _u32, _u64, _vp, _u32, _u64, _i]),   # dQ, dK, dV, their type
}

_side = capi.SideLibrary("libmispmm_attn_bwd.so", "MISPMM_ATTN_BWD_LIB", SIGNATURES)
LIB_PATH = _side.path
lib, check, last_error, last_kernel = _side.lib, _side.check, _side.last_error, _side.last_kernel
