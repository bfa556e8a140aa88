"""ctypes binding of include/mispmm_attn_csr_bf16_bwd.h (libmispmm_attn_csr_bf16_bwd.so: the backward of fused attention on a CSR
pattern with Q, K, V and grad_out in bf16, an eighth library beside libmispmm.so).

Loaded through capi.SideLibrary, which says why check() and last_kernel() go through the library's own handle.
MISPMM_ATTN_CSR_BF16_BWD_LIB points at another build."""
import ctypes

from . import capi

_c = ctypes
_vp, _u32, _u64, _i = _c.c_void_p, _c.c_uint32, _c.c_uint64, _c.c_int

# name -> (restype, argtypes); every symbol include/mispmm_attn_csr_bf16_bwd.h declares
SIGNATURES = {
    "mispmm_attn_csr_bf16_bwd": (_i, [_vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u32, _vp, _u64, _u32, _u32, _vp, _u64, _u32,
                                      _u32, _c.c_float, _vp, _u64, _vp, _u64, _u32, _vp, _vp, _u64, _u32, _vp, _i, _vp, _u64, _u32, _vp, _u64, _u32,
                                      _vp, _u64, _u32]),
}

_side = capi.SideLibrary("libmispmm_attn_csr_bf16_bwd.so", "MISPMM_ATTN_CSR_BF16_BWD_LIB", SIGNATURES)
LIB_PATH = _side.path
lib, check, last_error, last_kernel = _side.lib, _side.check, _side.last_error, _side.last_kernel
