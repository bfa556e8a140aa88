"""ctypes binding of include/mispmm_attn_csr_bf16.h (libmispmm_attn_csr_bf16.so: fused attention on a CSR pattern with Q, K and V in
bf16, a seventh library beside libmispmm.so).

Loaded through capi.SideLibrary, which says why check() and last_kernel() go through the library's own handle.
MISPMM_ATTN_CSR_BF16_LIB points at another build."""
import ctypes

from . import capi

_c = ctypes
_vp, _u32, _u64, _i = _c.c_void_p, _c.c_uint32, _c.c_uint64, _c.c_int

# name -> (restype, argtypes); every symbol include/mispmm_attn_csr_bf16.h declares
SIGNATURES = {
    "mispmm_attn_csr_bf16": (_i, [_vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _u64, _u32, _vp, _u64, _u32, _u32, _vp, _u64, _u32, _u32,
                                  _c.c_float, _vp, _u64, _vp, _u64, _u32, _i, _vp]),
}

_side = capi.SideLibrary("libmispmm_attn_csr_bf16.so", "MISPMM_ATTN_CSR_BF16_LIB", SIGNATURES)
LIB_PATH = _side.path
lib, check, last_error, last_kernel = _side.lib, _side.check, _side.last_error, _side.last_kernel
