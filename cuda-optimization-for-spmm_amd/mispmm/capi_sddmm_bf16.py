"""ctypes binding of include/mispmm_sddmm_bf16.h (libmispmm_sddmm_bf16.so: SDDMM on a CSR pattern with X and Y in bf16, a
ninth library beside libmispmm.so).

Loaded through capi.SideLibrary, which says why check() and last_kernel() go through the library's own handle.
MISPMM_SDDMM_BF16_LIB points at another build."""
import ctypes

from . import capi

_c = ctypes
_vp, _u32, _i = _c.c_void_p, _c.c_uint32, _c.c_int

# name -> (restype, argtypes); every symbol include/mispmm_sddmm_bf16.h declares
SIGNATURES = {
    "mispmm_sddmm_csr_bf16": (_i, [_vp, _u32, _u32, _u32, _vp, _vp, _vp, _u32, _vp, _u32, _u32, _vp, _i, _i]),
}

_side = capi.SideLibrary("libmispmm_sddmm_bf16.so", "MISPMM_SDDMM_BF16_LIB", SIGNATURES)
LIB_PATH = _side.path
lib, check, last_error, last_kernel = _side.lib, _side.check, _side.last_error, _side.last_kernel
