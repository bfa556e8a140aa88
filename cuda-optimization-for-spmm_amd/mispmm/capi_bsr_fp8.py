"""ctypes binding of include/mispmm_bsr_fp8.h (libmispmm_bsr_fp8.so: the block-sparse product with A's blocks and B in fp8
e4m3 on MFMA, a thirteenth library beside libmispmm.so).

Loaded through capi.SideLibrary, which says why check() and last_kernel() go through the library's own handle.
MISPMM_BSR_FP8_LIB points at another build."""
import ctypes

from . import capi

_c = ctypes
_vp, _u32, _i = _c.c_void_p, _c.c_uint32, _c.c_int

# name -> (restype, argtypes); every symbol include/mispmm_bsr_fp8.h declares
SIGNATURES = {
    "mispmm_bsr_fp8": (_i, [_vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _u32, _i]),
}

_side = capi.SideLibrary("libmispmm_bsr_fp8.so", "MISPMM_BSR_FP8_LIB", SIGNATURES)
LIB_PATH = _side.path
lib, check, last_error, last_kernel = _side.lib, _side.check, _side.last_error, _side.last_kernel
