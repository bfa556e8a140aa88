"""ctypes binding of include/mispmm_bsrc_fp8.h (libmispmm_bsrc_fp8.so: the fp8 e4m3 product on column-compacted strips in
step slots and the host helper that lays them out, a fourteenth library beside libmispmm.so).

Loaded through capi.SideLibrary, which says why check() and last_kernel() go through the library's own handle.
MISPMM_BSRC_FP8_LIB points at another build."""
import ctypes

from . import capi

_c = ctypes
_vp, _u32, _i = _c.c_void_p, _c.c_uint32, _c.c_int
_pu32 = _c.POINTER(_u32)

# name -> (restype, argtypes); every symbol include/mispmm_bsrc_fp8.h declares
SIGNATURES = {
    "mispmm_bsr_compact_slots_fp8_host": (_i, [_u32, _u32, _u32, _u32, _vp, _vp, _vp, _pu32, _pu32, _vp, _vp, _vp]),
    "mispmm_bsrc_slots_fp8": (_i, [_vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _u32, _i]),
}

_side = capi.SideLibrary("libmispmm_bsrc_fp8.so", "MISPMM_BSRC_FP8_LIB", SIGNATURES)
LIB_PATH = _side.path
lib, check, last_error, last_kernel = _side.lib, _side.check, _side.last_error, _side.last_kernel
