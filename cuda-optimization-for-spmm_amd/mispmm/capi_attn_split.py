"""ctypes binding of include/mispmm_attn_split.h (libmispmm_attn_split.so: the fused attention forward with every block row
split over several waves, a library beside libmispmm.so).

Loaded through capi.SideLibrary, which says why check() and last_kernel() go through the library's own handle.
MISPMM_ATTN_SPLIT_LIB points at another build."""
import ctypes

from . import capi
from .capi_attn import SIGNATURES as _ONE_WAVE

_c = ctypes
_vp, _u32, _u64 = _c.c_void_p, _c.c_uint32, _c.c_uint64

# name -> (restype, argtypes); every symbol include/mispmm_attn_split.h declares
SIGNATURES = {
    "mispmm_attn_bsr_split_workspace": (_u64, [_u32, _u32, _u32, _u32, _u32]),            # H, numBlockRows, bS, Dv, splits
    # the arguments of mispmm_attn_bsr_bf16, then splits, workspace, workspace_bytes
    "mispmm_attn_bsr_split_bf16": (_c.c_int, _ONE_WAVE["mispmm_attn_bsr_bf16"][1] + [_u32, _vp, _u64]),
}

_side = capi.SideLibrary("libmispmm_attn_split.so", "MISPMM_ATTN_SPLIT_LIB", SIGNATURES)
LIB_PATH = _side.path
lib, check, last_error, last_kernel = _side.lib, _side.check, _side.last_error, _side.last_kernel
