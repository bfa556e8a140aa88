"""ctypes binding of include/mispmm_attn_fp8_split.h (libmispmm_attn_fp8_split.so: the fp8 e4m3 fused attention forward with
every block row split over several waves and K / V heads shared by groups of query heads, a sixteenth library beside
libmispmm.so).

Loaded through capi.SideLibrary, which says why check() and last_kernel() go through the library's own handle.
MISPMM_ATTN_FP8_SPLIT_LIB points at another build."""
import ctypes

from . import capi
from .capi_attn_fp8 import SIGNATURES as _ONE_LAUNCH

_c = ctypes
_vp, _u32, _u64 = _c.c_void_p, _c.c_uint32, _c.c_uint64

# name -> (restype, argtypes); every symbol include/mispmm_attn_fp8_split.h declares
SIGNATURES = {
    "mispmm_attn_bsr_fp8_split_workspace": (_u64, [_u32, _u32, _u32, _u32, _u32]),        # H, numBlockRows, bS, Dv, splits
    # the arguments of mispmm_attn_bsr_fp8, then kv_group, splits, workspace, workspace_bytes
    "mispmm_attn_bsr_fp8_split": (_c.c_int, _ONE_LAUNCH["mispmm_attn_bsr_fp8"][1] + [_u32, _u32, _vp, _u64]),
}

_side = capi.SideLibrary("libmispmm_attn_fp8_split.so", "MISPMM_ATTN_FP8_SPLIT_LIB", SIGNATURES)
LIB_PATH = _side.path
lib, check, last_error, last_kernel = _side.lib, _side.check, _side.last_error, _side.last_kernel
