"""ctypes binding of include/mispmm_attn_csr_split.h (libmispmm_attn_csr_split.so: the fused attention forward on a CSR pattern
with every long row split over several lane groups, fp32 and bf16 operands, a twelfth library beside libmispmm.so).

Loaded through capi.SideLibrary, which says why check() and last_kernel() go through the library's own handle.
MISPMM_ATTN_CSR_SPLIT_LIB points at another build."""
import ctypes

from . import capi
from .capi_attn_csr import SIGNATURES as _F32
from .capi_attn_csr_bf16 import SIGNATURES as _BF16

_c = ctypes
_vp, _u32, _u64 = _c.c_void_p, _c.c_uint32, _c.c_uint64

# name -> (restype, argtypes); every symbol include/mispmm_attn_csr_split.h declares
SIGNATURES = {
    "mispmm_attn_csr_split_workspace": (_u64, [_u32, _u32, _u32, _u32]),            # H, M, Dv, splits
    "mispmm_attn_csr_split_last_partial": (_c.c_char_p, []),                         # the partial launch's note of the last call
    # the arguments of the one-launch export, then splits, min_batches, workspace, workspace_bytes
    "mispmm_attn_csr_split_f32": (_c.c_int, _F32["mispmm_attn_csr_f32"][1] + [_u32, _u32, _vp, _u64]),
    "mispmm_attn_csr_split_bf16": (_c.c_int, _BF16["mispmm_attn_csr_bf16"][1] + [_u32, _u32, _vp, _u64]),
}

_side = capi.SideLibrary("libmispmm_attn_csr_split.so", "MISPMM_ATTN_CSR_SPLIT_LIB", SIGNATURES)
LIB_PATH = _side.path
lib, check, last_error, last_kernel = _side.lib, _side.check, _side.last_error, _side.last_kernel


def last_partial():
    """The partial launch's kernel tag of this thread's last call that launched; last_kernel() holds the combine's."""
    return lib().mispmm_attn_csr_split_last_partial().decode()
