"""ctypes binding of include/mispmm_attn_csr_dbias.h (libmispmm_attn_csr_dbias.so: the bias gradient of fused attention on a CSR
pattern for fp32 and for bf16 operands, a tenth library beside libmispmm.so).

Loaded through capi.SideLibrary, which says why check() and last_kernel() go through the library's own handle.
MISPMM_ATTN_CSR_DBIAS_LIB points at another build."""
import ctypes

from . import capi

_c = ctypes
_vp, _u32, _u64, _i = _c.c_void_p, _c.c_uint32, _c.c_uint64, _c.c_int

# both entry points take the same arguments; the element type of Q, Kmat, V and grad_out is in the name
_ARGS = [_vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _u64, _u32, _vp, _u64, _u32, _u32, _vp, _u64, _u32, _u32, _c.c_float, _vp, _u64, _vp, _u64,
         _u32, _vp, _vp, _u64, _u32, _vp, _u64]

# name -> (restype, argtypes); every symbol include/mispmm_attn_csr_dbias.h declares
SIGNATURES = {
    "mispmm_attn_csr_dbias_f32": (_i, list(_ARGS)),
    "mispmm_attn_csr_dbias_bf16": (_i, list(_ARGS)),
}

_side = capi.SideLibrary("libmispmm_attn_csr_dbias.so", "MISPMM_ATTN_CSR_DBIAS_LIB", SIGNATURES)
LIB_PATH = _side.path
lib, check, last_error, last_kernel = _side.lib, _side.check, _side.last_error, _side.last_kernel
