"""ctypes binding of include/mispmm_attn_csr_bwd.h (libmispmm_attn_csr_bwd.so: the backward of fused attention on a CSR pattern in fp32, a sixth library beside
libmispmm.so).

libmispmm_attn_csr_bwd.so links the libmispmm.so that lies beside it and leaves its error text and its kernel tag THERE.  check() and
last_kernel() of this module therefore read both through the handle of the library loaded here -- a lookup through a handle
covers the library's own dependencies -- and not through capi.lib(), which MISPMM_LIB may have pointed at another build.
There is no CPU fallback: a missing library raises."""
import ctypes
import os

from . import capi

PKG_DIR = capi.PKG_DIR
LIB_PATH = os.environ.get("MISPMM_ATTN_CSR_BWD_LIB") or os.path.join(PKG_DIR, "libmispmm_attn_csr_bwd.so")

_c = ctypes
_vp, _u32, _u64, _i = _c.c_void_p, _c.c_uint32, _c.c_uint64, _c.c_int

# name -> (restype, argtypes); every symbol include/mispmm_attn_csr_bwd.h declares
SIGNATURES = {
    "mispmm_attn_csr_bwd_f32": (_i, [_vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u32, _vp, _u64, _u32, _u32, _vp, _u64, _u32,
                                     _u32, _c.c_float, _vp, _u64, _vp, _u64, _u32, _vp, _vp, _u64, _u32, _vp, _vp, _u64, _u32, _vp, _u64, _u32,
                                     _vp, _u64, _u32]),
}
# what the linked libmispmm.so answers for this library's calls
_SHARED = {
    "mispmm_last_error": (_c.c_char_p, []),
    "mispmm_last_kernel": (_c.c_char_p, []),
    "mispmm_status_string": (_c.c_char_p, [_i]),
}

_lib = None


def lib():
    """Load libmispmm_attn_csr_bwd.so (once) and attach the signatures.  Raises if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} is not built -- run `make -C {PKG_DIR}`; mispmm has no CPU fallback")
        try:
            import torch  # noqa: F401  torch's HIP runtime first, as in capi.lib()
        except ImportError:
            pass
        handle = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in {**SIGNATURES, **_SHARED}.items():
            fn = getattr(handle, name)          # AttributeError if the export is missing
            fn.restype, fn.argtypes = restype, argtypes
        _lib = handle
    return _lib


def check(status):
    if status != capi.OK:
        l = lib()
        detail = l.mispmm_last_error().decode() or l.mispmm_status_string(status).decode()
        raise capi.MispmmError(status, detail)


def last_error():
    return lib().mispmm_last_error().decode()


def last_kernel():
    """Tag of the device kernel the calling thread's last compute call enqueued, as the library linked here recorded it."""
    return lib().mispmm_last_kernel().decode()
