"""The timeline setter of the diagnostic library (`python -m xfm_amd.build --diag` -> xfm_amd/libxfm_hip_diag.so, loaded through
XFM_HIP_LIB): the default library carries no stamp code.  Used by tile_timeline.py and attn_timeline.py."""
import ctypes

from xfm_amd import _lib

NT_GEMM, ATTN_SHORT_BWD = 0, 1   # `which` of xfm_diag_set_timeline


def set_timeline(which, buf=None, flags=0):
    """Stamps of the next launches of kernel `which` go to the device tensor `buf`; None switches them off."""
    lib = _lib.load()
    try:
        fn = lib.xfm_diag_set_timeline
    except AttributeError:
        raise SystemExit(f"{_lib.LIB_PATH} has no xfm_diag_set_timeline: build the diagnostic library with `python -m xfm_amd.build --diag` "
                         f"and run with XFM_HIP_LIB=xfm_amd/libxfm_hip_diag.so") from None
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    if buf is None:
        _lib.check(fn(which, None, 0, 0), "xfm_diag_set_timeline")
    else:
        _lib.check(fn(which, buf.data_ptr(), buf.numel() * buf.element_size(), flags), "xfm_diag_set_timeline")
