"""Can the HIP runtime register host memory the process already has (hipHostRegister)?

The shared-memory exchange's zero-copy windows need it: every rank registers the POSIX segment so that
its walk writes into it and the device merge reads it (pe_hostx.cpp hx_zc_register).  Some machines
(a GPU passed through to a virtual machine) have no such registration; there the ranks agree on the
copying all-gather instead, and the tests whose subject is the zero-copy windows skip themselves.

The probe asks the runtime libplacement.so is linked against (looked up through the library's handle,
as _abi.hip_memcpy does) to register one shared anonymous mapping with the engine's flags."""
import ctypes
import functools
import mmap

from placement import _abi

REASON = "hipHostRegister is not supported here (the zero-copy exchange windows need the shared segment registered)"
HIP_HOST_REGISTER_PORTABLE, HIP_HOST_REGISTER_MAPPED = 1, 2


@functools.lru_cache(maxsize=None)
def host_register_supported() -> bool:
    lib = _abi.load()
    reg, unreg, last = lib.hipHostRegister, lib.hipHostUnregister, lib.hipGetLastError
    reg.restype = unreg.restype = last.restype = ctypes.c_int
    reg.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint]
    unreg.argtypes = [ctypes.c_void_p]
    last.argtypes = []
    seg = mmap.mmap(-1, 1 << 16)   # MAP_SHARED, as the segment's mapping is
    view = ctypes.c_char.from_buffer(seg)
    try:
        ok = reg(ctypes.addressof(view), len(seg), HIP_HOST_REGISTER_MAPPED | HIP_HOST_REGISTER_PORTABLE) == 0
        if ok:
            unreg(ctypes.addressof(view))
        last()   # (a failed registration is an answer, not an error left for the next HIP call)
    finally:
        del view
        seg.close()
    return ok
