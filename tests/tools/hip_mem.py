"""Device-to-device copies for the tests that reach context-owned buffers through the fu_test_* hooks."""
import ctypes as C

_hip = None


def memcpy_dtod(dst, src, nbytes):
    """hipMemcpy device -> device through the process's HIP runtime (the one torch loaded)."""
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMemcpy.restype = C.c_int
    rc = _hip.hipMemcpy(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(nbytes), 3)   # hipMemcpyDeviceToDevice
    assert rc == 0, rc
