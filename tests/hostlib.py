"""The one loader of libcubemapslam_host.so (the host build: literal loops, mirror classes, host builds of the cores) and the pointer helper for the
tests' *_hostlib modules.  Each of them declares the argument types of its own hm_* functions on the object load() returns."""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_H = None
p = lambda a: a.ctypes.data_as(C.c_void_p)


def load():
    global _H
    if _H is None:
        _H = C.CDLL(os.path.join(ROOT, "cubemapslam_amd", "lib", "libcubemapslam_host.so"))
        _H.hm_last_error.restype = C.c_char_p
    return _H
