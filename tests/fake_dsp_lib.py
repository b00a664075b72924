"""A stand-in for the loaded libdspeed_hip.so, for tests of the Python half of a gufunc call on a machine without a GPU.

``with installed() as fake:`` puts it where ``dspeed_amd._lib.lib()`` finds the library and takes it out again.  "Device" memory is host memory:
``dsp_malloc`` / ``dsp_host_alloc`` hand out real buffers, the copies are ``memmove``, ``dsp_memset`` is ``memset``, the frees release.  Every
single-processor entry point ``dsp_<name>_f32`` / ``_f64`` writes nothing, returns 0 and records its name and arguments in ``fake.calls``:
a pointer into a ``dsp_malloc`` allocation as ``["ptr", allocation index, byte offset, bytes of the allocation]``, a ``byref`` as ``"byref"``,
numbers and ``None`` as given.  Not a conftest, not collected: a plain helper (tests/test_gufunc_calls_cpu.py, tools/record_gufunc_calls.py)."""
import contextlib
import ctypes as C
import re

import numpy as np

_ENTRY = re.compile(r"dsp_[a-z0-9_]+_(f32|f64)")


class FakeLib:
    def __init__(self, real=None):
        self.real = real  # the library that was loaded before, if one was: memory of its own that is released meanwhile goes back to it
        # [address, bytes, buffer, live] in allocation order: the index is what a recorded pointer names.  A freed buffer is kept until the
        # stand-in goes, so that no later allocation gets its addresses and a pointer always names one allocation
        self.device = []
        self.host = {}    # address -> buffer
        self.calls = []

    # ---- memory
    @staticmethod
    def _buffer(nbytes):
        buf = np.zeros(max(int(nbytes), 1), dtype=np.uint8)  # (zeroed lazily by the OS where it is large)
        return buf.ctypes.data, buf

    def dsp_malloc(self, ref, nbytes):
        addr, buf = self._buffer(nbytes)
        self.device.append([addr, max(int(nbytes), 1), buf, True])
        ref._obj.value = addr
        return 0

    def dsp_free(self, ptr):
        for a in self.device:
            if a[0] == _address(ptr) and a[3]:
                a[3] = False
                return 0
        if self.real is not None:  # (an array of an earlier test, collected now)
            return self.real.dsp_free(ptr)
        raise AssertionError(f"dsp_free of {ptr!r}: not a live allocation")

    def dsp_host_alloc(self, ref, nbytes):
        addr, buf = self._buffer(nbytes)
        self.host[addr] = buf
        ref._obj.value = addr
        return 0

    def dsp_host_free(self, ptr):
        if _address(ptr) not in self.host and self.real is not None:
            return self.real.dsp_host_free(ptr)
        del self.host[_address(ptr)]
        return 0

    def dsp_h2d(self, dev, host, nbytes):
        C.memmove(_address(dev), _address(host), int(nbytes))
        return 0

    dsp_d2h = dsp_h2d  # (destination first in both)

    def dsp_memset(self, dev, value, nbytes, stream):
        C.memset(_address(dev), value, int(nbytes))
        return 0

    def live(self):
        """allocations of dsp_malloc not yet freed"""
        return sum(1 for a in self.device if a[3])

    # ---- the single-processor entry points
    def _name(self, value):
        if value is None or isinstance(value, float):
            return value
        if isinstance(value, (int, np.integer)):
            for k, (addr, nbytes, _, live) in enumerate(self.device):
                if addr <= int(value) < addr + nbytes:
                    assert live, "a pointer into freed device memory"
                    return ["ptr", k, int(value) - addr, nbytes]
            return int(value)
        if type(value).__name__ == "CArgObject":
            return "byref"
        raise AssertionError(f"unexpected argument {value!r} ({type(value).__name__})")

    def __getattr__(self, name):
        if not _ENTRY.fullmatch(name):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append([name] + [self._name(a) for a in args])
            return 0

        return entry


def _address(p):
    return p.value if isinstance(p, C.c_void_p) else int(p)


@contextlib.contextmanager
def installed():
    """the stand-in as the loaded library; the page-locked bounce buffer of the synchronous copies is the stand-in's for that time too
    (a buffer of the real library is put back afterwards, and the stand-in's is never left behind for it)"""
    from dspeed_amd import _lib, device

    real, bounce = _lib._lib, device._Bounce._local.__dict__.pop("buf", None)
    fake = FakeLib(real)
    _lib._lib = fake
    try:
        yield fake
    finally:
        device._Bounce._local.__dict__.pop("buf", None)
        if bounce is not None:
            device._Bounce._local.buf = bounce
        _lib._lib = real
