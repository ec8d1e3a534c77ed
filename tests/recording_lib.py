"""A stand-in for libpyslam_hipvol.so that runs no code of the library: for the CPU tests of the Python binding.

RecordingLib answers every hv_* name of _lib.SIGNATURES with HV_OK and records (name, args) in .calls.  What a call writes through
its out-parameters is scripted: script(name, n, ...) gives the values its scalar out-parameters (ctypes.byref(c_int64()) and the
like) receive, in argument order (0 where nothing is scripted); every integer field of a stats struct handed in by reference
receives a distinct small prime - STATS_PRIMES[struct class][field] - or what script(name, fields={...}) names.  A volume for it is
made with volume(cls): __new__, no hv_create, nothing that needs a device."""
import ctypes

import numpy as np

from pyslam_amd import _lib as L

HANDLE = 0xBEEF
_PRIMES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
_STATS = (L.HvDeintegrateStats, L.HvPruneStats, L.HvMergeStats, L.HvPackInfo, L.HvCheckStats, L.HvDistanceStats, L.HvComponentsStats,
          L.HvRemoveComponentsStats)
# struct class -> {field: the prime an unscripted call writes there}; HvCheckStats.count holds the first five primes
STATS_PRIMES = {cls: {name: _PRIMES[i] for i, (name, _) in enumerate(cls._fields_)} for cls in _STATS if cls is not L.HvCheckStats}
STATS_PRIMES[L.HvCheckStats] = {"count": _PRIMES[:5]}


class RecordingLib:
    def __init__(self):
        self.calls = []
        self.frames = None
        self.peeked = []
        self._counts = {}
        self._fields = {}
        self._peeks = {}

    def script(self, name, *counts, fields=None, peek=None):
        """peek = {argument index, the handle being 0: (dtype, count)}: the call copies what that pointer holds into .peeked[-1][index] (operands the
        binding builds for the call alone are gone afterwards)."""
        assert name in L.SIGNATURES, name
        self._counts[name] = counts
        if fields is not None:
            self._fields[name] = dict(fields)
        if peek is not None:
            self._peeks[name] = dict(peek)
        return self

    def names(self):
        return [name for name, _ in self.calls]

    def __getattr__(self, name):
        if name not in L.SIGNATURES:
            raise AttributeError(f"the library has no {name}")

        def record(*args):
            if name == "hv_tsdf_integrate_frames":  # the frames are borrowed for the call only: read them now
                F, h, w = args[4:7]
                dt = ctypes.c_uint16 if args[2] == L.HV_DEPTH_U16 else ctypes.c_float
                self.frames = [(np.ctypeslib.as_array(ctypes.cast(args[1][f], ctypes.POINTER(dt)), shape=(h, w)).copy(),
                                np.ctypeslib.as_array(ctypes.cast(args[3][f], ctypes.POINTER(ctypes.c_uint8)), shape=(h, w, 3)).copy())
                               for f in range(F)]
            if name in self._peeks:
                self.peeked.append({i: np.ctypeslib.as_array(ctypes.cast(addr(args[i]), ctypes.POINTER(np.ctypeslib.as_ctypes_type(dt))),
                                                             shape=(n,)).copy() for i, (dt, n) in self._peeks[name].items()})
            counts = iter(self._counts.get(name, ()))
            for a in args:
                obj = getattr(a, "_obj", None)  # ctypes.byref(obj)
                if isinstance(obj, _STATS):
                    for field, value in {**STATS_PRIMES[type(obj)], **self._fields.get(name, {})}.items():
                        if isinstance(value, tuple):
                            getattr(obj, field)[:] = value
                        else:
                            setattr(obj, field, value)
                elif isinstance(obj, ctypes._SimpleCData):
                    obj.value = next(counts, 0)
            self.calls.append((name, args))
            return L.HV_OK

        return record


def volume(cls, **attributes):
    """cls.__new__ with the stand-in library, the handle HANDLE and the given attributes (what cls.__init__ would have set)."""
    vol = cls.__new__(cls)
    vol._lib = RecordingLib()
    vol._h = ctypes.c_void_p(HANDLE)
    for name, value in attributes.items():
        setattr(vol, name, value)
    return vol


def addr(a):
    """The address an argument carries (c_void_p, a typed pointer, an int) or an array holds (numpy, torch); None for None."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    if isinstance(a, ctypes.c_void_p):
        return a.value
    if isinstance(a, ctypes._Pointer):
        return ctypes.cast(a, ctypes.c_void_p).value
    return int(a)


def ref(a):
    """The object behind a ctypes.byref(...) argument."""
    return a._obj
