"""An Engine whose device buffers sit between guard bands, and whose every call is audited against include/sylow_hip.h (helper of
test_guarded_engine.py and test_gpu_memory_contract.py; not a test).

GuardedArray has DeviceArray's interface over ONE allocation of GUARD + nbytes + GUARD bytes, `ptr` pointing behind the front guard.  The
whole allocation, body included, starts as the engine's current `fill` byte, so an output element no kernel stores keeps the fill and
differs between two runs under different fills.  GuardedEngine._call looks every pointer argument up among its live arrays, takes the
parameter's constness from the parsed prototypes (test_rust_ffi.parse_header) and its extent in bytes from the @shape line
(sylow_amd._shapes), runs the call, waits for the stream and then raises an AssertionError naming the entry point, the parameter and the
first offending byte offset when

  * a guard byte of any argument changed (the front guard as a negative offset),
  * the body of a `const` argument changed,
  * a non-const argument larger than its @shape extent changed beyond that extent.

`audited` collects (entry point, parameter) of every argument that went through the audit.  `written` logs, call by call, the raw bytes
of every non-const argument inside its @shape extent: the Python layer turns some outputs into a bool (is_one) or drops rows before it
returns them, and 0x5A and 0xFF are both true, so the fill comparison of test_gpu_memory_contract.py compares these bytes as well."""
import numpy as np

from sylow_amd import _lib, _shapes
from sylow_amd.engine import DeviceArray, Engine

GUARD = 4096                     # a multiple of 256 (ptr keeps the allocator's alignment); a 256-lane block storing one 64-bit word per lane is 2048
FILLS = (0x5A, 0xFF)             # 0xFF: every word >= p and every flag byte set


def constness():
    """{entry point: {pointer parameter: True (const) / False}} from the header's prototypes; every pointer parameter is one or the other"""
    from test_rust_ffi import parse_header
    return {name: {p[3]: bool(p[2]) for p in params if p[1]} for name, (_, params) in parse_header().items()}


class GuardedArray(DeviceArray):
    def __init__(self, engine, shape, dtype):
        import ctypes
        self.engine = engine
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        self.fill = engine.fill
        self.ptr = None
        p = ctypes.c_void_p()
        _lib.check(engine.lib.sylow_hip_malloc(ctypes.byref(p), self.nbytes + 2 * GUARD), "malloc")
        self.base = p.value
        self.ptr = self.base + GUARD
        whole = np.full(self.nbytes + 2 * GUARD, self.fill, dtype=np.uint8)
        _lib.check(engine.lib.sylow_hip_memcpy_h2d(self.base, whole.ctypes.data, whole.nbytes, engine.stream), "h2d")
        _lib.check(engine.lib.sylow_hip_stream_sync(engine.stream), "sync")
        engine._live[self.ptr] = self.nbytes
        engine._guarded[self.ptr] = self

    def free(self):
        if self.ptr:
            self.engine._live.pop(self.ptr, None)
            self.engine._guarded.pop(self.ptr, None)
            self.engine.lib.sylow_hip_free(self.base)
            self.ptr = self.base = None

    def whole(self):
        """front guard + body + back guard as bytes"""
        out = np.empty(self.nbytes + 2 * GUARD, dtype=np.uint8)
        _lib.check(self.engine.lib.sylow_hip_memcpy_d2h(out.ctypes.data, self.base, out.nbytes, self.engine.stream), "d2h")
        _lib.check(self.engine.lib.sylow_hip_stream_sync(self.engine.stream), "sync")
        return out


def first_difference(a, b):
    d = np.flatnonzero(a != b)
    return int(d[0]) if d.size else None


def audit_bytes(name, param, before, after, fill, nbytes, const, extent, guard=GUARD):
    """before / after: guard + body + guard of one argument around a call (`before` None: the body is not compared).  Raises AssertionError."""
    body = slice(guard, guard + nbytes)
    at = first_difference(after[:guard], np.uint8(fill))
    assert at is None, f"{name}: a write in front of {param}, at byte offset {at - guard}"
    at = first_difference(after[guard + nbytes:], np.uint8(fill))
    assert at is None, f"{name}: a write past the end of {param} ({nbytes} bytes), at byte offset {nbytes + at}"
    if before is None:
        return
    if const:
        at = first_difference(before[body], after[body])
        assert at is None, f"{name}: {param} is declared const and was modified at byte offset {at}"
    elif extent is not None and extent < nbytes:
        at = first_difference(before[body][extent:], after[body][extent:])
        assert at is None, f"{name}: a write to {param} beyond its @shape extent of {extent} bytes, at byte offset {extent + at}"


class GuardedEngine(Engine):
    def __init__(self, device=0, stream=None, fill=FILLS[0]):
        super().__init__(device, stream)
        self.fill = fill
        self._guarded = {}
        self._const = constness()
        self.audited = set()
        self.written = []                                  # (entry point, parameter, the raw bytes of its @shape extent after the call), in call order

    def empty(self, shape, dtype=np.uint64):
        return GuardedArray(self, shape, dtype)

    def _call(self, name, *args):
        names, shapes = _shapes.table().get(name, ((), {}))
        values = {}
        for n, a in zip(names, args):
            if n not in shapes and isinstance(a, (int, np.integer)) and not isinstance(a, bool):
                values[n] = int(a)
        outputs = {a for n, a in zip(names, args) if isinstance(a, int) and a in self._guarded and not self._const[name].get(n, False)}
        watched = []
        for n, a in zip(names, args):
            g = self._guarded.get(a) if isinstance(a, int) and not isinstance(a, bool) else None
            if g is None or n not in self._const.get(name, {}):
                continue
            try:
                extent = shapes[n].nbytes(values) if n in shapes else None
            except NameError:
                extent = None                              # a size argument of the expression was not an integer
            const = self._const[name][n] and a not in outputs     # an in-place call passes one array as input and output
            watched.append((n, g, const, extent, g.whole()))
        super()._call(name, *args)
        self.sync()
        for n, g, const, extent, before in watched:
            after = g.whole()
            audit_bytes(name, n, before, after, g.fill, g.nbytes, const, extent)
            self.audited.add((name, n))
            if not const and extent is not None:
                self.written.append((name, n, after[GUARD:GUARD + min(extent, g.nbytes)].copy()))
