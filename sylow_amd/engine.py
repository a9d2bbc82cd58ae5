"""Batch engine: device buffers + one method per C-ABI entry point, numpy in / numpy out.

Host-side arrays are array-of-structs uint64 [n, W] (W as in include/sylow_hip.h); the engine
transposes to the struct-of-arrays [W, n] device layout.  Device-resident use (bench.py) goes
through `DeviceArray` handles directly, so the timed region contains no host traffic.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib, _shapes


class DeviceArray:
    """A hipMalloc'ed buffer holding a numpy-shaped array (row-major)."""

    def __init__(self, engine: "Engine", shape, dtype):
        self.engine = engine
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        p = ctypes.c_void_p()
        _lib.check(engine.lib.sylow_hip_malloc(ctypes.byref(p), self.nbytes), "malloc")
        self.ptr = p.value
        engine._live[self.ptr] = self.nbytes              # what _shapes.check_call compares against the header's @shape lines

    def free(self):
        if self.ptr:
            self.engine._live.pop(self.ptr, None)
            self.engine.lib.sylow_hip_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def upload(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr, dtype=self.dtype)
        assert arr.nbytes == self.nbytes, (arr.shape, self.shape)
        _lib.check(self.engine.lib.sylow_hip_memcpy_h2d(self.ptr, arr.ctypes.data, self.nbytes, self.engine.stream), "h2d")
        _lib.check(self.engine.lib.sylow_hip_stream_sync(self.engine.stream), "sync")
        return self

    def download(self) -> np.ndarray:
        out = np.empty(self.shape, dtype=self.dtype)
        _lib.check(self.engine.lib.sylow_hip_memcpy_d2h(out.ctypes.data, self.ptr, self.nbytes, self.engine.stream), "d2h")
        _lib.check(self.engine.lib.sylow_hip_stream_sync(self.engine.stream), "sync")
        return out


def _aos(a, width):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.ndim == 1:
        a = a.reshape(-1, width)
    assert a.ndim == 2 and a.shape[1] == width, (a.shape, width)
    return a


class Engine:
    """One engine per process / GPU (one process per GPU, as torch.distributed launches them)."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self.lib = _lib.load()
        _lib.check(self.lib.sylow_hip_init(device), "sylow_hip_init")
        self.device = device
        self.stream = stream  # raw hipStream_t as int, or None for the default stream
        self._live = {}       # base pointer -> bytes of every live DeviceArray (checked against the header's @shape lines in _call)

    # ---- buffers ---------------------------------------------------------------------------
    def empty(self, shape, dtype=np.uint64) -> DeviceArray:
        return DeviceArray(self, shape, dtype)

    def to_device_soa(self, aos: np.ndarray, width: int) -> DeviceArray:
        a = _aos(aos, width)
        return self.empty((width, a.shape[0])).upload(np.ascontiguousarray(a.T))

    def to_device(self, arr: np.ndarray, dtype=None) -> DeviceArray:
        arr = np.ascontiguousarray(arr, dtype=dtype)
        return self.empty(arr.shape, arr.dtype).upload(arr)

    def from_device_soa(self, d: DeviceArray) -> np.ndarray:
        return np.ascontiguousarray(d.download().T)

    def sync(self):
        _lib.check(self.lib.sylow_hip_stream_sync(self.stream), "sync")

    def pinned_empty(self, shape, dtype=np.uint64) -> np.ndarray:
        """A numpy array over page-locked host memory (sylow_hip_host_malloc): every copy of the host pipeline is then asynchronous.
        The memory is released when the array (and every view of it) is garbage-collected."""
        dtype = np.dtype(dtype)
        nbytes = max(1, int(np.prod(shape, dtype=np.int64)) * dtype.itemsize)
        p = ctypes.c_void_p()
        _lib.check(self.lib.sylow_hip_host_malloc(ctypes.byref(p), nbytes), "host_malloc")
        lib, addr = self.lib, p.value

        class _Owner:
            def __del__(self_inner):
                try:
                    lib.sylow_hip_host_free(addr)
                except Exception:
                    pass
        buf = (ctypes.c_uint8 * nbytes).from_address(addr)
        buf._owner = _Owner()
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape, dtype=np.int64))).reshape(shape)

    def xoshiro_fp_soa(self, seed: int, n: int) -> np.ndarray:
        """n values < p from the SplitMix64-seeded xoshiro256** stream, host array in SoA layout [4, n]."""
        out = np.empty((4, n), dtype=np.uint64)
        _lib.check(self.lib.sylow_hip_host_xoshiro_fp(seed & ((1 << 64) - 1), out.ctypes.data, n, n), "xoshiro")
        return out

    def _flags(self, inf, n):
        if inf is None:
            return None
        f = np.ascontiguousarray(inf, dtype=np.uint8).reshape(n)
        return self.to_device(f)

    @staticmethod
    def _ptr(d):
        return None if d is None else d.ptr

    def _call(self, name, *args):
        # launches go to the calling thread's current device: re-assert ours (other code in the process may have switched it)
        try:
            _shapes.check_call(name, args, self._live)       # every buffer at least as large as include/sylow_hip.h's @shape says
        except ValueError as e:
            raise _lib.SylowHipError(str(e)) from None
        _lib.check(self.lib.sylow_hip_set_device(self.device), "sylow_hip_set_device")
        _lib.check(getattr(self.lib, name)(*args, self.stream), name)

    def trim(self, keep_bytes: int = 0):
        """Free this device's idle scratch blocks above `keep_bytes` whose last user has completed (sylow_hip_trim)."""
        _lib.check(self.lib.sylow_hip_set_device(self.device), "sylow_hip_set_device")
        _lib.check(self.lib.sylow_hip_trim(keep_bytes), "sylow_hip_trim")

    def set_option(self, name: str, value: int = -1):
        """A route selector / threshold of the library (sylow_hip_set_option; names = _lib.OPTIONS, value < 0 = the default).  Process-wide."""
        _lib.check(self.lib.sylow_hip_set_option(_lib.OPTIONS[name], value), "sylow_hip_set_option")

    def get_option(self, name: str) -> int:
        v = ctypes.c_int64(0)
        _lib.check(self.lib.sylow_hip_get_option(_lib.OPTIONS[name], ctypes.byref(v)), "sylow_hip_get_option")
        return int(v.value)

    def wall_clock_khz(self) -> int:
        v = ctypes.c_int32(0)
        _lib.check(self.lib.sylow_hip_wall_clock_khz(ctypes.byref(v)), "sylow_hip_wall_clock_khz")
        return int(v.value)

    def clock_probe(self, acc=None):
        """Switch the live clock probe of the metric's kernels on (acc: a zeroed DeviceArray of 256 uint64) or off (None)."""
        if acc is not None and acc.nbytes < 256 * 8:
            raise ValueError("clock_probe: the accumulator holds fewer than 256 uint64 words")
        _lib.check(self.lib.sylow_hip_clock_probe(acc.ptr if acc is not None else None), "sylow_hip_clock_probe")

    @staticmethod
    def clock_probe_summary(words, khz):
        """(sustained MHz, shader-clock ticks, wavefronts, longest wavefront in ms) from the 256 accumulator words and the constant rate."""
        w = np.asarray(words, dtype=np.uint64).reshape(64, 4)
        clk, wall, waves = int(w[:, 0].sum()), int(w[:, 1].sum()), int(w[:, 2].sum())
        mhz = clk / wall * khz / 1e3 if wall else None
        return mhz, clk, waves, (int(w[:, 3].max()) / khz if khz else None)

    def set_scratch_limit(self, nbytes: int = 0):
        """Upper bound for the multi-pair routes' line tables and g1_msm's working set (sylow_hip_set_scratch_limit; 0 = the defaults of
        12 GB and 1 GB).  Process-wide."""
        _lib.check(self.lib.sylow_hip_set_scratch_limit(nbytes), "sylow_hip_set_scratch_limit")

    def shutdown(self):
        """Free the library's scratch blocks and generator tables on every device (it stays usable)."""
        _lib.check(self.lib.sylow_hip_shutdown(), "sylow_hip_shutdown")

    # ---- field ops (numpy AoS in/out) -----------------------------------------------------
    def _binop(self, name, width, a, b):
        a, b = _aos(a, width), _aos(b, width)
        n = a.shape[0]
        da, db = self.to_device_soa(a, width), self.to_device_soa(b, width)
        do = self.empty((width, n))
        self._call(name, da.ptr, db.ptr, do.ptr, n)
        return self.from_device_soa(do)

    def _unop(self, name, width, a, *extra):
        a = _aos(a, width)
        n = a.shape[0]
        da = self.to_device_soa(a, width)
        do = self.empty((width, n))
        self._call(name, da.ptr, *extra, do.ptr, n)
        return self.from_device_soa(do)

    def fp_add(self, a, b): return self._binop("sylow_hip_fp_add_batch", 4, a, b)
    def fp_sub(self, a, b): return self._binop("sylow_hip_fp_sub_batch", 4, a, b)
    def fp_mul(self, a, b): return self._binop("sylow_hip_fp_mul_batch", 4, a, b)
    def fp_sqr(self, a): return self._unop("sylow_hip_fp_sqr_batch", 4, a)
    def fp_neg(self, a): return self._unop("sylow_hip_fp_neg_batch", 4, a)
    def fp_inv(self, a): return self._unop("sylow_hip_fp_inv_batch", 4, a)
    def fp_pow(self, a, e): return self._binop("sylow_hip_fp_pow_batch", 4, a, e)

    def fp_sqrt(self, a):
        a = _aos(a, 4)
        n = a.shape[0]
        da, do, dk = self.to_device_soa(a, 4), self.empty((4, n)), self.empty((n,), np.uint8)
        self._call("sylow_hip_fp_sqrt_batch", da.ptr, do.ptr, dk.ptr, n)
        return self.from_device_soa(do), dk.download()

    def fp_is_square(self, a):
        a = _aos(a, 4)
        n = a.shape[0]
        da, dk = self.to_device_soa(a, 4), self.empty((n,), np.uint8)
        self._call("sylow_hip_fp_is_square_batch", da.ptr, dk.ptr, n)
        return dk.download()

    def fr_add(self, a, b): return self._binop("sylow_hip_fr_add_batch", 4, a, b)
    def fr_sub(self, a, b): return self._binop("sylow_hip_fr_sub_batch", 4, a, b)
    def fr_mul(self, a, b): return self._binop("sylow_hip_fr_mul_batch", 4, a, b)
    def fr_sqr(self, a): return self._unop("sylow_hip_fr_sqr_batch", 4, a)
    def fr_neg(self, a): return self._unop("sylow_hip_fr_neg_batch", 4, a)
    def fr_inv(self, a): return self._unop("sylow_hip_fr_inv_batch", 4, a)
    # the same words as fr_inv by Montgomery's trick: ONE inversion per chunk of 2048 elements (sylow_hip_fr_batch_inv)
    def fr_batch_inv(self, a): return self._unop("sylow_hip_fr_batch_inv", 4, a)
    def fp2_mul(self, a, b): return self._binop("sylow_hip_fp2_mul_batch", 8, a, b)
    def fp2_sqr(self, a): return self._unop("sylow_hip_fp2_sqr_batch", 8, a)
    def fp2_inv(self, a): return self._unop("sylow_hip_fp2_inv_batch", 8, a)
    def fp6_mul(self, a, b): return self._binop("sylow_hip_fp6_mul_batch", 24, a, b)
    def fp6_inv(self, a): return self._unop("sylow_hip_fp6_inv_batch", 24, a)
    def fp2_residue_mul(self, a): return self._unop("sylow_hip_fp2_residue_mul_batch", 8, a)
    def fp6_sqr(self, a): return self._unop("sylow_hip_fp6_sqr_batch", 24, a)
    def fp6_residue_mul(self, a): return self._unop("sylow_hip_fp6_residue_mul_batch", 24, a)

    def _frobenius(self, name, width, a, e):
        a = _aos(a, width)
        n = a.shape[0]
        da, do = self.to_device_soa(a, width), self.empty((width, n))
        self._call(name, da.ptr, int(e), do.ptr, n)
        return self.from_device_soa(do)

    def fp2_frobenius(self, a, e): return self._frobenius("sylow_hip_fp2_frobenius_batch", 8, a, e)
    def fp6_frobenius(self, a, e): return self._frobenius("sylow_hip_fp6_frobenius_batch", 24, a, e)
    def fp12_mul(self, a, b): return self._binop("sylow_hip_fp12_mul_batch", 48, a, b)
    def fp12_sqr(self, a): return self._unop("sylow_hip_fp12_sqr_batch", 48, a)
    def fp12_inv(self, a): return self._unop("sylow_hip_fp12_inv_batch", 48, a)
    def fp12_frobenius(self, a, e): return self._unop("sylow_hip_fp12_frobenius_batch", 48, a, int(e))

    def f29_hook(self, op, a, b):
        a, b = _aos(a, 4), _aos(b, 4)
        n = a.shape[0]
        da, db = self.to_device_soa(a, 4), self.to_device_soa(b, 4)
        do = self.empty((4, n))
        self._call("sylow_hip_f29_hook_batch", int(op), da.ptr, db.ptr, do.ptr, n)
        return self.from_device_soa(do)

    def f29_raw(self, op, a, b=None, c=None, d=None, k0=0, k1=0):
        """sylow_hip_f29_raw_hook_batch: operands are (n, 9) int32 limb arrays (None = absent); returns (n, 9) int32, (n, 18) for op 13"""
        a = np.ascontiguousarray(a, dtype=np.int32).reshape(-1, 9)
        n = a.shape[0]

        def soa(x):
            if x is None:
                return None
            x = np.ascontiguousarray(x, dtype=np.int32).reshape(-1, 9)
            assert x.shape[0] == n, (x.shape, n)
            return self.to_device(np.ascontiguousarray(x.T))
        da, db, dc, dd = soa(a), soa(b), soa(c), soa(d)
        w = 18 if op == 13 else 9
        do = self.empty((w, n), np.int32)
        self._call("sylow_hip_f29_raw_hook_batch", int(op), da.ptr, self._ptr(db), self._ptr(dc), self._ptr(dd), int(k0), int(k1), do.ptr, n)
        return np.ascontiguousarray(do.download().T)

    def fp12_hook(self, op, a, b=None):
        a = _aos(a, 48)
        n = a.shape[0]
        da = self.to_device_soa(a, 48)
        db = self.to_device_soa(_aos(b, 48), 48) if b is not None else None
        do = self.empty((48, n))
        self._call("sylow_hip_fp12_hook_batch", int(op), da.ptr, self._ptr(db), do.ptr, n)
        return self.from_device_soa(do)

    def fp12_cyclotomic_sqr(self, a):
        return self._unop("sylow_hip_fp12_cyclotomic_sqr_batch", 48, a)

    def fp12_sparse_mul(self, f, ell):
        f, ell = _aos(f, 48), _aos(ell, 24)
        n = f.shape[0]
        df, dl = self.to_device_soa(f, 48), self.to_device_soa(ell, 24)
        do = self.empty((48, n))
        self._call("sylow_hip_fp12_sparse_mul_batch", df.ptr, dl.ptr, do.ptr, n)
        return self.from_device_soa(do)

    # Fp / Fr ::from_be_bytes / to_be_bytes (fp.rs:686-737, 746-778): (value mod modulus, status) -- both halves of the CtOption
    def _fe_from_bytes(self, name, blobs):
        n = len(blobs)
        assert all(len(b) == 32 for b in blobs)
        din = self.to_device(np.frombuffer(b"".join(blobs) or b"\x00", dtype=np.uint8))
        do, dst = self.empty((4, max(n, 1))), self.empty((max(n, 1),), np.uint8)
        self._call(name, din.ptr, do.ptr, dst.ptr, n)
        return self.from_device_soa(do)[:n], dst.download()[:n]

    def _fe_to_bytes(self, name, a):
        a = _aos(a, 4)
        n = a.shape[0]
        da, do = self.to_device_soa(a, 4), self.empty((n * 32,), np.uint8)
        self._call(name, da.ptr, do.ptr, n)
        raw = do.download().tobytes()
        return [raw[32 * i:32 * (i + 1)] for i in range(n)]

    def fp_from_be_bytes(self, blobs): return self._fe_from_bytes("sylow_hip_fp_from_be_bytes_batch", blobs)
    def fr_from_be_bytes(self, blobs): return self._fe_from_bytes("sylow_hip_fr_from_be_bytes_batch", blobs)
    def fp_to_be_bytes(self, a): return self._fe_to_bytes("sylow_hip_fp_to_be_bytes_batch", a)
    def fr_to_be_bytes(self, a): return self._fe_to_bytes("sylow_hip_fr_to_be_bytes_batch", a)

    # ---- groups ----------------------------------------------------------------------------
    def _scalar_mul(self, name, width, p_xy, p_inf, k):
        p_xy, k = _aos(p_xy, width), _aos(k, 4)
        n = p_xy.shape[0]
        dp, dk, di = self.to_device_soa(p_xy, width), self.to_device_soa(k, 4), self._flags(p_inf, n)
        do, doi = self.empty((width, n)), self.empty((n,), np.uint8)
        self._call(name, dp.ptr, self._ptr(di), dk.ptr, do.ptr, doi.ptr, n)
        return self.from_device_soa(do), doi.download()

    def g1_scalar_mul(self, p_xy, k, p_inf=None): return self._scalar_mul("sylow_hip_g1_scalar_mul_batch", 8, p_xy, p_inf, k)
    def g2_scalar_mul(self, p_xy, k, p_inf=None, subgroup=False):
        """k * P on the twist; subgroup=True: P is known to be in the r-torsion (4-way endomorphism split, ~1.8x faster)."""
        return self._scalar_mul("sylow_hip_g2_scalar_mul_subgroup_batch" if subgroup else "sylow_hip_g2_scalar_mul_batch", 16, p_xy, p_inf, k)

    def g2_generator_mul(self, k):
        """G2gen * k_i (the keygen shape) through the device's fixed-base table."""
        return self._generator_mul("sylow_hip_g2_generator_mul_batch", 16, k)

    def g1_generator_mul(self, k):
        """G1gen * k_i through the device's fixed-base table."""
        return self._generator_mul("sylow_hip_g1_generator_mul_batch", 8, k)

    def _generator_mul(self, name, width, k):
        k = _aos(k, 4)
        n = k.shape[0]
        dk = self.to_device_soa(k, 4)
        do, doi = self.empty((width, n)), self.empty((n,), np.uint8)
        self._call(name, dk.ptr, do.ptr, doi.ptr, n)
        return self.from_device_soa(do), doi.download()

    def g1_add(self, a_xy, b_xy, a_inf=None, b_inf=None):
        a_xy, b_xy = _aos(a_xy, 8), _aos(b_xy, 8)
        n = a_xy.shape[0]
        da, db = self.to_device_soa(a_xy, 8), self.to_device_soa(b_xy, 8)
        dai, dbi = self._flags(a_inf, n), self._flags(b_inf, n)
        do, doi = self.empty((8, n)), self.empty((n,), np.uint8)
        self._call("sylow_hip_g1_add_batch", da.ptr, self._ptr(dai), db.ptr, self._ptr(dbi), do.ptr, doi.ptr, n)
        return self.from_device_soa(do), doi.download()

    def g1_lincomb(self, p_xy, k, n_jobs, n_terms, p_inf=None):
        """sum_i k[j,i] * P[j,i]; inputs term-major: row i*n_jobs + j is term i of job j."""
        p_xy, k = _aos(p_xy, 8), _aos(k, 4)
        n = n_jobs * n_terms
        assert p_xy.shape[0] == n and k.shape[0] == n
        dp = self.to_device_soa(p_xy, 8) if n else None
        dk = self.to_device_soa(k, 4) if n else None
        di = self._flags(p_inf, n) if n else None
        do, doi = self.empty((8, n_jobs)), self.empty((n_jobs,), np.uint8)
        self._call("sylow_hip_g1_lincomb_batch", self._ptr(dp), self._ptr(di), self._ptr(dk), do.ptr, doi.ptr, n_jobs, n_terms)
        return self.from_device_soa(do), doi.download()

    def g2_add(self, a_xy, b_xy, a_inf=None, b_inf=None):
        a_xy, b_xy = _aos(a_xy, 16), _aos(b_xy, 16)
        n = a_xy.shape[0]
        da, db = self.to_device_soa(a_xy, 16), self.to_device_soa(b_xy, 16)
        dai, dbi = self._flags(a_inf, n), self._flags(b_inf, n)
        do, doi = self.empty((16, n)), self.empty((n,), np.uint8)
        self._call("sylow_hip_g2_add_batch", da.ptr, self._ptr(dai), db.ptr, self._ptr(dbi), do.ptr, doi.ptr, n)
        return self.from_device_soa(do), doi.download()

    def _group_binop(self, name, width, a_xy, b_xy, a_inf, b_inf):
        a_xy, b_xy = _aos(a_xy, width), _aos(b_xy, width)
        n = a_xy.shape[0]
        da, db = self.to_device_soa(a_xy, width), self.to_device_soa(b_xy, width)
        dai, dbi = self._flags(a_inf, n), self._flags(b_inf, n)
        do, doi = self.empty((width, n)), self.empty((n,), np.uint8)
        self._call(name, da.ptr, self._ptr(dai), db.ptr, self._ptr(dbi), do.ptr, doi.ptr, n)
        return self.from_device_soa(do), doi.download()

    def g1_sub(self, a_xy, b_xy, a_inf=None, b_inf=None): return self._group_binop("sylow_hip_g1_sub_batch", 8, a_xy, b_xy, a_inf, b_inf)
    def g2_sub(self, a_xy, b_xy, a_inf=None, b_inf=None): return self._group_binop("sylow_hip_g2_sub_batch", 16, a_xy, b_xy, a_inf, b_inf)

    def _projective_new(self, name, width, p_xyz):
        p_xyz = _aos(p_xyz, width)
        n = p_xyz.shape[0]
        dp, dst = self.to_device_soa(p_xyz, width), self.empty((n,), np.uint8)
        self._call(name, dp.ptr, dst.ptr, n)
        return dst.download()

    def g1_projective_new(self, p_xyz): return self._projective_new("sylow_hip_g1_projective_new_batch", 12, p_xyz)
    def g2_projective_new(self, p_xyz): return self._projective_new("sylow_hip_g2_projective_new_batch", 24, p_xyz)

    def _ct_eq(self, name, width, a_xyz, b_xyz):
        a_xyz, b_xyz = _aos(a_xyz, width), _aos(b_xyz, width)
        n = a_xyz.shape[0]
        da, db, deq = self.to_device_soa(a_xyz, width), self.to_device_soa(b_xyz, width), self.empty((n,), np.uint8)
        self._call(name, da.ptr, db.ptr, deq.ptr, n)
        return deq.download()

    def g1_ct_eq(self, a_xyz, b_xyz): return self._ct_eq("sylow_hip_g1_ct_eq_batch", 12, a_xyz, b_xyz)
    def g2_ct_eq(self, a_xyz, b_xyz): return self._ct_eq("sylow_hip_g2_ct_eq_batch", 24, a_xyz, b_xyz)

    def _double(self, name, width, a_xy, a_inf):
        a_xy = _aos(a_xy, width)
        n = a_xy.shape[0]
        da, dai = self.to_device_soa(a_xy, width), self._flags(a_inf, n)
        do, doi = self.empty((width, n)), self.empty((n,), np.uint8)
        self._call(name, da.ptr, self._ptr(dai), do.ptr, doi.ptr, n)
        return self.from_device_soa(do), doi.download()

    def g1_double(self, a_xy, a_inf=None): return self._double("sylow_hip_g1_double_batch", 8, a_xy, a_inf)
    def g2_double(self, a_xy, a_inf=None): return self._double("sylow_hip_g2_double_batch", 16, a_xy, a_inf)

    def gt_pow(self, gt, k):
        return self._binop_w("sylow_hip_gt_pow_batch", 48, gt, 4, k)

    def _binop_w(self, name, wa, a, wb, b):
        a, b = _aos(a, wa), _aos(b, wb)
        n = a.shape[0]
        da, db = self.to_device_soa(a, wa), self.to_device_soa(b, wb)
        do = self.empty((wa, n))
        self._call(name, da.ptr, db.ptr, do.ptr, n)
        return self.from_device_soa(do)

    def _normalize(self, name, win, wout, p):
        p = _aos(p, win)
        n = p.shape[0]
        dp = self.to_device_soa(p, win)
        do, doi = self.empty((wout, n)), self.empty((n,), np.uint8)
        self._call(name, dp.ptr, do.ptr, doi.ptr, n)
        return self.from_device_soa(do), doi.download()

    def g1_normalize(self, p_xyz): return self._normalize("sylow_hip_g1_normalize_batch", 12, 8, p_xyz)
    def g2_normalize(self, p_xyz): return self._normalize("sylow_hip_g2_normalize_batch", 24, 16, p_xyz)

    def g1_on_curve(self, p_xy, p_inf=None):
        p_xy = _aos(p_xy, 8)
        n = p_xy.shape[0]
        dp, di, dst = self.to_device_soa(p_xy, 8), self._flags(p_inf, n), self.empty((n,), np.uint8)
        self._call("sylow_hip_g1_on_curve_batch", dp.ptr, self._ptr(di), dst.ptr, n)
        return dst.download()

    def g2_psi(self, q_xy, q_inf=None):
        q_xy = _aos(q_xy, 16)
        n = q_xy.shape[0]
        dq, di = self.to_device_soa(q_xy, 16), self._flags(q_inf, n)
        do, doi, dst = self.empty((16, n)), self.empty((n,), np.uint8), self.empty((n,), np.uint8)
        self._call("sylow_hip_g2_psi_batch", dq.ptr, self._ptr(di), do.ptr, doi.ptr, dst.ptr, n)
        return self.from_device_soa(do), doi.download(), dst.download()

    def g2_subgroup_check(self, q_xy, q_inf=None):
        q_xy = _aos(q_xy, 16)
        n = q_xy.shape[0]
        dq, di = self.to_device_soa(q_xy, 16), self._flags(q_inf, n)
        ds = self.empty((n,), np.uint8)
        self._call("sylow_hip_g2_subgroup_check_batch", dq.ptr, self._ptr(di), ds.ptr, n)
        return ds.download()

    # ---- pairing ---------------------------------------------------------------------------
    def miller_loop(self, p_xy, q_xy):
        p_xy, q_xy = _aos(p_xy, 8), _aos(q_xy, 16)
        n = p_xy.shape[0]
        dp, dq = self.to_device_soa(p_xy, 8), self.to_device_soa(q_xy, 16)
        do = self.empty((48, n))
        self._call("sylow_hip_miller_loop_batch", dp.ptr, dq.ptr, do.ptr, n)
        return self.from_device_soa(do)

    def final_exp(self, f):
        return self._unop("sylow_hip_final_exp_batch", 48, f)

    def g1_sum(self, p_xy, p_inf=None):
        """sum_i P_i as one G1 point (the `+` fold of examples/verify_multiple_messages_same_signer.rs:41-60): ([1, 8] affine words, [1] flag)."""
        p_xy = _aos(p_xy, 8)
        n = p_xy.shape[0]
        dp = self.to_device_soa(p_xy, 8) if n else None
        dpi = self._flags(p_inf, n) if n else None
        do, doi = self.empty((8, 1)), self.empty((1,), np.uint8)
        self._call("sylow_hip_g1_sum_batch", self._ptr(dp), self._ptr(dpi), n, do.ptr, doi.ptr)
        return self.from_device_soa(do), doi.download()

    def g1_msm(self, p_xy, k, p_inf=None, window=-1, min_n=-1):
        """sum_i k_i * P_i as one G1 point by the bucket method (sylow_hip_g1_msm): ([1, 8] affine words, [1] flag), bit-identical to
        g1_lincomb(p_xy, k, 1, n).  k: [n, 4] Fp / Fr words (k >= p is reduced like Fp::new).  window / min_n >= 0 pin the plan
        (sylow_hip_g1_msm_tuned: window width 4..16, smallest n on the bucket route); < 0 = the defaults."""
        p_xy, k = _aos(p_xy, 8), _aos(k, 4)
        n = p_xy.shape[0]
        assert k.shape[0] == n
        dp = self.to_device_soa(p_xy, 8) if n else None
        dk = self.to_device_soa(k, 4) if n else None
        dpi = self._flags(p_inf, n) if n else None
        do, doi = self.empty((8, 1)), self.empty((1,), np.uint8)
        if window < 0 and min_n < 0:
            self._call("sylow_hip_g1_msm", self._ptr(dp), self._ptr(dpi), self._ptr(dk), n, do.ptr, doi.ptr)
        else:
            self._call("sylow_hip_g1_msm_tuned", self._ptr(dp), self._ptr(dpi), self._ptr(dk), n, int(window), int(min_n), do.ptr, doi.ptr)
        return self.from_device_soa(do), doi.download()

    def g2_sum(self, q_xy, q_inf=None):
        """sum_i Q_i as one G2 point (the `+` fold over public keys of examples/dkg.rs:309-314): ([1, 16] affine words, [1] flag)."""
        q_xy = _aos(q_xy, 16)
        n = q_xy.shape[0]
        dq = self.to_device_soa(q_xy, 16) if n else None
        dqi = self._flags(q_inf, n) if n else None
        do, doi = self.empty((16, 1)), self.empty((1,), np.uint8)
        self._call("sylow_hip_g2_sum_batch", self._ptr(dq), self._ptr(dqi), n, do.ptr, doi.ptr)
        return self.from_device_soa(do), doi.download()

    def g2_lincomb(self, p_xy, k, n_jobs, n_terms, p_inf=None):
        """sum_i k[j,i] * Q[j,i] in G2; inputs term-major: row i*n_jobs + j is term i of job j.  k >= p is reduced like Fp::new and the
        products are exact on the whole twist (no reduction mod r)."""
        p_xy, k = _aos(p_xy, 16), _aos(k, 4)
        n = n_jobs * n_terms
        assert p_xy.shape[0] == n and k.shape[0] == n
        dp = self.to_device_soa(p_xy, 16) if n else None
        dk = self.to_device_soa(k, 4) if n else None
        di = self._flags(p_inf, n) if n else None
        do, doi = self.empty((16, n_jobs)), self.empty((n_jobs,), np.uint8)
        self._call("sylow_hip_g2_lincomb_batch", self._ptr(dp), self._ptr(di), self._ptr(dk), do.ptr, doi.ptr, n_jobs, n_terms)
        return self.from_device_soa(do), doi.download()

    def g2_msm(self, p_xy, k, p_inf=None, window=-1, min_n=-1):
        """sum_i k_i * Q_i as one G2 point by the bucket method (sylow_hip_g2_msm): ([1, 16] affine words, [1] flag), bit-identical to
        g2_lincomb(p_xy, k, 1, n).  k: [n, 4] Fp words (k >= p is reduced like Fp::new; exact on the whole twist).  window / min_n >= 0
        pin the plan (sylow_hip_g2_msm_tuned: window width 4..16, smallest n on the bucket route); < 0 = the defaults."""
        p_xy, k = _aos(p_xy, 16), _aos(k, 4)
        n = p_xy.shape[0]
        assert k.shape[0] == n
        dp = self.to_device_soa(p_xy, 16) if n else None
        dk = self.to_device_soa(k, 4) if n else None
        dpi = self._flags(p_inf, n) if n else None
        do, doi = self.empty((16, 1)), self.empty((1,), np.uint8)
        if window < 0 and min_n < 0:
            self._call("sylow_hip_g2_msm", self._ptr(dp), self._ptr(dpi), self._ptr(dk), n, do.ptr, doi.ptr)
        else:
            self._call("sylow_hip_g2_msm_tuned", self._ptr(dp), self._ptr(dpi), self._ptr(dk), n, int(window), int(min_n), do.ptr, doi.ptr)
        return self.from_device_soa(do), doi.download()

    def pairing(self, p_xy, q_xy, p_inf=None, q_inf=None, pipelined=True, chunk=0, out=None):
        """pairing() (pairing.rs:870-893) on host arrays: [n, 8] / [n, 16] words in, [n, 48] Gt words out.  Default: the chunked,
        double-buffered host pipeline (sylow_hip_pairing_host: the copies of chunk k - 1 / k + 1 run beside the kernels of chunk k);
        `pipelined=False` is upload -> sylow_hip_pairing_batch -> download on the engine's stream (bit-identical).  `out`: a [n, 48]
        uint64 array to fill (e.g. from `pinned_empty`)."""
        p_xy, q_xy = _aos(p_xy, 8), _aos(q_xy, 16)
        n = p_xy.shape[0]
        if pipelined:
            assert q_xy.shape[0] == n
            gt = out if out is not None else np.empty((n, 48), dtype=np.uint64)
            assert gt.shape == (n, 48) and gt.dtype == np.uint64 and gt.flags.c_contiguous
            pi = None if p_inf is None else np.ascontiguousarray(p_inf, dtype=np.uint8).reshape(n)
            qi = None if q_inf is None else np.ascontiguousarray(q_inf, dtype=np.uint8).reshape(n)
            _lib.check(self.lib.sylow_hip_set_device(self.device), "sylow_hip_set_device")
            _lib.check(self.lib.sylow_hip_pairing_host(p_xy.ctypes.data, None if pi is None else pi.ctypes.data, q_xy.ctypes.data,
                                                       None if qi is None else qi.ctypes.data, gt.ctypes.data, n, chunk), "sylow_hip_pairing_host")
            return gt
        dp, dq = self.to_device_soa(p_xy, 8), self.to_device_soa(q_xy, 16)
        dpi, dqi = self._flags(p_inf, n), self._flags(q_inf, n)
        do = self.empty((48, n))
        self._call("sylow_hip_pairing_batch", dp.ptr, self._ptr(dpi), dq.ptr, self._ptr(dqi), do.ptr, n)
        return self.from_device_soa(do)

    def multi_pairing(self, p_xy, q_xy, offsets, p_inf=None, q_inf=None, skip_infinity=False, want_gt=True):
        p_xy, q_xy = _aos(p_xy, 8), _aos(q_xy, 16)
        n = p_xy.shape[0]
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        nj = off.shape[0] - 1
        dp = self.to_device_soa(p_xy, 8) if n else self.empty((8, 1))
        dq = self.to_device_soa(q_xy, 16) if n else self.empty((16, 1))
        dpi, dqi = (self._flags(p_inf, n), self._flags(q_inf, n)) if n else (None, None)
        doff = self.to_device(off)
        dgt = self.empty((48, max(nj, 1))) if want_gt else None
        dis = self.empty((max(nj, 1),), np.uint8)
        self._call("sylow_hip_multi_pairing_batch", dp.ptr, self._ptr(dpi), dq.ptr, self._ptr(dqi), doff.ptr, nj, n,
                   1 if skip_infinity else 0, self._ptr(dgt), dis.ptr)
        gt = self.from_device_soa(dgt)[:nj] if want_gt else None
        return gt, dis.download()[:nj]

    def glued_miller_loop(self, p_xy, q_xy, offsets):
        p_xy, q_xy = _aos(p_xy, 8), _aos(q_xy, 16)
        n = p_xy.shape[0]
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        nj = off.shape[0] - 1
        dp = self.to_device_soa(p_xy, 8) if n else None
        dq = self.to_device_soa(q_xy, 16) if n else None
        doff, df = self.to_device(off), self.empty((48, max(nj, 1)))
        self._call("sylow_hip_glued_miller_loop_batch", self._ptr(dp), self._ptr(dq), doff.ptr, nj, n, df.ptr)
        return self.from_device_soa(df)[:nj]

    def pairing_product(self, p_xy, q_xy, p_inf=None, q_inf=None, skip_infinity=False):
        """prod_i e(P_i, Q_i) as ONE Gt, computed in parallel over the batch; returns (gt [1, 48], is_one)."""
        p_xy, q_xy = _aos(p_xy, 8), _aos(q_xy, 16)
        n = p_xy.shape[0]
        dp = self.to_device_soa(p_xy, 8) if n else None
        dq = self.to_device_soa(q_xy, 16) if n else None
        dpi, dqi = (self._flags(p_inf, n), self._flags(q_inf, n)) if n else (None, None)
        dgt, dis = self.empty((48, 1)), self.empty((1,), np.uint8)
        self._call("sylow_hip_pairing_product_batch", self._ptr(dp), self._ptr(dpi), self._ptr(dq), self._ptr(dqi), n,
                   1 if skip_infinity else 0, dgt.ptr, dis.ptr)
        return self.from_device_soa(dgt), bool(dis.download()[0])

    def pairing_product_partial(self, p_xy, q_xy, p_inf=None, q_inf=None, skip_infinity=False):
        """Raw Miller product of one shard (no final exponentiation), [1, 48]."""
        p_xy, q_xy = _aos(p_xy, 8), _aos(q_xy, 16)
        n = p_xy.shape[0]
        dp = self.to_device_soa(p_xy, 8) if n else None
        dq = self.to_device_soa(q_xy, 16) if n else None
        dpi, dqi = (self._flags(p_inf, n), self._flags(q_inf, n)) if n else (None, None)
        df = self.empty((48, 1))
        self._call("sylow_hip_pairing_product_partial_batch", self._ptr(dp), self._ptr(dpi), self._ptr(dq), self._ptr(dqi), n,
                   1 if skip_infinity else 0, df.ptr)
        return self.from_device_soa(df)

    def fp12_product_final_exp(self, parts):
        """final_exponentiation(prod parts) for parts [k, 48]; returns (gt [1, 48], is_one)."""
        parts = _aos(parts, 48)
        k = parts.shape[0]
        dpa = self.to_device_soa(parts, 48) if k else None
        dgt, dis = self.empty((48, 1)), self.empty((1,), np.uint8)
        self._call("sylow_hip_fp12_product_final_exp", self._ptr(dpa), k, dgt.ptr, dis.ptr)
        return self.from_device_soa(dgt), bool(dis.download()[0])

    def pairing_product_all(self, p_xy, q_xy, comm=None, p_inf=None, q_inf=None, skip_infinity=False):
        """glued_pairing over the union of all ranks' pairs (comm = raw ncclComm_t as int, None = one rank)."""
        p_xy, q_xy = _aos(p_xy, 8), _aos(q_xy, 16)
        n = p_xy.shape[0]
        dp = self.to_device_soa(p_xy, 8) if n else None
        dq = self.to_device_soa(q_xy, 16) if n else None
        dpi, dqi = (self._flags(p_inf, n), self._flags(q_inf, n)) if n else (None, None)
        dgt, dis = self.empty((48, 1)), self.empty((1,), np.uint8)
        self._call("sylow_hip_pairing_product_all", self._ptr(dp), self._ptr(dpi), self._ptr(dq), self._ptr(dqi), n,
                   1 if skip_infinity else 0, comm, dgt.ptr, dis.ptr)
        return self.from_device_soa(dgt), bool(dis.download()[0])

    def all_valid(self, dflags: DeviceArray, comm=None) -> int:
        """AND of this rank's flags AND-ed over every rank of `comm` (raw ncclComm_t as int, None = one rank)."""
        out = self.empty((1,), np.int32)
        self._call("sylow_hip_all_valid", dflags.ptr, dflags.shape[0], comm, out.ptr)
        return int(out.download()[0])

    # G2PreComputed consumers (pairing.rs:590-619, 970-1022): coeffs [m, 87*24] as g2_precompute returns them
    @staticmethod
    def _check_table_idx(table_idx, n, m):
        """table_idx is consumed unchecked on the device (coeffs[table_idx[i]]): validate it while it is still a host array."""
        if table_idx is None:
            if n != m:
                raise ValueError(f"without table_idx, pair i reads table i: {n} G1 points need {n} tables, got {m}")
            return None
        ti = np.ascontiguousarray(table_idx, dtype=np.uint64).reshape(-1)
        if ti.shape[0] != n:
            raise ValueError(f"table_idx has {ti.shape[0]} entries for {n} G1 points")
        if n and (m == 0 or int(ti.max()) >= m):
            raise ValueError(f"table_idx refers to table {int(ti.max()) if n else 0}, only {m} tables were given")
        return ti

    def miller_loop_precomputed(self, coeffs, p_xy, table_idx=None):
        coeffs, p_xy = _aos(coeffs, 87 * 24), _aos(p_xy, 8)
        n, m = p_xy.shape[0], coeffs.shape[0]
        table_idx = self._check_table_idx(table_idx, n, m)
        dc, dp = self.to_device_soa(coeffs, 87 * 24), self.to_device_soa(p_xy, 8)
        dti = self.to_device(np.ascontiguousarray(table_idx, dtype=np.uint64)) if table_idx is not None else None
        do = self.empty((48, n))
        self._call("sylow_hip_miller_loop_precomputed_batch", dc.ptr, m, self._ptr(dti), dp.ptr, do.ptr, n)
        return self.from_device_soa(do)

    def glued_miller_loop_precomputed(self, coeffs, p_xy, offsets, table_idx=None):
        coeffs, p_xy = _aos(coeffs, 87 * 24), _aos(p_xy, 8)
        n, m = p_xy.shape[0], coeffs.shape[0]
        table_idx = self._check_table_idx(table_idx, n, m)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        nj = off.shape[0] - 1
        if nj < 0 or (nj >= 0 and (np.any(off[1:] < off[:-1]) or int(off[-1]) > n)):
            raise ValueError("offsets must be non-decreasing and end at most at the number of pairs")
        dc = self.to_device_soa(coeffs, 87 * 24) if m else None
        dp = self.to_device_soa(p_xy, 8) if n else None
        dti = self.to_device(np.ascontiguousarray(table_idx, dtype=np.uint64)) if table_idx is not None else None
        doff, df = self.to_device(off), self.empty((48, max(nj, 1)))
        self._call("sylow_hip_glued_miller_loop_precomputed_batch", self._ptr(dc), m, self._ptr(dti), self._ptr(dp), doff.ptr, nj, n, df.ptr)
        return self.from_device_soa(df)[:nj]

    # ---- wire formats ----------------------------------------------------------------------
    def _to_bytes(self, name, width, nbytes, xy, inf):
        xy = _aos(xy, width)
        n = xy.shape[0]
        d, di = self.to_device_soa(xy, width), self._flags(inf, n)
        do = self.empty((n * nbytes,), np.uint8)
        self._call(name, d.ptr, self._ptr(di), do.ptr, n)
        raw = do.download().tobytes()
        return [raw[nbytes * i:nbytes * (i + 1)] for i in range(n)]

    def _from_bytes(self, name, width, nbytes, blobs):
        n = len(blobs)
        assert all(len(b) == nbytes for b in blobs)
        din = self.to_device(np.frombuffer(b"".join(blobs), dtype=np.uint8))
        dxy, dinf, dst = self.empty((width, n)), self.empty((n,), np.uint8), self.empty((n,), np.uint8)
        self._call(name, din.ptr, dxy.ptr, dinf.ptr, dst.ptr, n)
        return self.from_device_soa(dxy), dinf.download(), dst.download()

    def g1_to_be_bytes(self, xy, inf=None): return self._to_bytes("sylow_hip_g1_to_be_bytes_batch", 8, 64, xy, inf)
    def g2_to_be_bytes(self, xy, inf=None): return self._to_bytes("sylow_hip_g2_to_be_bytes_batch", 16, 128, xy, inf)
    def g1_from_be_bytes(self, blobs): return self._from_bytes("sylow_hip_g1_from_be_bytes_batch", 8, 64, blobs)
    def g2_from_be_bytes(self, blobs): return self._from_bytes("sylow_hip_g2_from_be_bytes_batch", 16, 128, blobs)

    # ---- the value-typed calls on the reference's wire format (pipeline.hip) ----------------
    def pairing_from_bytes(self, p_blobs, q_blobs, chunk=0):
        """pairing() on G1Affine / G2Affine::to_be_bytes blobs (64 / 128 bytes each): decoding + validation on the device inside the host
        pipeline.  Returns (gt [n, 48], status_p [n], status_q [n]); an element with a non-zero status entered as the identity (Gt = 1)."""
        n = len(p_blobs)
        assert len(q_blobs) == n and all(len(b) == 64 for b in p_blobs) and all(len(b) == 128 for b in q_blobs)
        pb, qb = np.frombuffer(b"".join(p_blobs) or b"\0", dtype=np.uint8), np.frombuffer(b"".join(q_blobs) or b"\0", dtype=np.uint8)
        gt, sp, sq = np.empty((n, 48), dtype=np.uint64), np.empty((n,), dtype=np.uint8), np.empty((n,), dtype=np.uint8)
        _lib.check(self.lib.sylow_hip_set_device(self.device), "sylow_hip_set_device")
        _lib.check(self.lib.sylow_hip_pairing_host_bytes(pb.ctypes.data, qb.ctypes.data, gt.ctypes.data, sp.ctypes.data, sq.ctypes.data, n, chunk), "sylow_hip_pairing_host_bytes")
        return gt, sp, sq

    def bls_verify_from_bytes(self, pk_blobs, msgs, sig_blobs, chunk=0):
        """verify() on wire-format keys (128 bytes) and signatures (64 bytes).  Returns (ok [n], status_pk [n], status_sig [n])."""
        n = len(msgs)
        assert len(pk_blobs) == n and len(sig_blobs) == n and all(len(b) == 128 for b in pk_blobs) and all(len(b) == 64 for b in sig_blobs)
        kb, sb = np.frombuffer(b"".join(pk_blobs) or b"\0", dtype=np.uint8), np.frombuffer(b"".join(sig_blobs) or b"\0", dtype=np.uint8)
        blob = np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8)
        off = np.zeros(n + 1, dtype=np.uint64)
        if n:
            off[1:] = np.cumsum([len(m) for m in msgs])
        ok, sk, ss = np.empty((n,), dtype=np.uint8), np.empty((n,), dtype=np.uint8), np.empty((n,), dtype=np.uint8)
        _lib.check(self.lib.sylow_hip_set_device(self.device), "sylow_hip_set_device")
        _lib.check(self.lib.sylow_hip_bls_verify_host_bytes(kb.ctypes.data, blob.ctypes.data, off.ctypes.data, sb.ctypes.data, ok.ctypes.data,
                                                            sk.ctypes.data, ss.ctypes.data, n, chunk), "sylow_hip_bls_verify_host_bytes")
        return ok, sk, ss

    # ---- hashing / BLS ---------------------------------------------------------------------
    def _msgs(self, msgs):
        off = np.zeros(len(msgs) + 1, dtype=np.uint64)
        for i, m in enumerate(msgs):
            off[i + 1] = off[i] + len(m)
        blob = np.frombuffer(b"".join(msgs) or b"\x00", dtype=np.uint8)
        return self.to_device(blob), self.to_device(off)

    def fext_op(self, op, a, b=None):
        """Component-wise FieldExtension operators on Fp2 / Fp6 / Fp12 batches: op in add / sub / neg / scale (b = one Fp per element)."""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        n, width = a.shape
        degree = width // 4
        da, do = self.to_device_soa(a, width), self.empty((width, n))
        if op == "neg":
            self._call("sylow_hip_fext_neg_batch", da.ptr, do.ptr, degree, n)
        else:
            db = self.to_device_soa(_aos(b, 4 if op == "scale" else width), 4 if op == "scale" else width)
            self._call("sylow_hip_fext_%s_batch" % op, da.ptr, db.ptr, do.ptr, degree, n)
        return self.from_device_soa(do)

    def svdw_map(self, u):
        """SvdW map of field elements u [n, 4] -> (xy [n, 8], status [n])."""
        u = _aos(u, 4)
        n = u.shape[0]
        du = self.to_device_soa(u, 4)
        do, ds = self.empty((8, n)), self.empty((n,), np.uint8)
        self._call("sylow_hip_svdw_map_batch", du.ptr, do.ptr, ds.ptr, n)
        return self.from_device_soa(do), ds.download()

    def fp_compute_naf(self, k):
        """Fp::compute_naf on raw 256-bit values k [n, 4] -> (np [n, 4], nm [n, 4])."""
        k = _aos(k, 4)
        n = k.shape[0]
        dk = self.to_device_soa(k, 4)
        dp, dm = self.empty((4, n)), self.empty((4, n))
        self._call("sylow_hip_fp_compute_naf_batch", dk.ptr, dp.ptr, dm.ptr, n)
        return self.from_device_soa(dp), self.from_device_soa(dm)

    EXPANDERS = {"xmd_keccak256": 0, "xmd_sha256": 1, "xof_shake128": 2}     # SYLOW_HIP_EXPANDER_*

    @classmethod
    def _expander_id(cls, expander):
        return cls.EXPANDERS[expander] if isinstance(expander, str) else int(expander)

    def expand_message(self, msgs, length: int, expander=0, dst: bytes | None = None, k: int = 128):
        """Expander::expand_message under an RFC 9380 expander (a name of EXPANDERS or its id): uint8 [n, length]."""
        n = len(msgs)
        dm, doff = self._msgs(msgs)
        do = self.empty((n, max(length, 0)), np.uint8)
        self._call("sylow_hip_expand_message_batch", self._expander_id(expander), dm.ptr, doff.ptr, dst, len(dst) if dst else 0, k, length, do.ptr, n)
        return do.download()

    def hash_to_field(self, msgs, dst: bytes | None = None, expander=None, k: int = 128):
        n = len(msgs)
        dm, doff = self._msgs(msgs)
        do = self.empty((8, n))
        if expander is None:
            self._call("sylow_hip_hash_to_field_batch", dm.ptr, doff.ptr, dst, len(dst) if dst else 0, do.ptr, n)
        else:
            self._call("sylow_hip_hash_to_field_expander_batch", self._expander_id(expander), dm.ptr, doff.ptr, dst, len(dst) if dst else 0, k, do.ptr, n)
        return self.from_device_soa(do)

    def hash_to_g1(self, msgs, dst: bytes | None = None, expander=None, k: int = 128):
        n = len(msgs)
        dm, doff = self._msgs(msgs)
        do, doi = self.empty((8, n)), self.empty((n,), np.uint8)
        if expander is None:
            self._call("sylow_hip_hash_to_g1_batch", dm.ptr, doff.ptr, dst, len(dst) if dst else 0, do.ptr, doi.ptr, n)
        else:
            self._call("sylow_hip_hash_to_g1_expander_batch", self._expander_id(expander), dm.ptr, doff.ptr, dst, len(dst) if dst else 0, k, do.ptr, doi.ptr, n)
        return self.from_device_soa(do), doi.download()

    def bls_sign(self, sk, msgs, expander=None, dst: bytes | None = None, k: int = 128):
        sk = _aos(sk, 4)
        n = len(msgs)
        dm, doff = self._msgs(msgs)
        dsk = self.to_device_soa(sk, 4)
        do, doi = self.empty((8, n)), self.empty((n,), np.uint8)
        if expander is None and dst is None:
            self._call("sylow_hip_bls_sign_batch", dsk.ptr, dm.ptr, doff.ptr, do.ptr, doi.ptr, n)
        else:
            self._call("sylow_hip_bls_sign_expander_batch", self._expander_id(expander or 0), dst, len(dst) if dst else 0, k, dsk.ptr, dm.ptr, doff.ptr,
                       do.ptr, doi.ptr, n)
        return self.from_device_soa(do), doi.download()

    def bls_verify_hashed(self, pk_xy, h_xy, sig_xy, pk_inf=None, h_inf=None, sig_inf=None):
        """verify (lib.rs:223-236) on points H_i the caller hashed: ok_i = [ e(sig_i, G2gen) == e(H_i, pk_i) ]."""
        pk_xy, h_xy, sig_xy = _aos(pk_xy, 16), _aos(h_xy, 8), _aos(sig_xy, 8)
        n = h_xy.shape[0]
        dpk, dh, dsig = self.to_device_soa(pk_xy, 16), self.to_device_soa(h_xy, 8), self.to_device_soa(sig_xy, 8)
        dpi, dhi, dsi = self._flags(pk_inf, n), self._flags(h_inf, n), self._flags(sig_inf, n)
        dok = self.empty((n,), np.uint8)
        self._call("sylow_hip_bls_verify_hashed_batch", dpk.ptr, self._ptr(dpi), dh.ptr, self._ptr(dhi), dsig.ptr, self._ptr(dsi), dok.ptr, n)
        return dok.download()

    def bls_verify(self, pk_xy, msgs, sig_xy, pk_inf=None, sig_inf=None, fused=False, two_pairings=False, pipelined=True, chunk=0,
                   expander=None, dst: bytes | None = None, k: int = 128):
        """verify (lib.rs:223-236).  Default and `fused`: one final exponentiation per element; `two_pairings`: the literal form.
        The default form runs through the chunked host pipeline (sylow_hip_bls_verify_host) unless `pipelined=False`.
        `expander` / `dst`: H from another RFC 9380 suite (sylow_hip_bls_verify_expander_batch: one launch sequence, no host pipeline).
        `msgs`: a list of bytes, or a (blob uint8 array, offsets uint64 [n + 1]) pair."""
        pk_xy, sig_xy = _aos(pk_xy, 16), _aos(sig_xy, 8)
        if isinstance(msgs, tuple):
            blob, off = np.ascontiguousarray(msgs[0], dtype=np.uint8), np.ascontiguousarray(msgs[1], dtype=np.uint64)
            n = off.shape[0] - 1
        else:
            n = len(msgs)
            blob, off = None, None
        by_expander = expander is not None or dst is not None
        if by_expander and (fused or two_pairings):
            raise ValueError("bls_verify: expander / dst go with the default evaluation only")
        if pipelined and not two_pairings and not fused and not by_expander:
            if blob is None:
                blob = np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8)
                off = np.zeros(n + 1, dtype=np.uint64)
                if n:
                    off[1:] = np.cumsum([len(m) for m in msgs])
            ok = np.empty((n,), dtype=np.uint8)
            ki = None if pk_inf is None else np.ascontiguousarray(pk_inf, dtype=np.uint8).reshape(n)
            si = None if sig_inf is None else np.ascontiguousarray(sig_inf, dtype=np.uint8).reshape(n)
            _lib.check(self.lib.sylow_hip_set_device(self.device), "sylow_hip_set_device")
            _lib.check(self.lib.sylow_hip_bls_verify_host(pk_xy.ctypes.data, None if ki is None else ki.ctypes.data, blob.ctypes.data, off.ctypes.data,
                                                          sig_xy.ctypes.data, None if si is None else si.ctypes.data, ok.ctypes.data, n, chunk), "sylow_hip_bls_verify_host")
            return ok
        if blob is not None:
            msgs = [bytes(blob[int(off[i]):int(off[i + 1])]) for i in range(n)]
        dm, doff = self._msgs(msgs)
        dpk, dsig = self.to_device_soa(pk_xy, 16), self.to_device_soa(sig_xy, 8)
        dpi, dsi = self._flags(pk_inf, n), self._flags(sig_inf, n)
        dok = self.empty((n,), np.uint8)
        if by_expander:
            self._call("sylow_hip_bls_verify_expander_batch", self._expander_id(expander or 0), dst, len(dst) if dst else 0, k,
                       dpk.ptr, self._ptr(dpi), dm.ptr, doff.ptr, dsig.ptr, self._ptr(dsi), dok.ptr, n)
            return dok.download()
        name = "sylow_hip_bls_verify_two_pairings_batch" if two_pairings else "sylow_hip_bls_verify_fused_batch" if fused else "sylow_hip_bls_verify_batch"
        self._call(name, dpk.ptr, self._ptr(dpi), dm.ptr, doff.ptr, dsig.ptr, self._ptr(dsi), dok.ptr, n)
        return dok.download()

    @staticmethod
    def aggregate_shape_ok(n, n_pk):
        """The key-array shapes the aggregate entry points take for n (message, signature) rows (include/sylow_hip.h): one key, one key per
        row, committees (n_pk = c n: key j belongs to message j mod n) and key reuse (n = c n_pk, n_pk >= 2: row i is under key i mod n_pk)."""
        return n == 0 or n_pk in (1, n) or (n_pk > n and n_pk % n == 0) or (2 <= n_pk < n and n % n_pk == 0)

    def bls_aggregate_verify(self, pk_xy, msgs, sig_xy, pk_inf=None, sig_inf=None, comm=None):
        """One boolean for the whole batch: prod_i e(sig_i, G2gen) e(-H(msg_i), pk_i) == 1 (one key row = the same signer; c n key rows =
        committees of c keys, sig_i their aggregate signature; n / c key rows = keys reused with that period).  Returns (gt [48] words, is_one)."""
        pk_xy, sig_xy = _aos(pk_xy, 16), _aos(sig_xy, 8)
        n, n_pk = len(msgs), pk_xy.shape[0]
        assert sig_xy.shape[0] == n and self.aggregate_shape_ok(n, n_pk)
        dm, doff = self._msgs(msgs)
        dpk = self.to_device_soa(pk_xy, 16) if n_pk else None
        dsig = self.to_device_soa(sig_xy, 8) if n else None
        dpi, dsi = (self._flags(pk_inf, n_pk) if n_pk else None), (self._flags(sig_inf, n) if n else None)
        dgt, done = self.empty((48, 1)), self.empty((1,), np.uint8)
        self._call("sylow_hip_bls_aggregate_verify_batch", self._ptr(dpk), self._ptr(dpi), n_pk, dm.ptr, doff.ptr, self._ptr(dsig), self._ptr(dsi), n, comm, dgt.ptr, done.ptr)
        return self.from_device_soa(dgt)[0], int(done.download()[0])

    def bls_batch_verify_weighted(self, pk_xy, msgs, sig_xy, weights, pk_inf=None, sig_inf=None, comm=None):
        """The small-exponent batch test prod_i [e(sig_i, G2gen) e(-H(m_i), pk_i)]^(w_i) == identity (sound one-boolean batch
        verification); weights [n, 4] Fp values drawn by the caller after the signatures are fixed.  Returns (Gt words, bool)."""
        pk_xy, sig_xy, weights = _aos(pk_xy, 16), _aos(sig_xy, 8), _aos(weights, 4)
        n, n_pk = sig_xy.shape[0], pk_xy.shape[0]
        assert len(msgs) == n and weights.shape[0] == n and n_pk >= 1 and self.aggregate_shape_ok(n, n_pk)
        dpk, dsig, dw = self.to_device_soa(pk_xy, 16), self.to_device_soa(sig_xy, 8), self.to_device_soa(weights, 4)
        dm, doff = self._msgs(msgs)
        dpi, dsi = self._flags(pk_inf, n_pk), self._flags(sig_inf, n)
        dgt, dis = self.empty((48, 1)), self.empty((1,), np.uint8)
        self._call("sylow_hip_bls_batch_verify_weighted", dpk.ptr, self._ptr(dpi), n_pk, dm.ptr, doff.ptr, dsig.ptr, self._ptr(dsi), dw.ptr, n, comm, dgt.ptr, dis.ptr)
        return self.from_device_soa(dgt), bool(dis.download()[0])

    # ---- Groth16 under one verifying key.  vk = (alpha [1, 8], beta / gamma / delta [1, 16], ic [l + 1, 8]); inputs [n, l, 4]: any 256-bit
    # words, taken mod r ----
    def _groth16_vk(self, vk):
        alpha, beta, gamma, delta, ic = vk
        ic = _aos(ic, 8)
        assert ic.shape[0] >= 1
        return (self.to_device_soa(_aos(alpha, 8), 8), self.to_device_soa(_aos(beta, 16), 16), self.to_device_soa(_aos(gamma, 16), 16),
                self.to_device_soa(_aos(delta, 16), 16), self.to_device_soa(ic, 8), ic.shape[0] - 1)

    def _groth16_inputs(self, inputs, n, n_inputs):
        """[n, l, 4] (proof-major on the host) -> the device's input-major [4][l * n]"""
        inputs = np.ascontiguousarray(inputs, dtype=np.uint64).reshape(n, n_inputs, 4)
        if n == 0 or n_inputs == 0:
            return None
        return self.to_device_soa(np.ascontiguousarray(inputs.transpose(1, 0, 2)).reshape(n_inputs * n, 4), 4)

    def groth16_vk_x(self, ic, inputs):
        """vk_x_i = IC_0 + sum_j x_ij IC_j for every proof (sylow_hip_groth16_vk_x_batch): ([n, 8] affine words, [n] flags)."""
        ic = _aos(ic, 8)
        n_inputs = ic.shape[0] - 1
        n = np.asarray(inputs).shape[0]
        dic, dx = self.to_device_soa(ic, 8), self._groth16_inputs(inputs, n, n_inputs)
        do, doi = self.empty((8, max(n, 1))), self.empty((max(n, 1),), np.uint8)
        self._call("sylow_hip_groth16_vk_x_batch", dic.ptr, n_inputs, self._ptr(dx), n, do.ptr, doi.ptr)
        return self.from_device_soa(do)[:n], doi.download()[:n]

    def _groth16_proofs(self, a_xy, b_xy, c_xy, a_inf, b_inf, c_inf):
        a_xy, b_xy, c_xy = _aos(a_xy, 8), _aos(b_xy, 16), _aos(c_xy, 8)
        n = a_xy.shape[0]
        assert b_xy.shape[0] == n and c_xy.shape[0] == n
        up = lambda x, w: self.to_device_soa(x, w) if n else None
        fl = lambda x: self._flags(x, n) if n else None
        return n, up(a_xy, 8), fl(a_inf), up(b_xy, 16), fl(b_inf), up(c_xy, 8), fl(c_inf)

    def groth16_verify(self, vk, a_xy, b_xy, c_xy, inputs, a_inf=None, b_inf=None, c_inf=None):
        """e(-A_i, B_i) e(alpha, beta) e(vk_x_i, gamma) e(C_i, delta) == 1 for every proof under one verifying key
        (sylow_hip_groth16_verify_batch): [n] uint8.  Identities follow EIP-197; B, beta, gamma, delta must be in G2 proper."""
        dal, dbe, dga, dde, dic, n_inputs = self._groth16_vk(vk)
        n, da, dai, db, dbi, dc, dci = self._groth16_proofs(a_xy, b_xy, c_xy, a_inf, b_inf, c_inf)
        dx = self._groth16_inputs(inputs, n, n_inputs)
        dok = self.empty((max(n, 1),), np.uint8)
        self._call("sylow_hip_groth16_verify_batch", dal.ptr, dbe.ptr, dga.ptr, dde.ptr, dic.ptr, n_inputs, self._ptr(da), self._ptr(dai), self._ptr(db),
                   self._ptr(dbi), self._ptr(dc), self._ptr(dci), self._ptr(dx), n, dok.ptr)
        return dok.download()[:n]

    def groth16_batch_verify_weighted(self, vk, a_xy, b_xy, c_xy, inputs, weights, a_inf=None, b_inf=None, c_inf=None):
        """The small-exponent batch test of n Groth16 proofs as ONE Gt (sylow_hip_groth16_batch_verify_weighted); weights [n, 4] drawn by the
        caller after the proofs are fixed (any 256-bit words, taken mod r; 0 removes a proof).  Returns (Gt words [1, 48], bool)."""
        dal, dbe, dga, dde, dic, n_inputs = self._groth16_vk(vk)
        n, da, dai, db, dbi, dc, dci = self._groth16_proofs(a_xy, b_xy, c_xy, a_inf, b_inf, c_inf)
        dx = self._groth16_inputs(inputs, n, n_inputs)
        weights = _aos(weights, 4)
        assert weights.shape[0] == n
        dw = self.to_device_soa(weights, 4) if n else None
        dgt, dis = self.empty((48, 1)), self.empty((1,), np.uint8)
        self._call("sylow_hip_groth16_batch_verify_weighted", dal.ptr, dbe.ptr, dga.ptr, dde.ptr, dic.ptr, n_inputs, self._ptr(da), self._ptr(dai), self._ptr(db),
                   self._ptr(dbi), self._ptr(dc), self._ptr(dci), self._ptr(dx), self._ptr(dw), n, dgt.ptr, dis.ptr)
        return self.from_device_soa(dgt), bool(dis.download()[0])

    # ---- KZG openings under one SRS.  tau_g2 [1, 16]; an opening is (C [8], z [4], y [4], pi [8]); z, y and weights: any 256-bit words,
    # taken mod r ----
    def _kzg_openings(self, c_xy, z, y, pi_xy, c_inf, pi_inf):
        c_xy, z, y, pi_xy = _aos(c_xy, 8), _aos(z, 4), _aos(y, 4), _aos(pi_xy, 8)
        n = c_xy.shape[0]
        assert z.shape[0] == n and y.shape[0] == n and pi_xy.shape[0] == n
        up = lambda x, w: self.to_device_soa(x, w) if n else None
        fl = lambda x: self._flags(x, n) if n else None
        return n, (up(c_xy, 8), fl(c_inf), up(z, 4), up(y, 4), up(pi_xy, 8), fl(pi_inf))      # the caller holds them across its call

    def kzg_fold(self, c_xy, z, y, pi_xy, c_inf=None, pi_inf=None):
        """F_i = C_i - y_i G1gen + z_i pi_i for every opening (sylow_hip_kzg_fold_batch): ([n, 8] affine words, [n] flags)."""
        n, d = self._kzg_openings(c_xy, z, y, pi_xy, c_inf, pi_inf)
        args = [self._ptr(x) for x in d]
        do, doi = self.empty((8, max(n, 1))), self.empty((max(n, 1),), np.uint8)
        self._call("sylow_hip_kzg_fold_batch", *args, do.ptr, doi.ptr, n)
        return self.from_device_soa(do)[:n], doi.download()[:n]

    def kzg_verify(self, tau_g2, c_xy, z, y, pi_xy, c_inf=None, pi_inf=None):
        """e(C_i - y_i G1gen + z_i pi_i, G2gen) e(-pi_i, tau_g2) == 1 for every opening under one SRS (sylow_hip_kzg_verify_batch): [n]
        uint8.  Identities follow EIP-197; tau_g2 must be in G2 proper."""
        tau_g2 = _aos(tau_g2, 16)
        assert tau_g2.shape[0] == 1
        dtau = self.to_device_soa(tau_g2, 16)
        n, d = self._kzg_openings(c_xy, z, y, pi_xy, c_inf, pi_inf)
        args = [self._ptr(x) for x in d]
        dok = self.empty((max(n, 1),), np.uint8)
        self._call("sylow_hip_kzg_verify_batch", dtau.ptr, *args, dok.ptr, n)
        return dok.download()[:n]

    def kzg_verify_line_table(self, table: DeviceArray, c_xy, z, y, pi_xy, c_inf=None, pi_inf=None):
        """The same against a line table of tau_g2 cached with g2_line_table (sylow_hip_kzg_verify_line_table_batch)."""
        n, d = self._kzg_openings(c_xy, z, y, pi_xy, c_inf, pi_inf)
        args = [self._ptr(x) for x in d]
        dok = self.empty((max(n, 1),), np.uint8)
        self._call("sylow_hip_kzg_verify_line_table_batch", table.ptr, *args, dok.ptr, n)
        return dok.download()[:n]

    def kzg_batch_verify_weighted(self, tau_g2, c_xy, z, y, pi_xy, weights, c_inf=None, pi_inf=None):
        """The small-exponent batch test of n KZG openings as ONE Gt (sylow_hip_kzg_batch_verify_weighted); weights [n, 4] drawn by the
        caller after the openings are fixed (any 256-bit words, taken mod r; 0 removes an opening).  Returns (Gt words [1, 48], bool)."""
        tau_g2 = _aos(tau_g2, 16)
        assert tau_g2.shape[0] == 1
        dtau = self.to_device_soa(tau_g2, 16)
        n, d = self._kzg_openings(c_xy, z, y, pi_xy, c_inf, pi_inf)
        args = [self._ptr(x) for x in d]
        weights = _aos(weights, 4)
        assert weights.shape[0] == n
        dw = self.to_device_soa(weights, 4) if n else None
        dgt, dis = self.empty((48, 1)), self.empty((1,), np.uint8)
        self._call("sylow_hip_kzg_batch_verify_weighted", dtau.ptr, *args, self._ptr(dw), n, dgt.ptr, dis.ptr)
        return self.from_device_soa(dgt), bool(dis.download()[0])

    # ---- KZG, the prover's side.  polys [m, len, 4]: m polynomials of len coefficients, lowest degree first, any 256-bit words taken mod r;
    # srs_g1 [len, 8]: tau^k G1gen, k = 0 .. len - 1; z [m, 4].  The device layout is [m][4][len] (include/sylow_hip.h) ----
    @staticmethod
    def _kzg_polys(polys):
        a = np.ascontiguousarray(polys, dtype=np.uint64)
        assert a.ndim == 3 and a.shape[2] == 4 and a.shape[1] >= 1, a.shape
        return a

    def _kzg_polys_up(self, a):
        return self.to_device(np.ascontiguousarray(a.transpose(0, 2, 1))) if a.shape[0] else None

    def kzg_quotient(self, polys, z, want_q=True, want_y=True):
        """q_j = (f_j - f_j(z_j)) / (X - z_j) as [m, len, 4] canonical words (q[len - 1] = 0) and y_j = f_j(z_j) as [m, 4]
        (sylow_hip_kzg_quotient_batch); an output that is not wanted is None (want_q = False is plain evaluation)."""
        a, z = self._kzg_polys(polys), _aos(z, 4)
        m, ln = a.shape[0], a.shape[1]
        assert z.shape[0] == m and (want_q or want_y)
        dc, dz = self._kzg_polys_up(a), (self.to_device_soa(z, 4) if m else None)
        dq = self.empty((max(m, 1), 4, ln)) if want_q else None
        dy = self.empty((4, max(m, 1))) if want_y else None
        self._call("sylow_hip_kzg_quotient_batch", self._ptr(dc), ln, m, self._ptr(dz), self._ptr(dq), self._ptr(dy))
        q = np.ascontiguousarray(dq.download()[:m].transpose(0, 2, 1)) if want_q else None
        return q, (self.from_device_soa(dy)[:m] if want_y else None)

    def kzg_commit(self, srs_g1, polys, window=-1, min_len=-1):
        """C_j = sum_k f_jk srs_k for every polynomial (sylow_hip_kzg_commit_batch): ([m, 8] affine words, [m] flags).  window / min_len >= 0 pin
        the plan (sylow_hip_kzg_commit_batch_tuned: the bucket route's window width, the smallest len that takes it); the points do not
        depend on them."""
        a, srs = self._kzg_polys(polys), _aos(srs_g1, 8)
        m, ln = a.shape[0], a.shape[1]
        assert srs.shape[0] == ln
        dc, ds = self._kzg_polys_up(a), self.to_device_soa(srs, 8)
        do, doi = self.empty((8, max(m, 1))), self.empty((max(m, 1),), np.uint8)
        if window < 0 and min_len < 0:
            self._call("sylow_hip_kzg_commit_batch", ds.ptr, self._ptr(dc), ln, m, do.ptr, doi.ptr)
        else:
            self._call("sylow_hip_kzg_commit_batch_tuned", ds.ptr, self._ptr(dc), ln, m, int(window), int(min_len), do.ptr, doi.ptr)
        return self.from_device_soa(do)[:m], doi.download()[:m]

    def kzg_open(self, srs_g1, polys, z):
        """The opening of every f_j at z_j (sylow_hip_kzg_open_batch): (y [m, 4], pi [m, 8] affine words, pi flags [m]); pi_j is the identity
        exactly when f_j is constant."""
        a, srs, z = self._kzg_polys(polys), _aos(srs_g1, 8), _aos(z, 4)
        m, ln = a.shape[0], a.shape[1]
        assert srs.shape[0] == ln and z.shape[0] == m
        dc, ds, dz = self._kzg_polys_up(a), self.to_device_soa(srs, 8), (self.to_device_soa(z, 4) if m else None)
        dy, dp, dpi = self.empty((4, max(m, 1))), self.empty((8, max(m, 1))), self.empty((max(m, 1),), np.uint8)
        self._call("sylow_hip_kzg_open_batch", ds.ptr, self._ptr(dc), ln, m, self._ptr(dz), dy.ptr, dp.ptr, dpi.ptr)
        return self.from_device_soa(dy)[:m], self.from_device_soa(dp)[:m], dpi.download()[:m]

    def kzg_commit_evals(self, srs_g1, evals):
        """C_j for m polynomials given by their values on the domain of n = 2^log_n points, evals [m, n, 4] with evals[j, i] = f_j(w_n^i)
        (sylow_hip_kzg_commit_evals_batch: the inverse transform into scratch, then the commitment): ([m, 8] affine words, [m] flags)."""
        a, srs = self._kzg_polys(evals), _aos(srs_g1, 8)
        m, n = a.shape[0], a.shape[1]
        log_n = n.bit_length() - 1
        assert n == 1 << log_n and srs.shape[0] == n, (n, srs.shape)
        dc, ds = self._kzg_polys_up(a), self.to_device_soa(srs, 8)
        do, doi = self.empty((8, max(m, 1))), self.empty((max(m, 1),), np.uint8)
        self._call("sylow_hip_kzg_commit_evals_batch", ds.ptr, self._ptr(dc), log_n, m, do.ptr, doi.ptr)
        return self.from_device_soa(do)[:m], doi.download()[:m]

    # ---- KZG from evaluations.  evals [m, n, 4]: evals[j, i] = f_j(w_n^i), n = 2^log_n <= 2^28, any 256-bit words taken mod r;
    # srs_lagrange [n, 8]: L_i(tau) G1gen for the Lagrange basis of the same domain; z [m, 4] ----
    def _kzg_evals(self, evals):
        a = self._kzg_polys(evals)
        n = a.shape[1]
        log_n = n.bit_length() - 1
        assert n == 1 << log_n, n
        return a, a.shape[0], n, log_n

    def kzg_quotient_evals(self, evals, z, want_q=True, want_y=True):
        """y_j = f_j(z_j) as [m, 4] and the values on the domain of q_j = (f_j - y_j) / (X - z_j) as [m, n, 4] canonical words
        (sylow_hip_kzg_quotient_evals_batch; z_j inside the domain: q_j[k] = f_j'(w^k)); an output that is not wanted is None (want_q = False
        is barycentric evaluation alone)."""
        (a, m, n, log_n), z = self._kzg_evals(evals), _aos(z, 4)
        assert z.shape[0] == m and (want_q or want_y)
        dc, dz = self._kzg_polys_up(a), (self.to_device_soa(z, 4) if m else None)
        dq = self.empty((max(m, 1), 4, n)) if want_q else None
        dy = self.empty((4, max(m, 1))) if want_y else None
        self._call("sylow_hip_kzg_quotient_evals_batch", self._ptr(dc), log_n, m, self._ptr(dz), self._ptr(dq), self._ptr(dy))
        q = np.ascontiguousarray(dq.download()[:m].transpose(0, 2, 1)) if want_q else None
        return q, (self.from_device_soa(dy)[:m] if want_y else None)

    def kzg_open_evals(self, srs_lagrange, evals, z):
        """The opening of every f_j at z_j from its values under the Lagrange-basis SRS (sylow_hip_kzg_open_evals_batch): (y [m, 4], pi [m, 8]
        affine words, pi flags [m]); pi_j is the identity exactly when f_j is constant."""
        (a, m, n, log_n), srs, z = self._kzg_evals(evals), _aos(srs_lagrange, 8), _aos(z, 4)
        assert srs.shape[0] == n and z.shape[0] == m
        dc, ds, dz = self._kzg_polys_up(a), self.to_device_soa(srs, 8), (self.to_device_soa(z, 4) if m else None)
        dy, dp, dpi = self.empty((4, max(m, 1))), self.empty((8, max(m, 1))), self.empty((max(m, 1),), np.uint8)
        self._call("sylow_hip_kzg_open_evals_batch", ds.ptr, self._ptr(dc), log_n, m, self._ptr(dz), dy.ptr, dp.ptr, dpi.ptr)
        return self.from_device_soa(dy)[:m], self.from_device_soa(dp)[:m], dpi.download()[:m]

    # ---- KZG, folded openings.  groups: the G + 1 OFFSETS of the groups of consecutive polynomials (0 .. m, non-decreasing; a host array, read
    # before the call returns); z, gamma [G, 4]; the polynomials as in the prover's calls above ----
    @staticmethod
    def _kzg_groups(groups, m):
        gs = np.ascontiguousarray([int(x) for x in groups], dtype=np.uint64)
        if gs.ndim != 1 or gs.size < 1 or int(gs[0]) != 0 or int(gs[-1]) != m or (gs[1:] < gs[:-1]).any():
            raise ValueError(f"groups: G + 1 non-decreasing offsets from 0 to m = {m}")
        return gs, gs.size - 1

    def fr_lincomb(self, a, weights, groups):
        """out_g = sum_{j in group g} weights_j a_j over Fr for a [m, len, 4] and weights [m, 4]: [G, len, 4] canonical words
        (sylow_hip_fr_lincomb_batch); an empty group gives zeros."""
        a, w = self._kzg_polys(a), _aos(weights, 4)
        m, ln = a.shape[0], a.shape[1]
        gs, G = self._kzg_groups(groups, m)
        assert w.shape[0] == m
        if not m or not G:
            return np.zeros((G, ln, 4), dtype=np.uint64)
        da, dw, do = self._kzg_polys_up(a), self.to_device_soa(w, 4), self.empty((G, 4, ln))
        self._call("sylow_hip_fr_lincomb_batch", da.ptr, ln, m, dw.ptr, gs.ctypes.data, G, do.ptr)
        return np.ascontiguousarray(do.download().transpose(0, 2, 1))

    def fr_group_powers(self, gamma, groups, m):
        """[m, 4] words: gamma_g^i for polynomial i of group g (sylow_hip_fr_group_powers_batch); 0^0 = 1."""
        gamma = _aos(gamma, 4)
        gs, G = self._kzg_groups(groups, m)
        assert gamma.shape[0] == G
        if not m or not G:
            return np.zeros((m, 4), dtype=np.uint64)
        dg, do = self.to_device_soa(gamma, 4), self.empty((4, m))
        self._call("sylow_hip_fr_group_powers_batch", dg.ptr, gs.ctypes.data, G, m, do.ptr)
        return self.from_device_soa(do)

    def _kzg_open_multi(self, name, srs, a, size_arg, groups, z, gamma):
        srs, z, gamma = _aos(srs, 8), _aos(z, 4), _aos(gamma, 4)
        m, ln = a.shape[0], a.shape[1]
        gs, G = self._kzg_groups(groups, m)
        assert srs.shape[0] == ln and z.shape[0] == G and gamma.shape[0] == G
        identity = np.zeros((G, 8), dtype=np.uint64)
        identity[:, 4] = 1
        if not m or not G:                                     # the empty batch: every group is empty
            return np.zeros((m, 4), dtype=np.uint64), identity, np.ones(G, dtype=np.uint8)
        dc, ds, dz, dg = self._kzg_polys_up(a), self.to_device_soa(srs, 8), self.to_device_soa(z, 4), self.to_device_soa(gamma, 4)
        dy, dp, dpi = self.empty((4, m)), self.empty((8, G)), self.empty((G,), np.uint8)
        self._call(name, ds.ptr, dc.ptr, size_arg, m, gs.ctypes.data, G, dz.ptr, dg.ptr, dy.ptr, dp.ptr, dpi.ptr)
        return self.from_device_soa(dy), self.from_device_soa(dp), dpi.download()

    def kzg_open_multi(self, srs_g1, polys, groups, z, gamma):
        """Every group of polynomials opened at z_g under ONE proof folded with gamma_g (sylow_hip_kzg_open_multi_batch): (y [m, 4] with
        y_j = f_j(z_g), pi [G, 8] affine words, pi flags [G]); pi_g is word for word kzg_open of F_g = sum_j gamma_g^i f_j."""
        a = self._kzg_polys(polys)
        return self._kzg_open_multi("sylow_hip_kzg_open_multi_batch", srs_g1, a, a.shape[1], groups, z, gamma)

    def kzg_open_multi_evals(self, srs_lagrange, evals, groups, z, gamma):
        """The same from evaluation form under the Lagrange-basis SRS (sylow_hip_kzg_open_multi_evals_batch)."""
        a, m, n, log_n = self._kzg_evals(evals)
        return self._kzg_open_multi("sylow_hip_kzg_open_multi_evals_batch", srs_lagrange, a, log_n, groups, z, gamma)

    def _kzg_combine_args(self, c_xy, c_inf, y, groups, gamma):
        c_xy, y, gamma = _aos(c_xy, 8), _aos(y, 4), _aos(gamma, 4)
        m = c_xy.shape[0]
        gs, G = self._kzg_groups(groups, m)
        assert y.shape[0] == m and gamma.shape[0] == G
        up = lambda x, w: self.to_device_soa(x, w) if x.shape[0] else None
        return m, gs, G, (up(c_xy, 8), self._flags(c_inf, m) if m else None, up(y, 4), up(gamma, 4))

    def kzg_combine_openings(self, c_xy, y, groups, gamma, c_inf=None):
        """The verifier's folded rows (sylow_hip_kzg_combine_openings_batch): (C_F [G, 8] affine words, C_F flags [G], y_F [G, 4]) with
        C_F,g = sum_j gamma_g^i C_j and y_F,g = sum_j gamma_g^i y_j; an empty group gives the identity and 0."""
        m, gs, G, (dc, dci, dy, dg) = self._kzg_combine_args(c_xy, c_inf, y, groups, gamma)
        if not m or not G:
            identity = np.zeros((G, 8), dtype=np.uint64)
            identity[:, 4] = 1
            return identity, np.ones(G, dtype=np.uint8), np.zeros((G, 4), dtype=np.uint64)
        dcf, dcfi, dyf = self.empty((8, G)), self.empty((G,), np.uint8), self.empty((4, G))
        self._call("sylow_hip_kzg_combine_openings_batch", dc.ptr, self._ptr(dci), dy.ptr, m, gs.ctypes.data, G, dg.ptr, dcf.ptr, dcfi.ptr, dyf.ptr)
        return self.from_device_soa(dcf), dcfi.download(), self.from_device_soa(dyf)

    def kzg_verify_multi(self, tau_g2, c_xy, y, groups, z, gamma, pi_xy, c_inf=None, pi_inf=None):
        """ok [G]: the folded row (C_F,g, z_g, y_F,g, pi_g) of every group checked under tau_g2 (sylow_hip_kzg_verify_multi_batch).  An empty
        batch (m = 0) returns no flags."""
        tau_g2, z, pi_xy = _aos(tau_g2, 16), _aos(z, 4), _aos(pi_xy, 8)
        m, gs, G, (dc, dci, dy, dg) = self._kzg_combine_args(c_xy, c_inf, y, groups, gamma)
        assert tau_g2.shape[0] == 1 and z.shape[0] == G and pi_xy.shape[0] == G
        if not m or not G:
            return np.zeros(0, dtype=np.uint8)
        dtau, dz, dp, dpi, dok = self.to_device_soa(tau_g2, 16), self.to_device_soa(z, 4), self.to_device_soa(pi_xy, 8), self._flags(pi_inf, G), self.empty((G,), np.uint8)
        self._call("sylow_hip_kzg_verify_multi_batch", dtau.ptr, dc.ptr, self._ptr(dci), dy.ptr, m, gs.ctypes.data, G, dz.ptr, dg.ptr, dp.ptr, self._ptr(dpi), dok.ptr)
        return dok.download()

    # ---- KZG, one polynomial at several points under one proof (include/sylow_hip_kzg_points.h).  z, y [m, k, 4]: k points per row,
    # 1 <= k <= 64, any 256-bit words taken mod r; the device layout is [4][m k] with (row j, point i) at j k + i.  The library draws no
    # challenge and takes the SRS as given ----
    @staticmethod
    def _kzg_rows(z):
        z = np.ascontiguousarray(z, dtype=np.uint64)
        assert z.ndim == 3 and z.shape[2] == 4 and z.shape[1] >= 1, z.shape
        return z

    def _kzg_rows_up(self, z):
        return self.to_device_soa(z.reshape(-1, 4), 4) if z.shape[0] else None

    def _kzg_rows_down(self, d, m, k):
        return self.from_device_soa(d)[:m * k].reshape(m, k, 4)

    def kzg_points_weights(self, z):
        """The barycentric weights a[j, i] = 1 / prod_{l != i} (z[j, i] - z[j, l]) as [m, k, 4] canonical words, inv(0) = 0, and distinct [m]:
        1 iff the k points of row j are distinct mod r (sylow_hip_kzg_points_weights_batch)."""
        z = self._kzg_rows(z)
        m, k = z.shape[0], z.shape[1]
        dz, da, dd = self._kzg_rows_up(z), self.empty((4, max(m * k, 1))), self.empty((max(m, 1),), np.uint8)
        self._call("sylow_hip_kzg_points_weights_batch", self._ptr(dz), k, m, da.ptr, dd.ptr)
        return self._kzg_rows_down(da, m, k), dd.download()[:m]

    def kzg_quotient_points(self, polys, z, want_q=True, want_y=True):
        """q_j = sum_i a[j, i] (f_j - f_j(z[j, i])) / (X - z[j, i]) as [m, len, 4] canonical words -- f_j div prod_i (X - z[j, i]) for
        distinct points -- and y[j, i] = f_j(z[j, i]) as [m, k, 4] (sylow_hip_kzg_quotient_points_batch); an output that is not wanted is
        None.  A row with points repeated mod r gives what the formula gives under inv(0) = 0: not a valid opening."""
        a, z = self._kzg_polys(polys), self._kzg_rows(z)
        m, ln, k = a.shape[0], a.shape[1], z.shape[1]
        assert z.shape[0] == m and (want_q or want_y)
        dc, dz = self._kzg_polys_up(a), self._kzg_rows_up(z)
        dq = self.empty((max(m, 1), 4, ln)) if want_q else None
        dy = self.empty((4, max(m * k, 1))) if want_y else None
        self._call("sylow_hip_kzg_quotient_points_batch", self._ptr(dc), ln, m, self._ptr(dz), k, self._ptr(dq), self._ptr(dy))
        q = np.ascontiguousarray(dq.download()[:m].transpose(0, 2, 1)) if want_q else None
        return q, (self._kzg_rows_down(dy, m, k) if want_y else None)

    def kzg_open_points(self, srs_g1, polys, z):
        """The opening of every f_j at its k points under ONE proof (sylow_hip_kzg_open_points_batch): (y [m, k, 4], pi [m, 8] affine words,
        pi flags [m]); pi_j is the identity exactly when the quotient is zero (len <= k, or f_j of degree below k)."""
        a, srs, z = self._kzg_polys(polys), _aos(srs_g1, 8), self._kzg_rows(z)
        m, ln, k = a.shape[0], a.shape[1], z.shape[1]
        assert srs.shape[0] == ln and z.shape[0] == m
        dc, ds, dz = self._kzg_polys_up(a), self.to_device_soa(srs, 8), self._kzg_rows_up(z)
        dy, dp, dpi = self.empty((4, max(m * k, 1))), self.empty((8, max(m, 1))), self.empty((max(m, 1),), np.uint8)
        self._call("sylow_hip_kzg_open_points_batch", ds.ptr, self._ptr(dc), ln, m, self._ptr(dz), k, dy.ptr, dp.ptr, dpi.ptr)
        return self._kzg_rows_down(dy, m, k), self.from_device_soa(dp)[:m], dpi.download()[:m]

    def kzg_points_polys(self, z, y):
        """The verifier's Fr half (sylow_hip_kzg_points_polys_batch): (Z [n, k + 1, 4] with Z_j = prod_i (X - z[j, i]), monic,
        R [n, k, 4] with R_j the interpolant of the y[j, i] at the z[j, i], distinct [n]); coefficients lowest degree first."""
        z, y = self._kzg_rows(z), self._kzg_rows(y)
        n, k = z.shape[0], z.shape[1]
        assert y.shape == z.shape
        dz, dy = self._kzg_rows_up(z), self._kzg_rows_up(y)
        dzp, drp, dd = self.empty((max(n, 1), 4, k + 1)), self.empty((max(n, 1), 4, k)), self.empty((max(n, 1),), np.uint8)
        self._call("sylow_hip_kzg_points_polys_batch", self._ptr(dz), self._ptr(dy), k, n, dzp.ptr, drp.ptr, dd.ptr)
        return (np.ascontiguousarray(dzp.download()[:n].transpose(0, 2, 1)), np.ascontiguousarray(drp.download()[:n].transpose(0, 2, 1)),
                dd.download()[:n])

    def kzg_verify_points(self, srs_g1, srs_g2, c_xy, z, y, pi_xy, c_inf=None, pi_inf=None):
        """ok [n]: e(C_j - R_j(tau) G1gen, G2gen) e(-pi_j, Z_j(tau) G2gen) == 1 and the points of row j distinct mod r
        (sylow_hip_kzg_verify_points_batch).  srs_g1 [k, 8] = tau^i G1gen, i < k; srs_g2 [k + 1, 16] = tau^i G2gen, i <= k: the verifier's
        key, taken as given."""
        srs_g1, srs_g2, c_xy, pi_xy = _aos(srs_g1, 8), _aos(srs_g2, 16), _aos(c_xy, 8), _aos(pi_xy, 8)
        z, y = self._kzg_rows(z), self._kzg_rows(y)
        n, k = z.shape[0], z.shape[1]
        assert y.shape == z.shape and c_xy.shape[0] == n and pi_xy.shape[0] == n and srs_g1.shape[0] == k and srs_g2.shape[0] == k + 1
        if not n:
            return np.zeros(0, dtype=np.uint8)
        d1, d2, dc, dp = self.to_device_soa(srs_g1, 8), self.to_device_soa(srs_g2, 16), self.to_device_soa(c_xy, 8), self.to_device_soa(pi_xy, 8)
        dci, dpi, dz, dy, dok = self._flags(c_inf, n), self._flags(pi_inf, n), self._kzg_rows_up(z), self._kzg_rows_up(y), self.empty((n,), np.uint8)
        self._call("sylow_hip_kzg_verify_points_batch", d1.ptr, d2.ptr, dc.ptr, self._ptr(dci), dz.ptr, dy.ptr, k, n, dp.ptr, self._ptr(dpi), dok.ptr)
        return dok.download()

    # ---- Fr transforms on radix-2 domains.  values [m, n, 4] (or [n, 4]: one array), n = 2^log_n <= 2^28, any 256-bit words taken mod r ----
    def fr_ntt(self, values, inverse=False, shift=None, stages=-1):
        """forward: out_i = sum_k a_k (g w_n^i)^k; inverse: out_k = n^-1 g^-k sum_i a_i w_n^(-ik), natural order both ways, per array
        (sylow_hip_fr_ntt_batch).  shift: the coset shift g as [4] words (None: 1).  stages >= 1 pins the stages of a pass
        (sylow_hip_fr_ntt_batch_tuned); the values do not depend on it.  Canonical words in the shape of `values`."""
        a = np.ascontiguousarray(values, dtype=np.uint64)
        one = a.ndim == 2
        a = self._kzg_polys(a[None] if one else a)
        m, n = a.shape[0], a.shape[1]
        log_n = n.bit_length() - 1
        assert n == 1 << log_n, n
        din = self._kzg_polys_up(a)
        dsh = None if shift is None else self.to_device(np.ascontiguousarray(shift, dtype=np.uint64).reshape(4))
        dout = self.empty((max(m, 1), 4, n))
        if stages < 0:
            self._call("sylow_hip_fr_ntt_batch", self._ptr(din), log_n, m, int(bool(inverse)), self._ptr(dsh), dout.ptr)
        else:
            self._call("sylow_hip_fr_ntt_batch_tuned", self._ptr(din), log_n, m, int(bool(inverse)), self._ptr(dsh), int(stages), dout.ptr)
        out = np.ascontiguousarray(dout.download()[:m].transpose(0, 2, 1))
        return out[0] if one else out

    # ---- G1 transforms on radix-2 domains.  xy [m, n, 8] (or [n, 8]: one array) affine words, inf [m, n] (or [n]) flags or None, n = 2^log_n ----
    def g1_ntt(self, xy, inf=None, inverse=False, max_blocks=-1):
        """forward: out_i = sum_k w_n^(ik) P_k; inverse: out_k = n^-1 sum_i w_n^(-ik) P_i, natural order both ways, per array
        (sylow_hip_g1_ntt_batch).  max_blocks >= 1 caps the blocks of a stage launch (sylow_hip_g1_ntt_batch_tuned); the points do not depend
        on it.  (canonical affine words in the shape of `xy`, flags), the identity as (0, 1) + its flag."""
        a = np.ascontiguousarray(xy, dtype=np.uint64)
        one = a.ndim == 2
        a = a[None] if one else a
        assert a.ndim == 3 and a.shape[2] == 8 and a.shape[1] >= 1, a.shape
        m, n = a.shape[0], a.shape[1]
        log_n = n.bit_length() - 1
        assert n == 1 << log_n, n
        din = self.to_device(np.ascontiguousarray(a.transpose(0, 2, 1))) if m else None
        dinf = None if inf is None or not m else self.to_device(np.ascontiguousarray(inf, dtype=np.uint8).reshape(m, n))
        do, doi = self.empty((max(m, 1), 8, n)), self.empty((max(m, 1), n), np.uint8)
        if max_blocks < 0:
            self._call("sylow_hip_g1_ntt_batch", self._ptr(din), self._ptr(dinf), log_n, m, int(bool(inverse)), do.ptr, doi.ptr)
        else:
            self._call("sylow_hip_g1_ntt_batch_tuned", self._ptr(din), self._ptr(dinf), log_n, m, int(bool(inverse)), int(max_blocks), do.ptr, doi.ptr)
        out, flags = np.ascontiguousarray(do.download()[:m].transpose(0, 2, 1)), doi.download()[:m]
        return (out[0], flags[0]) if one else (out, flags)

    def kzg_srs_lagrange(self, xy):
        """The Lagrange-basis SRS L_i(tau) G1gen from the monomial one, xy [n, 8] = tau^k G1gen, n = 2^log_n (sylow_hip_kzg_srs_lagrange):
        ([n, 8] affine words, [n] flags); a set flag means tau lies in the domain."""
        srs = _aos(xy, 8)
        n = srs.shape[0]
        log_n = n.bit_length() - 1
        assert n >= 1 and n == 1 << log_n, n
        ds, do, doi = self.to_device_soa(srs, 8), self.empty((8, n)), self.empty((n,), np.uint8)
        self._call("sylow_hip_kzg_srs_lagrange", ds.ptr, log_n, do.ptr, doi.ptr)
        return self.from_device_soa(do), doi.download()

    # ---- KZG proofs at every point of the domain.  The table T is kept ON THE DEVICE: (DeviceArray [8, 2n] words, DeviceArray [2n] flags) ----
    def kzg_open_all_prepare(self, srs_g1):
        """The table of kzg_open_all from the monomial SRS, srs_g1 [n, 8] = tau^k G1gen, n = 2^log_n <= 2^27 (sylow_hip_kzg_open_all_prepare):
        the forward G1 transform of 2n points, x_(2n-1-t) = s_t for t <= n - 2 and the identity elsewhere.  Device arrays ([8, 2n] words,
        [2n] flags), built once per SRS; a set flag is an entry that is the identity, not an error."""
        srs = _aos(srs_g1, 8)
        n = srs.shape[0]
        log_n = n.bit_length() - 1
        assert n >= 1 and n == 1 << log_n, n
        ds, dt, dti = self.to_device_soa(srs, 8), self.empty((8, 2 * n)), self.empty((2 * n,), np.uint8)
        self._call("sylow_hip_kzg_open_all_prepare", ds.ptr, log_n, dt.ptr, dti.ptr)
        self.sync()                      # ds is released when this frame returns
        return dt, dti

    def kzg_open_all(self, table, polys, max_blocks=-1, want_y=True):
        """The proofs of every f_j at ALL n points w_n^i of its domain and its values there (sylow_hip_kzg_open_all_batch): (y [m, n, 4] or
        None, pi [m, n, 8] affine words, pi flags [m, n]).  table: what kzg_open_all_prepare returned, or host arrays ([2n, 8] words,
        [2n] flags or None).  polys [m, n, 4].  max_blocks >= 1 caps the blocks of a multiplying launch (sylow_hip_kzg_open_all_batch_tuned);
        the values do not depend on it."""
        a = self._kzg_polys(polys)
        m, n = a.shape[0], a.shape[1]
        log_n = n.bit_length() - 1
        assert n == 1 << log_n, n
        txy, tinf = table
        dt = txy if isinstance(txy, DeviceArray) else self.to_device_soa(_aos(txy, 8), 8)
        dti = tinf if tinf is None or isinstance(tinf, DeviceArray) else self.to_device(np.ascontiguousarray(tinf, dtype=np.uint8).reshape(-1))
        assert dt.shape == (8, 2 * n) and (dti is None or dti.shape == (2 * n,)), (dt.shape, n)
        dc = self._kzg_polys_up(a)
        dy = self.empty((max(m, 1), 4, n)) if want_y else None
        dp, dpi = self.empty((max(m, 1), 8, n)), self.empty((max(m, 1), n), np.uint8)
        if max_blocks < 0:
            self._call("sylow_hip_kzg_open_all_batch", dt.ptr, self._ptr(dti), self._ptr(dc), log_n, m, self._ptr(dy), dp.ptr, dpi.ptr)
        else:
            self._call("sylow_hip_kzg_open_all_batch_tuned", dt.ptr, self._ptr(dti), self._ptr(dc), log_n, m, int(max_blocks), self._ptr(dy), dp.ptr, dpi.ptr)
        y = np.ascontiguousarray(dy.download()[:m].transpose(0, 2, 1)) if want_y else None
        return y, np.ascontiguousarray(dp.download()[:m].transpose(0, 2, 1)), dpi.download()[:m]

    # ---- KZG proofs on every coset of the domain (include/sylow_hip_kzg_cosets.h): n = c l, c = 2^log_c cosets of l = 2^log_l points.  The
    # table is kept ON THE DEVICE: (DeviceArray [l, 8, 2c] words, DeviceArray [l, 2c] flags) ----
    def kzg_open_cosets_prepare(self, srs_g1, log_l):
        """The table of kzg_open_cosets from the monomial SRS, srs_g1 [n, 8] = tau^k G1gen, n = 2^(log_c + log_l) <= 2^27
        (sylow_hip_kzg_open_cosets_prepare): array a < l is the forward G1 transform of 2c points, x_(2c-1-u) = s_(a + l u) for u <= c - 2 and
        the identity elsewhere.  Built once per (SRS, log_l); a set flag is an entry that is the identity, not an error."""
        srs = _aos(srs_g1, 8)
        n = srs.shape[0]
        log_c = n.bit_length() - 1 - log_l
        assert n >= 1 and log_l >= 0 and log_c >= 0 and n == 1 << (log_c + log_l), (n, log_l)
        l, cc = 1 << log_l, 2 << log_c
        ds, dt, dti = self.to_device_soa(srs, 8), self.empty((l, 8, cc)), self.empty((l, cc), np.uint8)
        self._call("sylow_hip_kzg_open_cosets_prepare", ds.ptr, log_c, log_l, dt.ptr, dti.ptr)
        self.sync()                      # ds is released when this frame returns
        return dt, dti

    def kzg_open_cosets(self, table, polys, log_l, want_y=True, max_blocks=-1, planes_log=-1):
        """The proofs of every f_j on ALL c cosets of its domain and its values there (sylow_hip_kzg_open_cosets_batch): (y [m, n, 4] or None,
        pi [m, c, 8] affine words, pi flags [m, c]); value j of cell i is y[i + c j].  table: what kzg_open_cosets_prepare returned, or host
        arrays ([l, 2c, 8] words, [l, 2c] flags or None).  polys [m, n, 4].  max_blocks >= 1 caps the blocks of a multiplying launch and
        planes_log in 0 .. log_l pins the planes of the product-sums (sylow_hip_kzg_open_cosets_batch_tuned); the values do not depend on
        either."""
        a = self._kzg_polys(polys)
        m, n = a.shape[0], a.shape[1]
        log_c = n.bit_length() - 1 - log_l
        assert log_l >= 0 and log_c >= 0 and n == 1 << (log_c + log_l), (n, log_l)
        l, c = 1 << log_l, 1 << log_c
        txy, tinf = table
        dt = txy if isinstance(txy, DeviceArray) else self.to_device(np.ascontiguousarray(np.asarray(txy, dtype=np.uint64).reshape(l, 2 * c, 8).transpose(0, 2, 1)))
        dti = tinf if tinf is None or isinstance(tinf, DeviceArray) else self.to_device(np.ascontiguousarray(tinf, dtype=np.uint8).reshape(l, 2 * c))
        assert dt.shape == (l, 8, 2 * c) and (dti is None or dti.shape == (l, 2 * c)), (dt.shape, l, c)
        dc = self._kzg_polys_up(a)
        dy = self.empty((max(m, 1), 4, n)) if want_y else None
        dp, dpi = self.empty((max(m, 1), 8, c)), self.empty((max(m, 1), c), np.uint8)
        if max_blocks < 0 and planes_log < 0:
            self._call("sylow_hip_kzg_open_cosets_batch", dt.ptr, self._ptr(dti), self._ptr(dc), log_c, log_l, m, self._ptr(dy), dp.ptr, dpi.ptr)
        else:
            self._call("sylow_hip_kzg_open_cosets_batch_tuned", dt.ptr, self._ptr(dti), self._ptr(dc), log_c, log_l, m, int(max_blocks), int(planes_log),
                       self._ptr(dy), dp.ptr, dpi.ptr)
        y = np.ascontiguousarray(dy.download()[:m].transpose(0, 2, 1)) if want_y else None
        return y, np.ascontiguousarray(dp.download()[:m].transpose(0, 2, 1)), dpi.download()[:m]

    def _kzg_cells_up(self, idx, cells, log_l):
        cells = np.ascontiguousarray(cells, dtype=np.uint64)
        idx = np.ascontiguousarray(idx, dtype=np.uint64).reshape(-1)
        rows = idx.shape[0]
        assert cells.shape == (rows, 1 << log_l, 4), (cells.shape, rows, log_l)
        return rows, (self.to_device(idx) if rows else None), self._kzg_polys_up(cells)

    def kzg_coset_interp(self, idx, cells, log_c, log_l):
        """R_j = the polynomial of degree below l with the values cells [rows, l, 4] on coset idx_j mod c (sylow_hip_kzg_coset_interp_batch):
        (R [rows, l, 4] canonical words, lowest degree first, in_range [rows] = idx_j < c)."""
        rows, di, dv = self._kzg_cells_up(idx, cells, log_l)
        dr, dg = self.empty((max(rows, 1), 4, 1 << log_l)), self.empty((max(rows, 1),), np.uint8)
        self._call("sylow_hip_kzg_coset_interp_batch", self._ptr(dv), self._ptr(di), log_c, log_l, rows, dr.ptr, dg.ptr)
        return np.ascontiguousarray(dr.download()[:rows].transpose(0, 2, 1)), dg.download()[:rows]

    def kzg_cosets_reduce(self, srs_g1, c_xy, idx, cells, log_c, log_l, c_inf=None):
        """The rows the single-point verifiers take with y = 0 under tau^l G2gen (sylow_hip_kzg_cosets_reduce_batch): (C_j - R_j(tau) G1gen
        as [rows, 8] affine words, its flags [rows], z_j = v^idx_j as [rows, 4], in_range [rows]).  srs_g1 [l, 8] = tau^k G1gen, k < l."""
        srs, c_xy = _aos(srs_g1, 8), _aos(c_xy, 8)
        rows, di, dv = self._kzg_cells_up(idx, cells, log_l)
        assert srs.shape[0] == 1 << log_l and c_xy.shape[0] == rows
        if not rows:
            return np.zeros((0, 8), np.uint64), np.zeros(0, np.uint8), np.zeros((0, 4), np.uint64), np.zeros(0, np.uint8)
        ds, dc, dci = self.to_device_soa(srs, 8), self.to_device_soa(c_xy, 8), self._flags(c_inf, rows)
        do, doi, dz, dg = self.empty((8, rows)), self.empty((rows,), np.uint8), self.empty((4, rows)), self.empty((rows,), np.uint8)
        self._call("sylow_hip_kzg_cosets_reduce_batch", ds.ptr, dc.ptr, self._ptr(dci), di.ptr, dv.ptr, log_c, log_l, rows, do.ptr, doi.ptr, dz.ptr, dg.ptr)
        return self.from_device_soa(do), doi.download(), self.from_device_soa(dz), dg.download()

    def kzg_verify_cosets(self, srs_g1, tau_l_g2, c_xy, idx, cells, pi_xy, log_c, log_l, c_inf=None, pi_inf=None):
        """ok [rows]: e(C_j - R_j(tau) G1gen, G2gen) e(-pi_j, tau^l G2gen - v^idx_j G2gen) == 1 and idx_j < c
        (sylow_hip_kzg_verify_cosets_batch).  srs_g1 [l, 8] = tau^k G1gen, k < l; tau_l_g2 [1, 16] = tau^l G2gen, taken as given."""
        srs, tau, c_xy, pi_xy = _aos(srs_g1, 8), _aos(tau_l_g2, 16), _aos(c_xy, 8), _aos(pi_xy, 8)
        rows, di, dv = self._kzg_cells_up(idx, cells, log_l)
        assert srs.shape[0] == 1 << log_l and tau.shape[0] == 1 and c_xy.shape[0] == rows and pi_xy.shape[0] == rows
        if not rows:
            return np.zeros(0, dtype=np.uint8)
        ds, dtau, dc, dp = self.to_device_soa(srs, 8), self.to_device_soa(tau, 16), self.to_device_soa(c_xy, 8), self.to_device_soa(pi_xy, 8)
        dci, dpi, dok = self._flags(c_inf, rows), self._flags(pi_inf, rows), self.empty((rows,), np.uint8)
        self._call("sylow_hip_kzg_verify_cosets_batch", ds.ptr, dtau.ptr, dc.ptr, self._ptr(dci), di.ptr, dv.ptr, log_c, log_l, rows, dp.ptr, self._ptr(dpi), dok.ptr)
        return dok.download()

    # ---- a KZG polynomial of degree below n / 2 from any half of its cells (include/sylow_hip_kzg_recover.h): present [m, c] bytes,
    # non-zero = the cell is held; y [m, n, 4] in the layout of kzg_open_cosets' y (value j of cell i at y[i + c j]) ----
    def _kzg_present_up(self, present, log_c):
        p = np.ascontiguousarray(present, dtype=np.uint8)
        p = p[None] if p.ndim == 1 else p
        assert p.ndim == 2 and p.shape[1] == 1 << log_c, (p.shape, log_c)
        return p.shape[0], (self.to_device(p) if p.shape[0] else None)

    def kzg_recover_vanish(self, present, log_c, log_l):
        """The values of Z = prod_(i missing) (X^l - v^i) on the domain and on the coset 5 <w_n>, c of each per row
        (sylow_hip_kzg_recover_vanish_batch): (zd [m, c, 4], zc [m, c, 4], status [m]); status 1 = more than c / 2 cells missing (zd = 0,
        zc = 1)."""
        m, dp = self._kzg_present_up(present, log_c)
        c = 1 << log_c
        dzd, dzc, dst = self.empty((max(m, 1), 4, c)), self.empty((max(m, 1), 4, c)), self.empty((max(m, 1),), np.uint8)
        self._call("sylow_hip_kzg_recover_vanish_batch", self._ptr(dp), log_c, log_l, m, dzd.ptr, dzc.ptr, dst.ptr)
        if not m:
            return np.zeros((0, c, 4), np.uint64), np.zeros((0, c, 4), np.uint64), np.zeros(0, np.uint8)
        return np.ascontiguousarray(dzd.download().transpose(0, 2, 1)), np.ascontiguousarray(dzc.download().transpose(0, 2, 1)), dst.download()

    def kzg_recover(self, y, present, log_c, log_l, want_y=True):
        """The polynomials of degree below n / 2 whose values on the held cells are those of y (sylow_hip_kzg_recover_batch): (coeffs
        [m, n, 4], y [m, n, 4] with every cell restored or None, status [m]).  Words of y in cells that are not held are never part of the
        result.  status 0 = recovered, 1 = more than c / 2 cells missing (zero rows), 2 = the held cells are not the values of such a
        polynomial (coeffs is then what the five steps yield, its upper half not zero)."""
        a = self._kzg_polys(y)
        m, n = a.shape[0], a.shape[1]
        assert n == 1 << (log_c + log_l), (n, log_c, log_l)
        mp, dp = self._kzg_present_up(present, log_c)
        assert mp == m, (mp, m)
        dy = self._kzg_polys_up(a)
        dc, dst = self.empty((max(m, 1), 4, n)), self.empty((max(m, 1),), np.uint8)
        dyo = self.empty((max(m, 1), 4, n)) if want_y else None
        self._call("sylow_hip_kzg_recover_batch", self._ptr(dy), self._ptr(dp), log_c, log_l, m, dc.ptr, self._ptr(dyo), dst.ptr)
        coeffs = np.ascontiguousarray(dc.download()[:m].transpose(0, 2, 1))
        return coeffs, (np.ascontiguousarray(dyo.download()[:m].transpose(0, 2, 1)) if want_y else None), dst.download()[:m]

    # ---- many cells of many KZG blobs as one boolean over shared commitments (include/sylow_hip_kzg_cells.h): row k is (idx_k < c,
    # com_idx_k < n_com, cells[k] [l, 4], weights[k] [4]); a row out of range adds nothing and clears the flag unless its weight is 0 mod r ----
    def _kzg_cell_rows_up(self, idx, com_idx, cells, weights, log_l):
        rows, di, dv = self._kzg_cells_up(idx, cells, log_l)
        com_idx = np.ascontiguousarray(com_idx, dtype=np.uint64).reshape(-1)
        weights = _aos(weights, 4)
        assert com_idx.shape[0] == rows and weights.shape[0] == rows, (com_idx.shape, weights.shape, rows)
        return rows, di, (self.to_device(com_idx) if rows else None), dv, (self.to_device_soa(weights, 4) if rows else None)

    def kzg_cells_fold(self, idx, com_idx, cells, weights, log_c, log_l, n_com, route=-1, max_blocks=-1):
        """The Fr half of the check (sylow_hip_kzg_cells_fold_batch): (W [n_com, 4] = the weights summed per commitment, A [l, 4] = the
        coefficients of sum_k r_k R_k, r [rows, 4] = the weights mod r, rz [rows, 4] = r_k v^idx_k, in_range: bool); r and rz are 0 for a
        dropped row.  route 0 / 1 pins the row / column route and max_blocks >= 1 caps the blocks of a launch
        (sylow_hip_kzg_cells_fold_batch_tuned); the words depend on neither."""
        rows, di, dci, dv, dw = self._kzg_cell_rows_up(idx, com_idx, cells, weights, log_l)
        n_com = int(n_com)
        dwo, dao = self.empty((4, max(n_com, 1))), self.empty((4, 1 << log_l))
        dr, drz, dg = self.empty((4, max(rows, 1))), self.empty((4, max(rows, 1))), self.empty((1,), np.uint8)
        ins = [self._ptr(di), self._ptr(dci), self._ptr(dv), self._ptr(dw), log_c, log_l, rows, n_com]
        outs = [dwo.ptr, dao.ptr, dr.ptr, drz.ptr, dg.ptr]
        if route < 0 and max_blocks < 0:
            self._call("sylow_hip_kzg_cells_fold_batch", *ins, *outs)
        else:
            self._call("sylow_hip_kzg_cells_fold_batch_tuned", *ins, int(route), int(max_blocks), *outs)
        return (self.from_device_soa(dwo)[:n_com], self.from_device_soa(dao), self.from_device_soa(dr)[:rows], self.from_device_soa(drz)[:rows],
                bool(dg.download()[0]))

    def _kzg_cells_points_up(self, srs_g1, c_xy, pi_xy, c_inf, pi_inf, rows, log_l):
        srs, c_xy, pi_xy = _aos(srs_g1, 8), _aos(c_xy, 8), _aos(pi_xy, 8)
        n_com = c_xy.shape[0]
        assert srs.shape[0] == 1 << log_l and pi_xy.shape[0] == rows, (srs.shape, pi_xy.shape, rows, log_l)
        return n_com, (self.to_device_soa(srs, 8), self.to_device_soa(c_xy, 8) if n_com else None, self._flags(c_inf, n_com) if n_com else None,
                       self.to_device_soa(pi_xy, 8) if rows else None, self._flags(pi_inf, rows) if rows else None)

    def kzg_cells_reduce(self, srs_g1, c_xy, idx, com_idx, cells, pi_xy, weights, log_c, log_l, c_inf=None, pi_inf=None):
        """The whole batch as ONE row of the single-point verifiers under tau^l G2gen (sylow_hip_kzg_cells_reduce_batch): (F [1, 8],
        F flag [1], P [1, 8], P flag [1], in_range: bool) with F = sum_b W_b C_b + sum_k (r_k v^idx_k) pi_k - A(tau) G1gen and
        P = sum_k r_k pi_k; the row is (F, z = 0, y = 0, P).  srs_g1 [l, 8] = tau^k G1gen, k < l; c_xy [n_com, 8]; pi_xy [rows, 8]."""
        rows, di, dci, dv, dw = self._kzg_cell_rows_up(idx, com_idx, cells, weights, log_l)
        n_com, (ds, dc, dcf, dp, dpf) = self._kzg_cells_points_up(srs_g1, c_xy, pi_xy, c_inf, pi_inf, rows, log_l)
        df, dfi, dpo, dpi, dg = self.empty((8, 1)), self.empty((1,), np.uint8), self.empty((8, 1)), self.empty((1,), np.uint8), self.empty((1,), np.uint8)
        self._call("sylow_hip_kzg_cells_reduce_batch", ds.ptr, self._ptr(dc), self._ptr(dcf), self._ptr(di), self._ptr(dci), self._ptr(dv), self._ptr(dp),
                   self._ptr(dpf), self._ptr(dw), log_c, log_l, rows, n_com, df.ptr, dfi.ptr, dpo.ptr, dpi.ptr, dg.ptr)
        return self.from_device_soa(df), dfi.download(), self.from_device_soa(dpo), dpi.download(), bool(dg.download()[0])

    def kzg_cells_verify_weighted(self, srs_g1, tau_l_g2, c_xy, idx, com_idx, cells, pi_xy, weights, log_c, log_l, c_inf=None, pi_inf=None):
        """"are ALL the cells valid?" as ONE Gt (sylow_hip_kzg_cells_verify_weighted): (Gt words [1, 48], is_one AND in_range: bool,
        in_range: bool).  weights [rows, 4] drawn by the caller AFTER the rows are fixed (any 256-bit words, taken mod r; 0 removes a row).
        tau_l_g2 [1, 16] = tau^l G2gen, taken as given."""
        tau = _aos(tau_l_g2, 16)
        assert tau.shape[0] == 1
        rows, di, dci, dv, dw = self._kzg_cell_rows_up(idx, com_idx, cells, weights, log_l)
        n_com, (ds, dc, dcf, dp, dpf) = self._kzg_cells_points_up(srs_g1, c_xy, pi_xy, c_inf, pi_inf, rows, log_l)
        dtau, dgt, dis, dg = self.to_device_soa(tau, 16), self.empty((48, 1)), self.empty((1,), np.uint8), self.empty((1,), np.uint8)
        self._call("sylow_hip_kzg_cells_verify_weighted", ds.ptr, dtau.ptr, self._ptr(dc), self._ptr(dcf), self._ptr(di), self._ptr(dci), self._ptr(dv),
                   self._ptr(dp), self._ptr(dpf), self._ptr(dw), log_c, log_l, rows, n_com, dgt.ptr, dis.ptr, dg.ptr)
        return self.from_device_soa(dgt), bool(dis.download()[0]), bool(dg.download()[0])

    # ---- scans over Fr and PLONK's permutation grand product (include/sylow_hip_fr_scan.h).  Rows are [m, len, 4] on the host (or [len, 4]:
    # one row) and [m][4][len] on the device; any 256-bit words, taken mod r; op 0 = sum, 1 = product ----
    def _fr_rows(self, a):
        a = np.ascontiguousarray(a, dtype=np.uint64)
        one = a.ndim == 2
        return one, self._kzg_polys(a[None] if one else a)

    def _fr_rows_down(self, d, m, one):
        out = np.ascontiguousarray(d.download()[:m].transpose(0, 2, 1))
        return out[0] if one else out

    def _fr_totals_down(self, d, m, one):
        t = self.from_device_soa(d)[:m]
        return t[0] if one else t

    def fr_scan(self, a, op, exclusive=False, max_blocks=-1, totals_tile=-1):
        """out[j, k] = a[j, 0] o .. o a[j, k] (exclusive: up to k - 1, the identity at k = 0) and the rows' totals [m, 4]
        (sylow_hip_fr_scan_batch).  max_blocks >= 1 caps the blocks of a launch and totals_tile in 1 .. 256 pins the chunk totals the second
        level scans per step (sylow_hip_fr_scan_batch_tuned); the words depend on neither."""
        one, a = self._fr_rows(a)
        m, ln = a.shape[0], a.shape[1]
        da, do, dt = self._kzg_polys_up(a), self.empty((max(m, 1), 4, ln)), self.empty((4, max(m, 1)))
        if max_blocks < 0 and totals_tile < 0:
            self._call("sylow_hip_fr_scan_batch", self._ptr(da), ln, m, int(op), int(bool(exclusive)), do.ptr, dt.ptr)
        else:
            self._call("sylow_hip_fr_scan_batch_tuned", self._ptr(da), ln, m, int(op), int(bool(exclusive)), int(max_blocks), int(totals_tile), do.ptr, dt.ptr)
        return self._fr_rows_down(do, m, one), self._fr_totals_down(dt, m, one)

    def fr_ratio_scan(self, num, den, op, max_blocks=-1, totals_tile=-1):
        """The exclusive scan of t = num / den, inv(0) = 0 (sylow_hip_fr_ratio_scan_batch): (out [m, len, 4] with out[j, 0] the identity and
        out[j, k] = t[j, 0] o .. o t[j, k - 1], the totals t[j, 0] o .. o t[j, len - 1] as [m, 4], status [m]: bit 0 = a denominator of the row
        is 0 mod r).  num None: all ones.  The denominators of a chunk share one inversion and no inverse or ratio reaches memory."""
        one, d = self._fr_rows(den)
        m, ln = d.shape[0], d.shape[1]
        dn = None
        if num is not None:
            _, nm = self._fr_rows(num)
            assert nm.shape == d.shape, (nm.shape, d.shape)
            dn = self._kzg_polys_up(nm)
        dd, do, dt, ds = self._kzg_polys_up(d), self.empty((max(m, 1), 4, ln)), self.empty((4, max(m, 1))), self.empty((max(m, 1),), np.uint8)
        if max_blocks < 0 and totals_tile < 0:
            self._call("sylow_hip_fr_ratio_scan_batch", self._ptr(dn), self._ptr(dd), ln, m, int(op), do.ptr, dt.ptr, ds.ptr)
        else:
            self._call("sylow_hip_fr_ratio_scan_batch_tuned", self._ptr(dn), self._ptr(dd), ln, m, int(op), int(max_blocks), int(totals_tile), do.ptr, dt.ptr, ds.ptr)
        st = ds.download()[:m]
        return self._fr_rows_down(do, m, one), self._fr_totals_down(dt, m, one), (st[0] if one else st)

    def plonk_identity(self, shifts, log_n):
        """The identity columns of the permutation argument, out[j, i] = shifts[j] w_n^i as [W, n, 4] (sylow_hip_plonk_identity_batch)."""
        sh = _aos(shifts, 4)
        W = sh.shape[0]
        ds, do = self.to_device_soa(sh, 4), self.empty((W, 4, 1 << log_n))
        self._call("sylow_hip_plonk_identity_batch", ds.ptr, int(log_n), W, do.ptr)
        return np.ascontiguousarray(do.download().transpose(0, 2, 1))

    def plonk_permutation(self, wires, sigma, shifts, beta, gamma, max_blocks=-1, totals_tile=-1):
        """z of the copy-constraint argument for m instances over one permutation (sylow_hip_plonk_permutation_batch): wires [m, W, n, 4],
        sigma [W, n, 4], shifts [W, 4], beta and gamma [m, 4] DRAWN AFTER THE WIRE COMMITMENTS ARE FIXED -> (z [m, n, 4] with z[j, 0] = 1,
        z_n [m, 4], status [m]: bit 0 = a zero denominator, bit 1 = z_n != 1, 0 = the copy constraints hold)."""
        w, sg, sh = np.ascontiguousarray(wires, dtype=np.uint64), np.ascontiguousarray(sigma, dtype=np.uint64), _aos(shifts, 4)
        beta, gamma = _aos(beta, 4), _aos(gamma, 4)
        assert w.ndim == 4 and w.shape[3] == 4 and sg.ndim == 3, (w.shape, sg.shape)
        m, W, n = w.shape[0], w.shape[1], w.shape[2]
        log_n = n.bit_length() - 1
        assert n == 1 << log_n and sg.shape == (W, n, 4) and sh.shape[0] == W and beta.shape[0] == m and gamma.shape[0] == m, (w.shape, sg.shape, sh.shape)
        dw = self.to_device(np.ascontiguousarray(w.transpose(0, 1, 3, 2))) if m else None
        dsg, dsh = self.to_device(np.ascontiguousarray(sg.transpose(0, 2, 1))), self.to_device_soa(sh, 4)
        db, dg = (self.to_device_soa(beta, 4), self.to_device_soa(gamma, 4)) if m else (None, None)
        dz, dt, ds = self.empty((max(m, 1), 4, n)), self.empty((4, max(m, 1))), self.empty((max(m, 1),), np.uint8)
        ins = [self._ptr(dw), dsg.ptr, dsh.ptr, self._ptr(db), self._ptr(dg), log_n, W, m]
        if max_blocks < 0 and totals_tile < 0:
            self._call("sylow_hip_plonk_permutation_batch", *ins, dz.ptr, dt.ptr, ds.ptr)
        else:
            self._call("sylow_hip_plonk_permutation_batch_tuned", *ins, int(max_blocks), int(totals_tile), dz.ptr, dt.ptr, ds.ptr)
        return np.ascontiguousarray(dz.download()[:m].transpose(0, 2, 1)), self.from_device_soa(dt)[:m], ds.download()[:m]

    # ---- PLONK's quotient polynomial (include/sylow_plonk.h).  n = 2^log_n, N = 2^(log_n + log_e); the table of a circuit stays on the device:
    # [2 W + 3][4][N] then [4][E] as one flat array of words ----
    def plonk_quotient_prepare(self, selectors, sigma, log_e=2):
        """The table of one circuit (sylow_plonk_quotient_prepare): selectors [W + 2, n, 4] -- the values on <w_n> of q_0 .. q_(W-1), q_M,
        q_C -- and sigma [W, n, 4] as for plonk_permutation -> a DeviceArray of 4 N (2 W + 3) + 4 E words: the rows on the coset
        K = 5 <w_N>, then (X^n - 1)^-1 there."""
        sel, sg = np.ascontiguousarray(selectors, dtype=np.uint64), np.ascontiguousarray(sigma, dtype=np.uint64)
        assert sel.ndim == 3 and sg.ndim == 3 and sel.shape[2] == 4, (sel.shape, sg.shape)
        W, n = sg.shape[0], sg.shape[1]
        log_n = n.bit_length() - 1
        assert n == 1 << log_n and sel.shape == (W + 2, n, 4) and sg.shape == (W, n, 4), (sel.shape, sg.shape)
        dsel, dsg = self.to_device(np.ascontiguousarray(sel.transpose(0, 2, 1))), self.to_device(np.ascontiguousarray(sg.transpose(0, 2, 1)))
        table = self.empty((4 * (n << log_e) * (2 * W + 3) + 4 * (1 << log_e),))
        self._call("sylow_plonk_quotient_prepare", dsel.ptr, dsg.ptr, log_n, int(log_e), W, table.ptr)
        return table

    def plonk_quotient_table_up(self, rows, zinv):
        """a table from host words: rows [2 W + 3, N, 4] and zinv [E, 4] -> the DeviceArray plonk_quotient_prepare would return for them"""
        rows, zinv = np.ascontiguousarray(rows, dtype=np.uint64), _aos(zinv, 4)
        return self.to_device(np.concatenate([rows.transpose(0, 2, 1).reshape(-1), zinv.T.reshape(-1)]))

    def plonk_quotient_table_down(self, table, W, log_n, log_e):
        """(rows [2 W + 3, N, 4], zinv [E, 4]) of a table on the device"""
        flat, big, E = table.download().reshape(-1), 1 << (log_n + log_e), 1 << log_e
        rows = flat[:4 * big * (2 * W + 3)].reshape(2 * W + 3, 4, big).transpose(0, 2, 1)
        return np.ascontiguousarray(rows), np.ascontiguousarray(flat[4 * big * (2 * W + 3):].reshape(4, E).T)

    def _plonk_challenges_up(self, m, *scalars):
        out = []
        for v in scalars:
            v = _aos(v, 4)
            assert v.shape[0] == m, (v.shape, m)
            out.append(self.to_device_soa(v, 4) if m else None)
        return out

    def plonk_quotient_evals(self, table, wires_ext, z_ext, pi_ext, shifts, beta, gamma, alpha, log_n, log_e=2, max_blocks=-1):
        """The fused kernel alone (sylow_plonk_quotient_evals_batch): the values on K of the wires [m, W, N, 4], of z [m, N, 4] and of the
        public inputs ([m, N, 4] or None), shifts [W, 4], one (beta, gamma, alpha) per instance as [m, 4], THE CALLER'S -> t_ext [m, N, 4],
        (gate + alpha perm + alpha^2 boundary) / (X^n - 1) point by point.  max_blocks >= 1 caps the blocks of the launch; the words do
        not depend on it."""
        w, z, sh = np.ascontiguousarray(wires_ext, dtype=np.uint64), np.ascontiguousarray(z_ext, dtype=np.uint64), _aos(shifts, 4)
        assert w.ndim == 4 and w.shape[3] == 4 and z.ndim == 3, (w.shape, z.shape)
        m, W, big = w.shape[0], w.shape[1], 1 << (log_n + log_e)
        assert w.shape == (m, W, big, 4) and z.shape == (m, big, 4) and sh.shape[0] == W, (w.shape, z.shape, sh.shape)
        dw = self.to_device(np.ascontiguousarray(w.transpose(0, 1, 3, 2))) if m else None
        dz, dpi = self._kzg_polys_up(z), None
        if pi_ext is not None:
            p = np.ascontiguousarray(pi_ext, dtype=np.uint64)
            assert p.shape == z.shape, (p.shape, z.shape)
            dpi = self._kzg_polys_up(p)
        db, dg, da = self._plonk_challenges_up(m, beta, gamma, alpha)
        dsh, dt = self.to_device_soa(sh, 4), self.empty((max(m, 1), 4, big))
        ins = [table.ptr, self._ptr(dw), self._ptr(dz), self._ptr(dpi), dsh.ptr, self._ptr(db), self._ptr(dg), self._ptr(da), int(log_n), int(log_e), W, m]
        if max_blocks < 0:
            self._call("sylow_plonk_quotient_evals_batch", *ins, dt.ptr)
        else:
            self._call("sylow_plonk_quotient_evals_batch_tuned", *ins, int(max_blocks), dt.ptr)
        return np.ascontiguousarray(dt.download()[:m].transpose(0, 2, 1))

    def plonk_quotient(self, table, wires, z, pi, shifts, beta, gamma, alpha, log_n, log_e=2, max_blocks=-1):
        """t from COEFFICIENTS (sylow_plonk_quotient_batch): wires [m, W, len_w, 4], z [m, len_z, 4], pi [m, n, 4] or None, the lengths free
        in 1 .. N (blinded polynomials are longer than n) -> (t [m, N, 4], the coefficients of the polynomial of degree < N that equals the
        numerator over X^n - 1 on K, status [m]: bit 0 = a coefficient above the degree bound is not 0, the constraints do not hold)."""
        w, z, sh = np.ascontiguousarray(wires, dtype=np.uint64), np.ascontiguousarray(z, dtype=np.uint64), _aos(shifts, 4)
        assert w.ndim == 4 and w.shape[3] == 4 and z.ndim == 3 and z.shape[2] == 4, (w.shape, z.shape)
        m, W, len_w, len_z, n, big = w.shape[0], w.shape[1], w.shape[2], z.shape[1], 1 << log_n, 1 << (log_n + log_e)
        assert z.shape[0] == m and sh.shape[0] == W, (w.shape, z.shape, sh.shape)
        dw = self.to_device(np.ascontiguousarray(w.transpose(0, 1, 3, 2))) if m else None
        dz, dpi = self._kzg_polys_up(z), None
        if pi is not None:
            p = np.ascontiguousarray(pi, dtype=np.uint64)
            assert p.shape == (m, n, 4), p.shape
            dpi = self._kzg_polys_up(p)
        db, dg, da = self._plonk_challenges_up(m, beta, gamma, alpha)
        dsh, dt, ds = self.to_device_soa(sh, 4), self.empty((max(m, 1), 4, big)), self.empty((max(m, 1),), np.uint8)
        ins = [table.ptr, self._ptr(dw), len_w, self._ptr(dz), len_z, self._ptr(dpi), dsh.ptr, self._ptr(db), self._ptr(dg), self._ptr(da), int(log_n), int(log_e), W, m]
        if max_blocks < 0:
            self._call("sylow_plonk_quotient_batch", *ins, dt.ptr, ds.ptr)
        else:
            self._call("sylow_plonk_quotient_batch_tuned", *ins, int(max_blocks), dt.ptr, ds.ptr)
        return np.ascontiguousarray(dt.download()[:m].transpose(0, 2, 1)), ds.download()[:m]

    # ---- PLONK's closing rounds (include/sylow_popen.h): the evaluations at zeta, the linearisation polynomial, the two openings.  The
    # coefficient table of a circuit stays on the device: [2 W + 2][4][n] ----
    def plonk_open_prepare(self, selectors, sigma):
        """The coefficient table of one circuit (sylow_popen_prepare): selectors [W + 2, n, 4] and sigma [W, n, 4] as for
        plonk_quotient_prepare -> a DeviceArray [2 W + 2, 4, n]: the coefficients of q_0 .. q_(W-1), q_M, q_C, sigma_0 .. sigma_(W-1)."""
        sel, sg = np.ascontiguousarray(selectors, dtype=np.uint64), np.ascontiguousarray(sigma, dtype=np.uint64)
        assert sel.ndim == 3 and sg.ndim == 3 and sel.shape[2] == 4, (sel.shape, sg.shape)
        W, n = sg.shape[0], sg.shape[1]
        log_n = n.bit_length() - 1
        assert n == 1 << log_n and sel.shape == (W + 2, n, 4) and sg.shape == (W, n, 4), (sel.shape, sg.shape)
        dsel, dsg = self.to_device(np.ascontiguousarray(sel.transpose(0, 2, 1))), self.to_device(np.ascontiguousarray(sg.transpose(0, 2, 1)))
        ctable = self.empty((2 * W + 2, 4, n))
        self._call("sylow_popen_prepare", dsel.ptr, dsg.ptr, log_n, W, ctable.ptr)
        return ctable

    def plonk_open_ctable_up(self, rows):
        """a coefficient table from host words: rows [2 W + 2, n, 4] -> the DeviceArray plonk_open_prepare would return for them"""
        return self.to_device(np.ascontiguousarray(np.ascontiguousarray(rows, dtype=np.uint64).transpose(0, 2, 1)))

    def plonk_open_ctable_down(self, ctable):
        """rows [2 W + 2, n, 4] of a coefficient table on the device"""
        return np.ascontiguousarray(ctable.download().transpose(0, 2, 1))

    def _plonk_open_polys_up(self, ctable, wires, z, pi):
        W, n = ctable.shape[0] // 2 - 1, ctable.shape[2]
        z = np.ascontiguousarray(z, dtype=np.uint64)
        assert z.ndim == 3 and z.shape[2] == 4 and z.shape[1] >= 1, z.shape
        m, dw, len_w, dpi = z.shape[0], None, 1, None
        if wires is not None:
            w = np.ascontiguousarray(wires, dtype=np.uint64)
            assert w.ndim == 4 and w.shape[:2] == (m, W) and w.shape[3] == 4 and w.shape[2] >= 1, (w.shape, z.shape, W)
            len_w, dw = w.shape[2], (self.to_device(np.ascontiguousarray(w.transpose(0, 1, 3, 2))) if m else None)
        if pi is not None:
            p = np.ascontiguousarray(pi, dtype=np.uint64)
            assert p.shape == (m, n, 4), p.shape
            dpi = self._kzg_polys_up(p)
        return W, n.bit_length() - 1, m, dw, len_w, self._kzg_polys_up(z), z.shape[1], dpi

    def plonk_open_evaluate(self, ctable, wires, z, pi, zeta, max_blocks=-1):
        """The 2 W + 1 evaluations of m instances (sylow_popen_evaluate_batch): the COEFFICIENTS of the wires [m, W, len_w, 4], of z
        [m, len_z, 4] and of the public inputs ([m, n, 4] or None), zeta [m, 4] DRAWN AFTER THE COMMITMENTS TO t ARE FIXED -> evals
        [m, 2 W + 1, 4]: w_j(zeta) for j < W, sigma_j(zeta) for j < W - 1, z(zeta w_n), PI(zeta).  max_blocks >= 1 caps the blocks of a
        launch; the words do not depend on it."""
        W, log_n, m, dw, len_w, dz, len_z, dpi = self._plonk_open_polys_up(ctable, wires, z, pi)
        dzeta, = self._plonk_challenges_up(m, zeta)
        de = self.empty((4, (2 * W + 1) * max(m, 1)))
        ins = [ctable.ptr, self._ptr(dw), len_w, self._ptr(dz), len_z, self._ptr(dpi), self._ptr(dzeta), log_n, W, m]
        if max_blocks < 0:
            self._call("sylow_popen_evaluate_batch", *ins, de.ptr)
        else:
            self._call("sylow_popen_evaluate_batch_tuned", *ins, int(max_blocks), de.ptr)
        return self.from_device_soa(de)[:(2 * W + 1) * m].reshape(m, 2 * W + 1, 4)

    def plonk_open_linearise(self, ctable, wires, z, t, evals, shifts, beta, gamma, alpha, zeta, v, log_e=2, len_out=None, want_r=True, want_f=True,
                             max_blocks=-1):
        """r and F of m instances (sylow_popen_linearise_batch): t [m, N, 4] as plonk_quotient returns it, evals [m, 2 W + 1, 4] as
        plonk_open_evaluate returns them, v [m, 4] DRAWN AFTER THE EVALUATIONS ARE FIXED -> (r [m, len_out, 4] or None, F [m, len_out, 4]
        or None, status [m]: bit 0 = r(zeta) != 0, bit 1 = zeta^n = 1).  len_out None: the shortest the outputs allow.  Without want_f,
        wires and v may be None."""
        assert want_r or want_f
        W, log_n, m, dw, len_w, dz, len_z, _ = self._plonk_open_polys_up(ctable, wires if want_f else None, z, None)
        n, big = 1 << log_n, 1 << (log_n + log_e)
        t, ev, sh = np.ascontiguousarray(t, dtype=np.uint64), np.ascontiguousarray(evals, dtype=np.uint64), _aos(shifts, 4)
        assert t.shape == (m, big, 4) and ev.shape == (m, 2 * W + 1, 4) and sh.shape[0] == W, (t.shape, ev.shape, sh.shape)
        if len_out is None:
            len_out = max(n, len_z, len_w if want_f else 1)
        dt, dev, dsh = self._kzg_polys_up(t), (self.to_device_soa(ev.reshape(-1, 4), 4) if m else None), self.to_device_soa(sh, 4)
        db, dg, da, dzeta = self._plonk_challenges_up(m, beta, gamma, alpha, zeta)
        dv = self._plonk_challenges_up(m, v)[0] if want_f else None
        dr = self.empty((max(m, 1), 4, len_out)) if want_r else None
        df = self.empty((max(m, 1), 4, len_out)) if want_f else None
        ds = self.empty((max(m, 1),), np.uint8)
        ins = [ctable.ptr, self._ptr(dw), len_w, self._ptr(dz), len_z, self._ptr(dt), self._ptr(dev), dsh.ptr, self._ptr(db), self._ptr(dg), self._ptr(da),
               self._ptr(dzeta), self._ptr(dv), log_n, int(log_e), W, m, int(len_out)]
        if max_blocks < 0:
            self._call("sylow_popen_linearise_batch", *ins, self._ptr(dr), self._ptr(df), ds.ptr)
        else:
            self._call("sylow_popen_linearise_batch_tuned", *ins, int(max_blocks), self._ptr(dr), self._ptr(df), ds.ptr)
        down = lambda d: None if d is None else np.ascontiguousarray(d.download()[:m].transpose(0, 2, 1))
        return down(dr), down(df), ds.download()[:m]

    def plonk_open(self, srs_g1, ctable, wires, z, pi, t, shifts, beta, gamma, alpha, zeta, v, log_e=2):
        """The full route (sylow_popen_open_batch) under the monomial SRS srs_g1 [len_f, 8], len_f >= max(n, len_z, len_w): (evals
        [m, 2 W + 1, 4], (W_zeta [m, 8], flags [m]), (W_omega [m, 8], flags [m]), status [m]).  The proofs are word for word kzg_open of F
        at zeta and of z at zeta w_n.  v IS TAKEN BESIDE zeta: a caller whose v depends on the evaluations composes plonk_open_evaluate,
        plonk_open_linearise and kzg_open."""
        W, log_n, m, dw, len_w, dz, len_z, dpi = self._plonk_open_polys_up(ctable, wires, z, pi)
        srs, t, sh = _aos(srs_g1, 8), np.ascontiguousarray(t, dtype=np.uint64), _aos(shifts, 4)
        assert t.shape == (m, 1 << (log_n + log_e), 4) and sh.shape[0] == W, (t.shape, sh.shape)
        dsrs, dt, dsh = self.to_device_soa(srs, 8), self._kzg_polys_up(t), self.to_device_soa(sh, 4)
        db, dg, da, dzeta, dv = self._plonk_challenges_up(m, beta, gamma, alpha, zeta, v)
        mm = max(m, 1)
        de, d1, d1i, d2, d2i, ds = (self.empty((4, (2 * W + 1) * mm)), self.empty((8, mm)), self.empty((mm,), np.uint8), self.empty((8, mm)),
                                    self.empty((mm,), np.uint8), self.empty((mm,), np.uint8))
        self._call("sylow_popen_open_batch", dsrs.ptr, ctable.ptr, self._ptr(dw), len_w, self._ptr(dz), len_z, self._ptr(dpi), self._ptr(dt), dsh.ptr, self._ptr(db),
                   self._ptr(dg), self._ptr(da), self._ptr(dzeta), self._ptr(dv), log_n, int(log_e), W, m, srs.shape[0], de.ptr, d1.ptr, d1i.ptr, d2.ptr, d2i.ptr,
                   ds.ptr)
        return (self.from_device_soa(de)[:(2 * W + 1) * m].reshape(m, 2 * W + 1, 4), (self.from_device_soa(d1)[:m], d1i.download()[:m]),
                (self.from_device_soa(d2)[:m], d2i.download()[:m]), ds.download()[:m])

    # ---- the batched PLONK verifier (include/sylow_pverify.h).  A key is (points, flags or None) as host words [2 W + 2, 8] / [2 W + 2] or as
    # the pair of DeviceArrays plonk_verify_key_up returns; proofs are [m, W + E + 3, 8] words + flags [m, W + E + 3] or None on the host and
    # slot-major on the device; evals [m, 2 W + 1, 4] exactly as plonk_open_evaluate returns them; pub [m, n_pub, 4] or None ----
    def plonk_verify_key_up(self, vk_xy, vk_inf=None):
        """a verifying key onto the device, once: ([8][2 W + 2] words, flags or None)"""
        vk = _aos(vk_xy, 8)
        return self.to_device_soa(vk, 8), self._flags(vk_inf, vk.shape[0])

    def _plonk_verify_up(self, evals, pub, shifts, challenges, log_n, log_e, vk=None, proofs=None, proof_inf=None):
        ev, sh = np.ascontiguousarray(evals, dtype=np.uint64), _aos(shifts, 4)
        assert ev.ndim == 3 and ev.shape[2] == 4 and ev.shape[1] == 2 * sh.shape[0] + 1, (ev.shape, sh.shape)
        m, W, E = ev.shape[0], sh.shape[0], 1 << int(log_e)
        n_pub, dpub = 0, None
        if pub is not None:
            p = np.ascontiguousarray(pub, dtype=np.uint64)
            assert p.ndim == 3 and p.shape[0] == m and p.shape[2] == 4, p.shape
            n_pub = p.shape[1]
            dpub = self.to_device_soa(np.ascontiguousarray(p.transpose(1, 0, 2)).reshape(-1, 4), 4) if m and n_pub else None
        dev = self.to_device_soa(ev.reshape(-1, 4), 4) if m else None
        ins = [self._ptr(dev), self._ptr(dpub), n_pub, self.to_device_soa(sh, 4)] + self._plonk_challenges_up(m, *challenges)
        dims = [int(log_n), int(log_e), W, m]
        pts = []
        if vk is not None:
            dvk, dvi = vk if isinstance(vk[0], DeviceArray) else self.plonk_verify_key_up(*vk)
            assert dvk.shape == (8, 2 * W + 2), dvk.shape
            pr = np.ascontiguousarray(proofs, dtype=np.uint64)
            assert pr.shape == (m, W + E + 3, 8), (pr.shape, m, W, E)
            dpr = self.to_device_soa(np.ascontiguousarray(pr.transpose(1, 0, 2)).reshape(-1, 8), 8) if m else None
            dpi = None
            if proof_inf is not None and m:
                dpi = self.to_device(np.ascontiguousarray(np.asarray(proof_inf, dtype=np.uint8).reshape(m, W + E + 3).T))
            pts = [dvk, dvi, dpr, dpi]
        held = [dev, dpub] + ins[3:] + pts
        return m, W, E, [self._ptr(x) if isinstance(x, DeviceArray) or x is None else x for x in pts], \
            [self._ptr(x) if isinstance(x, DeviceArray) else x for x in ins], dims, held

    def plonk_verify_scalars(self, evals, pub, shifts, beta, gamma, alpha, zeta, v, u, log_n, log_e=2, max_blocks=-1):
        """The term scalars of m proofs (sylow_pverify_scalars_batch): (k [m, 3 W + E + 5, 4] in the header's term order, y [m, 4], status
        [m]: bit 1 = zeta^n = 1), canonical words.  Slot 2 W of evals is not read.  max_blocks >= 1 caps the blocks of a launch; the words do
        not depend on it."""
        m, W, E, _, ins, dims, held = self._plonk_verify_up(evals, pub, shifts, (beta, gamma, alpha, zeta, v, u), log_n, log_e)
        T, mm = 3 * W + E + 5, max(m, 1)
        dk, dy, ds = self.empty((4, T * mm)), self.empty((4, mm)), self.empty((mm,), np.uint8)
        if max_blocks < 0:
            self._call("sylow_pverify_scalars_batch", *ins, *dims, dk.ptr, dy.ptr, ds.ptr)
        else:
            self._call("sylow_pverify_scalars_batch_tuned", *ins, *dims, int(max_blocks), dk.ptr, dy.ptr, ds.ptr)
        k = self.from_device_soa(dk)[:T * m].reshape(T, m, 4).transpose(1, 0, 2)
        return np.ascontiguousarray(k), self.from_device_soa(dy)[:m], ds.download()[:m]

    def plonk_verify_fold(self, vk, proofs, evals, pub, shifts, beta, gamma, alpha, zeta, v, u, log_n, log_e=2, proof_inf=None):
        """The KZG row of every proof (sylow_pverify_fold_batch): ((C [m, 8], flags [m]), (pi [m, 8], flags [m]), y [m, 4], status [m]); C and
        pi are bit-identical to g1_lincomb over the literal terms."""
        m, W, E, pts, ins, dims, held = self._plonk_verify_up(evals, pub, shifts, (beta, gamma, alpha, zeta, v, u), log_n, log_e, vk, proofs, proof_inf)
        mm = max(m, 1)
        dc, dci, dp, dpi, dy, ds = (self.empty((8, mm)), self.empty((mm,), np.uint8), self.empty((8, mm)), self.empty((mm,), np.uint8), self.empty((4, mm)),
                                    self.empty((mm,), np.uint8))
        self._call("sylow_pverify_fold_batch", *pts, *ins, *dims, dc.ptr, dci.ptr, dp.ptr, dpi.ptr, dy.ptr, ds.ptr)
        return ((self.from_device_soa(dc)[:m], dci.download()[:m]), (self.from_device_soa(dp)[:m], dpi.download()[:m]), self.from_device_soa(dy)[:m],
                ds.download()[:m])

    def plonk_verify(self, tau_g2, vk, proofs, evals, pub, shifts, beta, gamma, alpha, zeta, v, u, log_n, log_e=2, proof_inf=None):
        """(ok [m], status [m]) for m proofs of one circuit (sylow_pverify_verify_batch): ok_i = both openings of proof i verify under u_i, and
        0 where status bit 1 (zeta^n = 1) is set.  tau_g2 [1, 16] words or a DeviceArray [16, 1]; it must lie in G2 proper."""
        dtau = tau_g2 if isinstance(tau_g2, DeviceArray) else self.to_device_soa(_aos(tau_g2, 16), 16)
        assert dtau.shape == (16, 1), dtau.shape
        m, W, E, pts, ins, dims, held = self._plonk_verify_up(evals, pub, shifts, (beta, gamma, alpha, zeta, v, u), log_n, log_e, vk, proofs, proof_inf)
        dok, ds = self.empty((max(m, 1),), np.uint8), self.empty((max(m, 1),), np.uint8)
        self._call("sylow_pverify_verify_batch", dtau.ptr, *pts, *ins, *dims, dok.ptr, ds.ptr)
        return dok.download()[:m], ds.download()[:m]

    def plonk_batch_verify_weighted(self, tau_g2, vk, proofs, evals, pub, shifts, beta, gamma, alpha, zeta, v, u, weights, log_n, log_e=2, proof_inf=None):
        """m proofs as ONE Gt (sylow_pverify_batch_verify_weighted): (Gt words [1, 48], bool, status [m]); weights [m, 4] drawn by the caller
        AFTER all proofs are fixed (any 256-bit words, taken mod r; 0 removes a proof).  The bool is False when a proof with a nonzero weight
        has zeta^n = 1."""
        dtau = tau_g2 if isinstance(tau_g2, DeviceArray) else self.to_device_soa(_aos(tau_g2, 16), 16)
        assert dtau.shape == (16, 1), dtau.shape
        m, W, E, pts, ins, dims, held = self._plonk_verify_up(evals, pub, shifts, (beta, gamma, alpha, zeta, v, u), log_n, log_e, vk, proofs, proof_inf)
        dw, = self._plonk_challenges_up(m, weights)
        dgt, dis, ds = self.empty((48, 1)), self.empty((1,), np.uint8), self.empty((max(m, 1),), np.uint8)
        self._call("sylow_pverify_batch_verify_weighted", dtau.ptr, *pts, *ins, self._ptr(dw), *dims, dgt.ptr, dis.ptr, ds.ptr)
        return self.from_device_soa(dgt), bool(dis.download()[0]), ds.download()[:m]

    # ---- Groth16, the prover's side.  A sparse matrix is CSR: (row_ptr [rows + 1], col [nnz], val [nnz, 4]); Fr batches are [m, n, 4] on the
    # host and [m][4][n] on the device; any 256-bit words, taken mod r ----
    def _csr_up(self, csr):
        row_ptr, col, val = csr
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64).reshape(-1)
        col, val = np.ascontiguousarray(col, dtype=np.uint64).reshape(-1), _aos(val, 4)
        nnz = col.shape[0]
        assert row_ptr.shape[0] >= 1 and val.shape[0] == nnz
        return self.to_device(row_ptr), (self.to_device(col) if nnz else None), (self.to_device_soa(val, 4) if nnz else None), row_ptr.shape[0] - 1, nnz

    def fr_spmv(self, csr, w, n_out=None, lanes_log=-1):
        """out_j = M w_j for the CSR matrix `csr` and the vectors w [m, n_cols, 4] (or [n_cols, 4]: one vector), padded with zero rows to n_out
        (None: rows) (sylow_hip_fr_spmv_batch).  lanes_log >= 0 pins 2^lanes_log lanes per row (sylow_hip_fr_spmv_batch_tuned); the values do
        not depend on it.  An entry whose column is n_cols or more contributes zero.  Canonical words [m, n_out, 4] (or [n_out, 4])."""
        a = np.ascontiguousarray(w, dtype=np.uint64)
        one = a.ndim == 2
        a = a[None] if one else a
        assert a.ndim == 3 and a.shape[2] == 4, a.shape
        m, n_cols = a.shape[0], a.shape[1]
        drp, dcol, dval, rows, nnz = self._csr_up(csr)
        n_out = rows if n_out is None else int(n_out)
        dw = self._kzg_polys_up(a) if m and n_cols else None
        dout = self.empty((max(m, 1), 4, max(n_out, 1)))
        if lanes_log < 0:
            self._call("sylow_hip_fr_spmv_batch", drp.ptr, self._ptr(dcol), self._ptr(dval), rows, nnz, self._ptr(dw), n_cols, m, n_out, dout.ptr)
        else:
            self._call("sylow_hip_fr_spmv_batch_tuned", drp.ptr, self._ptr(dcol), self._ptr(dval), rows, nnz, self._ptr(dw), n_cols, m, n_out, int(lanes_log), dout.ptr)
        out = np.ascontiguousarray(dout.download()[:m, :, :n_out].transpose(0, 2, 1))
        return out[0] if one else out

    def groth16_quotient(self, a, b, c):
        """h = the coefficients of the polynomial of degree < n that equals (a b - c) / (X^n - 1) on the coset 5 <w_n>, for a, b, c [m, n, 4]:
        the values of three polynomials on the domain of n = 2^log_n points (sylow_hip_groth16_quotient_batch).  Canonical words [m, n, 4];
        h[n - 1] = 0 where a_i b_i = c_i on the whole domain."""
        a, b, c = (self._kzg_polys(x) for x in (a, b, c))
        m, n = a.shape[0], a.shape[1]
        log_n = n.bit_length() - 1
        assert n == 1 << log_n and b.shape == a.shape and c.shape == a.shape, (a.shape, b.shape, c.shape)
        da, db, dc = (self._kzg_polys_up(x) for x in (a, b, c))
        dh = self.empty((max(m, 1), 4, n))
        self._call("sylow_hip_groth16_quotient_batch", self._ptr(da), self._ptr(db), self._ptr(dc), log_n, m, dh.ptr)
        return np.ascontiguousarray(dh.download()[:m].transpose(0, 2, 1))

    def groth16_prove(self, mats, n_vars, n_inputs, log_n, pk, z, r, s):
        """m proofs for the witnesses z [m, n_vars, 4] of one circuit under one proving key with the caller's randomness r, s [m, 4]
        (sylow_hip_groth16_prove_batch).  mats: the CSR matrices (A, B, C), n_cons rows each; pk: a mapping with alpha_g1, beta_g1, delta_g1
        [1, 8], beta_g2, delta_g2 [1, 16] and the queries a_query, b_g1_query, b_g2_query, h_query, l_query as (words, flags or None).
        Returns ((A [m, 8], flags), (B [m, 16], flags), (C [m, 8], flags)).  Neither z_0 = 1 nor the constraints are checked."""
        z, r, s = np.ascontiguousarray(z, dtype=np.uint64), _aos(r, 4), _aos(s, 4)
        assert z.ndim == 3 and z.shape[2] == 4, z.shape
        m = z.shape[0]
        assert r.shape[0] == m and s.shape[0] == m and z.shape[1] == n_vars
        up = [self._csr_up(x) for x in mats]
        n_cons = up[0][3]
        assert all(u[3] == n_cons for u in up)
        csr_args = [v for u in up for v in (u[0].ptr, self._ptr(u[1]), self._ptr(u[2]), u[4])]
        single = [self.to_device_soa(_aos(pk[k], w), w) for k, w in (("alpha_g1", 8), ("beta_g1", 8), ("delta_g1", 8), ("beta_g2", 16), ("delta_g2", 16))]
        held, query_args = [], []
        for k, w in (("a_query", 8), ("b_g1_query", 8), ("b_g2_query", 16), ("h_query", 8), ("l_query", 8)):
            xy, inf = pk[k]
            xy = _aos(xy, w)
            dxy = self.to_device_soa(xy, w) if xy.shape[0] else None
            dinf = self._flags(inf, xy.shape[0]) if xy.shape[0] else None
            held += [dxy, dinf]
            query_args += [self._ptr(dxy), self._ptr(dinf)]
        dz = self._kzg_polys_up(z)
        dr, ds = (self.to_device_soa(x, 4) if m else None for x in (r, s))
        mm = max(m, 1)
        da, dai, db, dbi, dc, dci = (self.empty((8, mm)), self.empty((mm,), np.uint8), self.empty((16, mm)), self.empty((mm,), np.uint8),
                                     self.empty((8, mm)), self.empty((mm,), np.uint8))
        self._call("sylow_hip_groth16_prove_batch", *csr_args, n_cons, int(n_vars), int(n_inputs), int(log_n), *[d.ptr for d in single], *query_args,
                   self._ptr(dz), self._ptr(dr), self._ptr(ds), m, da.ptr, dai.ptr, db.ptr, dbi.ptr, dc.ptr, dci.ptr)
        return ((self.from_device_soa(da)[:m], dai.download()[:m]), (self.from_device_soa(db)[:m], dbi.download()[:m]),
                (self.from_device_soa(dc)[:m], dci.download()[:m]))

    def bls_aggregate_partial(self, pk_xy, msgs, sig_xy, weights=None, pk_inf=None, sig_inf=None):
        """One shard's raw Miller product of the (weighted) aggregate check, [1, 48] words: the input of fp12_product_final_exp."""
        pk_xy, sig_xy = _aos(pk_xy, 16), _aos(sig_xy, 8)
        n, n_pk = len(msgs), pk_xy.shape[0]
        assert sig_xy.shape[0] == n and n_pk >= 1 and self.aggregate_shape_ok(n, n_pk)
        dpk, dsig = self.to_device_soa(pk_xy, 16), self.to_device_soa(sig_xy, 8)
        dm, doff = self._msgs(msgs)
        dpi, dsi = self._flags(pk_inf, n_pk), self._flags(sig_inf, n)
        df = self.empty((48, 1))
        if weights is None:
            self._call("sylow_hip_bls_aggregate_partial_batch", dpk.ptr, self._ptr(dpi), n_pk, dm.ptr, doff.ptr, dsig.ptr, self._ptr(dsi), n, df.ptr)
        else:
            weights = _aos(weights, 4)
            assert weights.shape[0] == n
            dw = self.to_device_soa(weights, 4)
            self._call("sylow_hip_bls_weighted_partial_batch", dpk.ptr, self._ptr(dpi), n_pk, dm.ptr, doff.ptr, dsig.ptr, self._ptr(dsi), dw.ptr, n, df.ptr)
        return self.from_device_soa(df)

    def bls_verify_same_signer(self, pk_xy, msgs, sig_xy, pk_inf=None, sig_inf=None):
        pk_xy, sig_xy = _aos(pk_xy, 16), _aos(sig_xy, 8)
        assert pk_xy.shape[0] == 1
        n = len(msgs)
        dm, doff = self._msgs(msgs)
        dpk, dsig = self.to_device_soa(pk_xy, 16), self.to_device_soa(sig_xy, 8)
        dpi, dsi = self._flags(pk_inf, 1), self._flags(sig_inf, n)
        dok = self.empty((n,), np.uint8)
        self._call("sylow_hip_bls_verify_same_signer_batch", dpk.ptr, self._ptr(dpi), dm.ptr, doff.ptr, dsig.ptr, self._ptr(dsi), dok.ptr, n)
        return dok.download()

    def g2_line_table(self, pk_xy) -> DeviceArray:
        """Device-resident line table of ONE key (opaque int32 words): build once, reuse across bls_verify_line_table calls."""
        pk_xy = _aos(pk_xy, 16)
        assert pk_xy.shape[0] == 1
        dpk = self.to_device_soa(pk_xy, 16)
        table = self.empty((int(self.lib.sylow_hip_g2_line_table_words()),), np.int32)
        self._call("sylow_hip_g2_line_table", dpk.ptr, 1, 0, table.ptr)
        self.sync()                      # dpk is released when this frame returns
        return table

    def bls_verify_line_table(self, table: DeviceArray, msgs, sig_xy, pk_inf=None, sig_inf=None):
        sig_xy = _aos(sig_xy, 8)
        n = len(msgs)
        dm, doff = self._msgs(msgs)
        dsig = self.to_device_soa(sig_xy, 8)
        dpi, dsi = self._flags(pk_inf, 1), self._flags(sig_inf, n)
        dok = self.empty((n,), np.uint8)
        self._call("sylow_hip_bls_verify_line_table_batch", table.ptr, self._ptr(dpi), dm.ptr, doff.ptr, dsig.ptr, self._ptr(dsi), dok.ptr, n)
        return dok.download()

    def g2_precompute(self, q_xy):
        q_xy = _aos(q_xy, 16)
        n = q_xy.shape[0]
        dq = self.to_device_soa(q_xy, 16)
        dc = self.empty((87 * 24, n))
        self._call("sylow_hip_g2_precompute_batch", dq.ptr, dc.ptr, n)
        return self.from_device_soa(dc)

    def flags_all(self, dflags: DeviceArray) -> int:
        out = self.empty((1,), np.int32)
        self._call("sylow_hip_flags_all", dflags.ptr, dflags.shape[0], out.ptr)
        return int(out.download()[0])

    # ---- Poseidon over Fr (include/sylow_poseidon.h): the circomlib instance, t = 2 .. 17.  The parameter table of a width is kept ON THE
    # DEVICE by the caller; Fr batches are [.., 4] on the host, any 256-bit words taken mod r ----
    def poseidon_table(self, t: int) -> DeviceArray:
        """The parameter table of width t (sylow_poseidon_prepare): the round constants, then M, an element as 4 consecutive words.  Built
        once per width; the call synchronises the stream once."""
        words = int(self.lib.sylow_poseidon_table_words(int(t)))
        if not words:
            raise _lib.SylowHipError(f"poseidon: t = {t} is outside 2 .. 17")
        table = self.empty((words // 4, 4))
        self._call("sylow_poseidon_prepare", int(t), table.ptr)
        return table

    @staticmethod
    def _poseidon_rows(values, width=None):
        a = np.ascontiguousarray(values, dtype=np.uint64)
        assert a.ndim == 3 and a.shape[2] == 4 and (width is None or a.shape[1] == width), a.shape
        return a

    def _poseidon_up(self, a):
        """[n, c, 4] -> device [c][4][n] (None for an empty batch)"""
        return self.to_device(np.ascontiguousarray(a.transpose(1, 2, 0))) if a.shape[0] and a.shape[1] else None

    def poseidon_permute(self, table: DeviceArray, states, route=-1, max_blocks=-1):
        """The permutation of n states [n, t, 4] (sylow_poseidon_permute_batch): canonical words [n, t, 4].  route 0 / 1 pins the narrow /
        the wide kernel and max_blocks >= 1 caps the blocks (sylow_poseidon_permute_batch_tuned); the words depend on neither."""
        a = self._poseidon_rows(states)
        n, t = a.shape[0], a.shape[1]
        din, dout = self._poseidon_up(a), self.empty((t, 4, max(n, 1)))
        if route < 0 and max_blocks < 0:
            self._call("sylow_poseidon_permute_batch", table.ptr, t, self._ptr(din), n, dout.ptr)
        else:
            self._call("sylow_poseidon_permute_batch_tuned", table.ptr, t, self._ptr(din), n, int(route), int(max_blocks), dout.ptr)
        return np.ascontiguousarray(dout.download()[:, :, :n].transpose(2, 0, 1))

    def poseidon_hash(self, table: DeviceArray, inputs, init=None, route=-1, max_blocks=-1):
        """hash(inputs_i) for n rows of k inputs [n, k, 4] under the table of t = k + 1 (sylow_poseidon_hash_batch): canonical words [n, 4].
        init [n, 4]: circomlibjs's initState (None: zeros).  route and max_blocks as for poseidon_permute."""
        a = self._poseidon_rows(inputs)
        n, k = a.shape[0], a.shape[1]
        din, dout = self._poseidon_up(a), self.empty((4, max(n, 1)))
        dinit = None if init is None or not n else self.to_device_soa(_aos(init, 4), 4)
        assert dinit is None or dinit.shape == (4, n), dinit.shape
        if route < 0 and max_blocks < 0:
            self._call("sylow_poseidon_hash_batch", table.ptr, k, self._ptr(din), self._ptr(dinit), n, dout.ptr)
        else:
            self._call("sylow_poseidon_hash_batch_tuned", table.ptr, k, self._ptr(din), self._ptr(dinit), n, int(route), int(max_blocks), dout.ptr)
        return self.from_device_soa(dout)[:n]

    def poseidon_merkle_build_device(self, table3: DeviceArray, dleaves: DeviceArray, depth: int, m: int, wide_max=-1, max_blocks=-1):
        """m trees over device leaves [m][4][2^depth] (sylow_poseidon_merkle_build_batch): device (nodes [m][4][2^depth - 1], roots [4][m])."""
        n = 1 << depth
        dnodes, droot = self.empty((max(m, 1), 4, n - 1)), self.empty((4, max(m, 1)))
        if wide_max < 0 and max_blocks < 0:
            self._call("sylow_poseidon_merkle_build_batch", table3.ptr, self._ptr(dleaves), int(depth), m, dnodes.ptr, droot.ptr)
        else:
            self._call("sylow_poseidon_merkle_build_batch_tuned", table3.ptr, self._ptr(dleaves), int(depth), m, int(wide_max), int(max_blocks), dnodes.ptr, droot.ptr)
        return dnodes, droot

    def poseidon_merkle_build(self, table3: DeviceArray, leaves, wide_max=-1, max_blocks=-1):
        """The nodes of m binary trees over leaves [m, n, 4], n = 2^depth >= 2, node = hash([left, right]): (nodes [m, n - 1, 4], levels 1 ..
        depth one after another with the root last, roots [m, 4]).  wide_max pins the item count up to which a level runs on the wide
        kernel (sylow_poseidon_merkle_build_batch_tuned); the words do not depend on it."""
        a = self._poseidon_rows(leaves)
        m, n = a.shape[0], a.shape[1]
        depth = n.bit_length() - 1
        assert n == 1 << depth and depth >= 1, n
        dleaves = self.to_device(np.ascontiguousarray(a.transpose(0, 2, 1))) if m else None
        dnodes, droot = self.poseidon_merkle_build_device(table3, dleaves, depth, m, wide_max, max_blocks)
        return np.ascontiguousarray(dnodes.download()[:m].transpose(0, 2, 1)), self.from_device_soa(droot)[:m]

    def poseidon_merkle_open(self, dleaves, dnodes, depth: int, m: int, tree, index):
        """The siblings of q leaves of trees held on the device (sylow_poseidon_merkle_open_batch): (siblings [q, depth, 4], level 0 first,
        status [q]: bit 0 = tree or index out of range, the row zeros)."""
        tree, index = (np.ascontiguousarray(x, dtype=np.uint64).reshape(-1) for x in (tree, index))
        q = tree.shape[0]
        assert index.shape[0] == q
        dt, di = (self.to_device(x) if q else None for x in (tree, index))
        dsib, dst = self.empty((int(depth), 4, max(q, 1))), self.empty((max(q, 1),), np.uint8)
        self._call("sylow_poseidon_merkle_open_batch", self._ptr(dleaves), self._ptr(dnodes), int(depth), m, self._ptr(dt), self._ptr(di), q, dsib.ptr, dst.ptr)
        return np.ascontiguousarray(dsib.download()[:, :, :q].transpose(2, 0, 1)), dst.download()[:q]

    def _poseidon_paths_up(self, leaf, index, siblings):
        leaf, index = _aos(leaf, 4), np.ascontiguousarray(index, dtype=np.uint64).reshape(-1)
        sib = self._poseidon_rows(siblings)
        q, depth = leaf.shape[0], sib.shape[1]
        assert index.shape[0] == q and sib.shape[0] == q
        return q, depth, (self.to_device_soa(leaf, 4) if q else None), (self.to_device(index) if q else None), self._poseidon_up(sib)

    def poseidon_merkle_root(self, table3: DeviceArray, leaf, index, siblings):
        """The root each of q paths leads to (sylow_poseidon_merkle_root_batch): leaf [q, 4], index [q], siblings [q, depth, 4] ->
        (roots [q, 4], status [q]); bit k of index set: the node is the right child at level k."""
        q, depth, dl, di, ds = self._poseidon_paths_up(leaf, index, siblings)
        dr, dst = self.empty((4, max(q, 1))), self.empty((max(q, 1),), np.uint8)
        self._call("sylow_poseidon_merkle_root_batch", table3.ptr, self._ptr(dl), self._ptr(di), self._ptr(ds), depth, q, dr.ptr, dst.ptr)
        return self.from_device_soa(dr)[:q], dst.download()[:q]

    def poseidon_merkle_verify(self, table3: DeviceArray, leaf, index, siblings, roots, route=-1, max_blocks=-1):
        """(ok [q], status [q]) for q paths against roots [1, 4] (one root for all) or [q, 4] (sylow_poseidon_merkle_verify_batch): ok_i = the
        recomputed root equals the root mod r, and 0 wherever status is not 0."""
        q, depth, dl, di, ds = self._poseidon_paths_up(leaf, index, siblings)
        roots = _aos(roots, 4)
        droots = self.to_device_soa(roots, 4)
        dok, dst = self.empty((max(q, 1),), np.uint8), self.empty((max(q, 1),), np.uint8)
        if route < 0 and max_blocks < 0:
            self._call("sylow_poseidon_merkle_verify_batch", table3.ptr, self._ptr(dl), self._ptr(di), self._ptr(ds), depth, q, droots.ptr, roots.shape[0], dok.ptr, dst.ptr)
        else:
            self._call("sylow_poseidon_merkle_verify_batch_tuned", table3.ptr, self._ptr(dl), self._ptr(di), self._ptr(ds), depth, q, droots.ptr, roots.shape[0],
                       int(route), int(max_blocks), dok.ptr, dst.ptr)
        return dok.download()[:q], dst.download()[:q]
