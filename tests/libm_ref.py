"""Loader of tests/native/libm_ref.cpp: the host libm and the host build of the restatements as array
functions with clrrt_selftest_math's fn codes, plus the bit comparisons the math tests share."""
import atexit
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_PD = C.POINTER(C.c_double)


@functools.lru_cache(maxsize=None)
def lib():
    td = tempfile.mkdtemp(prefix="libm_ref_")
    atexit.register(shutil.rmtree, td, ignore_errors=True)
    so = os.path.join(td, "libm_ref.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-builtin", "-shared", "-fPIC", "-o", so,
                    os.path.join(HERE, "native", "libm_ref.cpp"), "-lm"], check=True)
    L = C.CDLL(so)
    for name in ("eval_libm", "eval_restated"):
        f = getattr(L, name)
        f.restype = None
        f.argtypes = [C.c_int, C.c_int, _PD, _PD, _PD]
    return L


def _eval(name, fn, a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.zeros_like(a) if b is None else np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape and a.ndim == 1
    out = np.empty_like(a)
    getattr(lib(), name)(fn, len(a), a.ctypes.data_as(_PD), b.ctypes.data_as(_PD), out.ctypes.data_as(_PD))
    return out


def eval_libm(fn, a, b=None):
    return _eval("eval_libm", fn, a, b)


def eval_restated(fn, a, b=None):
    return _eval("eval_restated", fn, a, b)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def mismatches(x, y):
    """Indices where x and y differ in bits; a NaN matches any NaN."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return np.flatnonzero((bits(x) != bits(y)) & ~(np.isnan(x) & np.isnan(y)))


def describe(fn_name, idx, a, b, got, want, what="got"):
    """The first mismatches as text: arguments, the bits under test, libm's bits."""
    rows = [f"{fn_name}({float(a[i])!r} [{float(a[i]).hex()}], {float(b[i])!r}): {what} {int(bits(got)[i]):#018x} "
            f"libm {int(bits(want)[i]):#018x}" for i in idx[:6]]
    return f"{len(idx)} mismatches; " + "; ".join(rows)


def ulp_distance(x, y, single=False):
    """Distance in units of the last place (of float32 if single) between finite values; 0 where both are NaN or
    equal, inf where only one is finite."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if single:
        kx = np.asarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        ky = np.asarray(y, dtype=np.float32).view(np.int32).astype(np.int64)
        kx = np.where(kx < 0, -(kx & 0x7fffffff), kx)
        ky = np.where(ky < 0, -(ky & 0x7fffffff), ky)
    else:
        kx, ky = bits(x).astype(np.int64), bits(y).astype(np.int64)  # sign-magnitude -> a monotone integer line
        kx = np.where(kx < 0, -(kx & 0x7fffffffffffffff), kx)
        ky = np.where(ky < 0, -(ky & 0x7fffffffffffffff), ky)
    d = np.abs(kx.astype(np.float64) - ky.astype(np.float64))
    fin = np.isfinite(x) & np.isfinite(y)
    same = (np.isnan(x) & np.isnan(y)) | (x == y)
    return np.where(same, 0.0, np.where(fin, d, np.inf))
