"""ctypes binding of the feature-export test entries in libathd_ktest.so (csrc/ktest.cpp: kt_export_cf, kt_export_spec)
and their numpy references.  A plain helper module of tests/test_gpu_head.py; the library handle, the guarded device
buffers and the synchronise-or-stop helper are those of tests/ktest.py."""
import ctypes

import numpy as np

import ktest as kt

lib = kt.lib

KtExportCf = kt._struct("KtExportCf", "src src_bf16 nb rows C Cs out".split(), {"src", "out"})
KtExportSpec = kt._struct("KtExportSpec", "specT B Tspec z".split(), {"specT", "z"})
for _n in ("export_cf", "export_spec"):
    getattr(lib, "kt_sizeof_" + _n).restype = ctypes.c_int64
    getattr(lib, "kt_" + _n).argtypes = [ctypes.c_void_p, ctypes.c_void_p]

GUARD = 4096     # elements of sentinel on either side of every buffer


def sizes_match():
    return {"export_cf": (lib.kt_sizeof_export_cf(), ctypes.sizeof(KtExportCf)),
            "export_spec": (lib.kt_sizeof_export_spec(), ctypes.sizeof(KtExportSpec))}


def export_cf(x: np.ndarray, Cs: int, bf16: bool):
    """x: (nb, rows, C) float32 values, or uint16 bf16 bit patterns with bf16=True -> ((nb, Cs, rows) float32 from the
    kernel, whether all four guard bands are intact)"""
    nb, rows, C = x.shape
    src = kt.Buf(x, "bf16" if bf16 else "f32", GUARD)
    out = kt.Buf(np.zeros(nb * Cs * rows, np.float32), "f32", GUARD, output=True)
    d = kt.fill(KtExportCf, src=src.ptr, src_bf16=int(bf16), nb=nb, rows=rows, C=C, Cs=Cs, out=out.ptr)
    rc = lib.kt_export_cf(ctypes.byref(d), None)
    assert rc == 0, rc
    kt.sync()
    got, ok_out = out.host()
    _, ok_src = src.host()
    return got.reshape(nb, Cs, rows), ok_out and ok_src


def export_cf_ref(x: np.ndarray, Cs: int, bf16: bool) -> np.ndarray:
    v = (x.astype(np.uint32) << 16).view(np.float32) if bf16 else x
    return np.ascontiguousarray(v[..., :Cs].transpose(0, 2, 1))


def export_spec(specT: np.ndarray):
    """specT (B, Ts, 2048, 4) float32 -> ((B, 2, 2048, Ts, 2) float32 from the kernel, guard bands intact)"""
    B, Ts = specT.shape[:2]
    src = kt.Buf(specT, "f32", GUARD)
    out = kt.Buf(np.zeros(specT.size, np.float32), "f32", GUARD, output=True)
    d = kt.fill(KtExportSpec, specT=src.ptr, B=B, Tspec=Ts, z=out.ptr)
    rc = lib.kt_export_spec(ctypes.byref(d), None)
    assert rc == 0, rc
    kt.sync()
    got, ok_out = out.host()
    _, ok_src = src.host()
    return got.reshape(B, 2, 2048, Ts, 2), ok_out and ok_src


def export_spec_ref(specT: np.ndarray) -> np.ndarray:
    B, Ts = specT.shape[:2]
    return np.ascontiguousarray(specT.reshape(B, Ts, 2048, 2, 2).transpose(0, 3, 2, 1, 4))
