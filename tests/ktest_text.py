"""ctypes binding of the CLAP text tower's test entries in libathd_ktest.so (csrc/ktest.cpp: kt_tt_gemm, kt_tt_attn) and
their numpy float64 references.  A plain helper module of tests/test_gpu_clap_text.py; the library handle, the guarded
device buffers and the synchronise-or-stop helper are those of tests/ktest.py."""
import ctypes

import numpy as np

import ktest as kt

lib = kt.lib

GEMM_FIELDS = "W bf16 X ldx M N K bias res ldr act part out ldo".split()
ATTN_FIELDS = "part S bias mask P L out".split()
KtTtGemm = kt._struct("KtTtGemm", GEMM_FIELDS, set("W X bias res part out".split()))
KtTtAttn = kt._struct("KtTtAttn", ATTN_FIELDS, set("part bias mask out".split()))
for _n in ("tt_gemm", "tt_attn"):
    getattr(lib, "kt_sizeof_" + _n).restype = ctypes.c_int64
    getattr(lib, "kt_" + _n).argtypes = [ctypes.c_void_p, ctypes.c_void_p]
lib.kt_tt_gemm_plan.restype = ctypes.c_int64
lib.kt_tt_gemm_plan.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]

ACT_NONE, ACT_GELU, ACT_TANH, ACT_RELU = 0, 1, 2, 3
SHAPES = [(2304, 768), (768, 768), (3072, 768), (768, 3072), (512, 768), (512, 512)]     # (N, K)


def sizes_match():
    return {"tt_gemm": (lib.kt_sizeof_tt_gemm(), ctypes.sizeof(KtTtGemm)),
            "tt_attn": (lib.kt_sizeof_tt_attn(), ctypes.sizeof(KtTtAttn))}


def gemm_plan(N, K):
    """{S, W, KW} of the shape's split, or None"""
    out = (ctypes.c_int64 * 3)()
    if not lib.kt_tt_gemm_plan(N, K, out):
        return None
    return dict(zip(("S", "W", "KW"), out))


def bf16_bits(x):
    """float32 array -> uint16 bf16 bit patterns, round to nearest even"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(x):
    """float32 array rounded to bf16, as float32"""
    return (bf16_bits(x).astype(np.uint32) << 16).view(np.float32).reshape(np.shape(x))


def erf64(x):
    import math
    return np.vectorize(math.erf, otypes=[np.float64])(x)


def act64(z, act):
    if act == ACT_GELU:
        return 0.5 * z * (1.0 + erf64(z / np.sqrt(2.0)))
    if act == ACT_TANH:
        return np.tanh(z)
    if act == ACT_RELU:
        return np.maximum(z, 0.0)
    return z
