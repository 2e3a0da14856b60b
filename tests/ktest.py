"""ctypes binding of libathd_ktest.so (csrc/ktest.cpp): the kernel launchers of libathd.so behind flat descriptors.
A plain helper module of tests/test_gpu_kernels.py; importing it needs the built libraries but no GPU."""
import ctypes
import json
import os

import numpy as np

import athd.native as native          # loads libathd.so first (RTLD_GLOBAL)

LIB_PATH = os.path.join(os.path.dirname(native.LIB_PATH), "libathd_ktest.so")
lib = ctypes.CDLL(LIB_PATH)

ROUTES = ["REFUSED", "ROWLN", "ROWLN_TEXT", "GEMM3_LN", "GEMM2_AGN", "GEMM5", "GEMM3_V3", "GEMM3_V7", "GEMM2",
          "V1_BF16", "V1_F32"]


def _struct(name, fields, pointers):
    return type(name, (ctypes.Structure,),
                {"_fields_": [(f, ctypes.c_void_p if f in pointers else ctypes.c_int64) for f in fields]})


GEMM_FIELDS = ("A a_bf16 nb H_in W C_in a_ld a_cs a_bs a_hs ntaps in_stride in_off dil H_out a_norm a_gn_stats "
               "a_gn_count a_gn_w a_gn_b Wp N K Kp bias C c_bf16 H_out_total o_stride o_off ldo col_off c_bs store c4 "
               "col_split hi_row_off store_mask k_blk act res res_bf16 res_scale res_gn_stats res_gn_count res_gn_w "
               "res_gn_b row_add stats gn_stats gn_count gn_w gn_b pbias pfold res_div res_bs ln_w ln_b ln_out "
               "sk_ws").split()
GEMM_PTRS = set("A a_norm a_gn_stats a_gn_w a_gn_b Wp bias C c4 res res_scale res_gn_stats res_gn_w res_gn_b row_add "
                "stats gn_stats gn_w gn_b pbias ln_w ln_b ln_out sk_ws".split())
ATTN_FIELDS = ("Q q_bf16 q_bs q_ld q_off K k_bf16 k_bs k_ld k_off V v_bf16 v_bs v_ld v_off O o_bf16 o_bs o_ld "
               "nb Nq Nk heads scale_bits").split()
LN_FIELDS = "x nb N C w b gn_stats gn_w gn_b gn_writeback pos out out_bf16 w2 b2 out2".split()
CT_FIELDS = "x w bias out stats nb H W keep".split()

KtGemm = _struct("KtGemm", GEMM_FIELDS, GEMM_PTRS)
KtAttn = _struct("KtAttn", ATTN_FIELDS, {"Q", "K", "V", "O"})
KtLn = _struct("KtLn", LN_FIELDS, set("x w b gn_stats gn_w gn_b pos out w2 b2 out2".split()))
KtConvT4 = _struct("KtConvT4", CT_FIELDS, set("x w bias out stats".split()))

for _n in ("gemm", "attn", "ln", "convt4"):
    getattr(lib, "kt_sizeof_" + _n).restype = ctypes.c_int64
lib.kt_sk_bytes.restype = ctypes.c_int64
lib.kt_sk_resident.restype = ctypes.c_int64
lib.kt_sk_resident.argtypes = [ctypes.c_void_p]
lib.kt_sk_plan.restype = None
lib.kt_sk_plan.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
lib.kt_gemm.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
lib.kt_gemm_route.argtypes = [ctypes.c_void_p, ctypes.c_int]
lib.kt_attn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
lib.kt_layernorm.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
lib.kt_convt4.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
_P, _I = ctypes.c_void_p, ctypes.c_int64
lib.kt_to_bf16.argtypes = [_P, _P, _I, _P]
lib.kt_stats.argtypes = [_P, _I, _I, _P, _P]
lib.kt_input_norm_params.argtypes = [_P, _I, _I, _P, _P, _P]
lib.kt_gn_gelu.argtypes = [_P, _I, _I, _I, _P, _P, _P, _I, _P]
lib.kt_gn_gelu_bf16.argtypes = [_P, _P, _I, _I, _I, _P, _P, _P, _P]
lib.kt_gn_apply.argtypes = [_P, _I, _I, _I, _P, _P, _P, _P]


def sizes_match():
    return {n: (getattr(lib, "kt_sizeof_" + n)(), ctypes.sizeof(s))
            for n, s in (("gemm", KtGemm), ("attn", KtAttn), ("ln", KtLn), ("convt4", KtConvT4))}


GEMM_DEFAULTS = dict(nb=1, H_in=1, W=1, a_cs=1, a_bs=-1, a_hs=-1, ntaps=1, in_stride=1, dil=1, H_out=1, H_out_total=1,
                     o_stride=1, c_bs=-1, store=1, hi_row_off=1, store_mask=3, pfold=1, res_div=1)


def fill(struct, **kw):
    s = struct()
    if struct is KtGemm:
        kw = {**GEMM_DEFAULTS, **kw}
    names = {f for f, _ in struct._fields_}
    for k, v in kw.items():
        if k not in names:
            raise KeyError(k)
        setattr(s, k, v)
    return s


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


# ---- device buffers with guard bands (torch tensors) ----
F32_GUARD = 3.0e38            # operand bands: large and finite (times a zero weight it is still 0)
BF16_GUARD_BITS = 0x7F7F      # 3.39e38
F32_SENTINEL = -7.0e22        # output bands and rows the kernel must not touch
BF16_SENTINEL_BITS = 0xF2F2


class Buf:
    """a device buffer [guard | n elements | guard]; kind 'f32', 'f64' or 'bf16' (uint16 bit patterns on the host)"""

    def __init__(self, host, kind, guard, output=False, fill_value=None):
        import torch
        self.kind, self.guard = kind, int(guard)
        host = np.ascontiguousarray(host).ravel()
        self.n = host.size
        if kind == "bf16":
            band = BF16_SENTINEL_BITS if output else BF16_GUARD_BITS
            full = np.full(self.n + 2 * self.guard, band, dtype=np.uint16)
            full[self.guard:self.guard + self.n] = host.astype(np.uint16)
            self.t = torch.from_numpy(full.view(np.int16)).cuda()
        else:
            dt = np.float32 if kind == "f32" else np.float64
            band = F32_SENTINEL if output else F32_GUARD
            full = np.full(self.n + 2 * self.guard, band, dtype=dt)
            full[self.guard:self.guard + self.n] = host.astype(dt)
            self.t = torch.from_numpy(full).cuda()
        self.band = band
        self.ptr = self.t.data_ptr() + self.guard * self.t.element_size()

    def host(self):
        """(interior, bands_intact)"""
        full = self.t.cpu().numpy()
        if self.kind == "bf16":
            full = full.view(np.uint16)
        g = self.guard
        inner = full[g:g + self.n]
        bands = np.concatenate([full[:g], full[g + self.n:]])
        return inner.copy(), bool((bands == np.array(self.band, dtype=full.dtype)).all())


def sync():
    import torch
    torch.cuda.synchronize()


# ---- the parity report ----
# written to $ATHD_OUT (the measurement scripts' output directory, default bench_out/ in the repository root)
REPORT = os.path.join(os.environ.get("ATHD_OUT") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                 "bench_out"), "kernel_parity_report.json")
_report = {}


def record(case, **kw):
    _report[case] = kw
    try:
        os.makedirs(os.path.dirname(REPORT), exist_ok=True)
        with open(REPORT, "w") as f:
            json.dump(_report, f, indent=1, sort_keys=True)
    except OSError:
        pass
