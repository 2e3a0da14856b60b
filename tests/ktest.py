"""ctypes binding of libathd_ktest.so (csrc/ktest.cpp): the kernel launchers of libathd.so behind flat descriptors.
A plain helper module of tests/test_gpu_kernels.py, tests/test_gpu_dconv.py, tests/test_gpu_dec.py and
tests/test_gpu_spectral.py (tests/test_gpu_track_kernels.py uses its buffers, sync and report only); importing it needs the built libraries but no GPU (the host-side packers, folds, plans and shape
predicates it exports are compared on the CPU, tests/test_dconv_refs.py, tests/test_dec_refs.py,
tests/test_spectral_refs.py, and the forward's workspace layout, tests/test_workspace_refs.py)."""
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
C3_FIELDS = "x w kp bias h st M L C dil".split()
AP_FIELDS = "hb w kp bias st gn_w gn_b scale x M L C rewrite rw_w rw_kp rw_bias rw_out rw_c4".split()
DS_FIELDS = "x x_bf16 h nb L C dil w3 b3 g1w g1b w1 b1 gram1 g2w g2b scale st_h st_y fast".split()
GM_FIELDS = "h out nb L H stats w b gram st_y".split()
# (the [2] pointer arrays of FencRowDesc as two fields each: name0, name1)
FR_FIELDS = ("in_ a_norm B Fin Fout T wc wc_ld bc w30 w31 w3_ld b30 b31 g1w0 g1w1 g1b0 g1b1 w10 w11 w1_ld b10 b11 "
             "g2w0 g2w1 g2b0 g2b1 gram0 gram1 scale0 scale1 wr wr_ld br row_add out out4 cin c").split()

KtGemm = _struct("KtGemm", GEMM_FIELDS, GEMM_PTRS)
KtAttn = _struct("KtAttn", ATTN_FIELDS, {"Q", "K", "V", "O"})
KtLn = _struct("KtLn", LN_FIELDS, set("x w b gn_stats gn_w gn_b pos out w2 b2 out2".split()))
KtConvT4 = _struct("KtConvT4", CT_FIELDS, set("x w bias out stats".split()))
KtConv3 = _struct("KtConv3", C3_FIELDS, set("x w bias h st".split()))
KtApply = _struct("KtApply", AP_FIELDS, set("hb w bias st gn_w gn_b scale x rw_w rw_bias rw_out rw_c4".split()))
KtDcSmall = _struct("KtDcSmall", DS_FIELDS, set("x h w3 b3 g1w g1b w1 b1 gram1 g2w g2b scale st_h st_y".split()))
KtGnMom = _struct("KtGnMom", GM_FIELDS, set("h out stats w b gram st_y".split()))
KtFencRow = _struct("KtFencRow", FR_FIELDS, set(FR_FIELDS) - set("B Fin Fout T wc_ld w3_ld w1_ld wr_ld cin c".split()))

MG_FIELDS = ("src src_bf16 H_src kept C stats gn_count gn_w gn_b skip skip_bf16 H_skip C_skip P out out_bf16 H_out W NI "
             "proj_w proj_b fast_gelu").split()
LR_FIELDS = ("steps Z Zs z_bf16 z_taps Hs Hk Hd W Co P NI bias stats gn_w gn_b fast_gelu skip skip_bf16 H_skip C_skip out "
             "out_bf16 S Wt w_ld Ci z4 gram gq").split()
DL_FIELDS = ("in_ in_bf16 NI P H W T fold skip skip_bf16 H_skip C_skip out g g_bf16 Hg stats gn_count gn_w gn_b fast_gelu "
             "skip2 skip2_bf16 H_skip2 C_skip2").split()
KtMerge = _struct("KtMerge", MG_FIELDS, set("src stats gn_w gn_b skip out proj_w proj_b".split()))
KtLowRank = _struct("KtLowRank", LR_FIELDS,
                    set("steps Z Zs bias stats gn_w gn_b skip out S Wt z4 gram gq".split()))
KtDecLast = _struct("KtDecLast", DL_FIELDS, set("in_ fold skip out g stats gn_w gn_b skip2".split()))
_DEC = (("merge", KtMerge), ("lowrank", KtLowRank), ("declast", KtDecLast))

_NEW = (("conv3", KtConv3), ("apply", KtApply), ("dcsmall", KtDcSmall), ("gnmom", KtGnMom), ("fencrow", KtFencRow))
for _n in ("gemm", "attn", "ln", "convt4", "lrstep") + tuple(n for n, _ in _NEW + _DEC):
    getattr(lib, "kt_sizeof_" + _n).restype = ctypes.c_int64
lib.kt_sk_bytes.restype = ctypes.c_int64
lib.kt_sk_resident.restype = ctypes.c_int64
lib.kt_sk_resident.argtypes = [ctypes.c_void_p]
lib.kt_sk_plan.restype = None
lib.kt_sk_plan.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
lib.kt_gemm.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
lib.kt_gemm_route.argtypes = [ctypes.c_void_p, ctypes.c_int]
lib.kt_attn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
lib.kt_attn_pp.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
lib.kt_layernorm.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
lib.kt_convt4.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
_P, _I = ctypes.c_void_p, ctypes.c_int64
lib.kt_to_bf16.argtypes = [_P, _P, _I, _P]
lib.kt_stats.argtypes = [_P, _I, _I, _P, _P]
lib.kt_input_norm_params.argtypes = [_P, _I, _I, _P, _P, _P]
lib.kt_gn_gelu.argtypes = [_P, _I, _I, _I, _P, _P, _P, _I, _P]
lib.kt_gn_gelu_bf16.argtypes = [_P, _P, _I, _I, _I, _P, _P, _P, _P]
lib.kt_gn_apply.argtypes = [_P, _I, _I, _I, _P, _P, _P, _P]
for _n in ("dconv_conv3", "dconv_apply", "dconv_small", "gn_gelu_mom", "fenc_row"):
    getattr(lib, "kt_" + _n).argtypes = [_P, _P]
lib.kt_gn_gelu_bf16in.argtypes = [_P, _P, _I, _I, _I, _P, _P, _P, _P]
lib.kt_fenc_row_supported.argtypes = [_I, _I, _I]
lib.kt_dconv_conv3_supported.argtypes = [_I, _I, _I, _I]
lib.kt_dconv_apply_supported.argtypes = [_I, _I, _I, _I]
lib.kt_gn_gelu_mom_supported.argtypes = [_I, _I]
lib.kt_dconv_plan.restype = None
lib.kt_dconv_plan.argtypes = [_I, _I, _I, _I, _I, _P]
for _n in ("glu_src", "rewrite_perm", "host_f2bf"):
    getattr(lib, "kt_" + _n).restype = _I
lib.kt_glu_src.argtypes = [_I, _I]
lib.kt_rewrite_perm.argtypes = [_I]
lib.kt_host_f2bf.argtypes = [_I]
lib.kt_conv1x1_moments.restype = None
lib.kt_conv1x1_moments.argtypes = [_P, _P, _I, _I, _I, _P]

# ---- the decoder kernels and the folded last level ----
for _n in ("dec_merge", "fdec_lr_stats", "fdec_lr_merge", "fdec1_gram", "fdec_last", "tdec_last", "fdec_tail",
           "tdec_tail"):
    getattr(lib, "kt_" + _n).argtypes = [_P, _P]
lib.kt_fdec1_gram_supported.argtypes = [_P]
lib.kt_tdec_tail_supported.argtypes = [_P]
lib.kt_fdec_lr_steps.argtypes = [_P, _I, _I, _I, _I, _P]
for _n in ("fl_dc", "ft_dc", "tl_in", "tt_rows", "dm_run", "merge_maxp", "g_wb", "fdec1_gram_blocks",
           "fdec1_gram_q_doubles"):
    getattr(lib, "kt_" + _n).restype = _I
    getattr(lib, "kt_" + _n).argtypes = []
lib.kt_fdec1_gram_floats.restype = _I
lib.kt_fdec1_gram_floats.argtypes = [_I, _I]
lib.kt_dec_last_fold.restype = _I
lib.kt_dec_last_fold.argtypes = [_P, _P, _P, _P, _I, _P]
lib.kt_convt_rows.restype = _I
lib.kt_convt_rows.argtypes = [_P, _P, _I, _I, _I, _I, _P, _P]
# ---- the spectral front and back end, tconv0, text_vec, the position tables (tests/test_gpu_spectral.py) ----
ST_FIELDS = "wav nb T Tspec tw tw64 win specT stats pp_L pp_left pp_ext_left pp_Lx".split()
IS_FIELDS = "fo NI Tspec P T spec tw tw64 win win2 xt2 tnorm out part".split()
TC_FIELDS = "wav nb T Lo w bias tnorm out out_bf16".split()
TV_FIELDS = "text NI P per_item maT ma mcT mc b2 a c0 c2".split()
KtStft = _struct("KtStft", ST_FIELDS, set("wav tw tw64 win specT stats".split()))
KtIstft = _struct("KtIstft", IS_FIELDS, set("fo spec tw tw64 win win2 xt2 tnorm out part".split()))
KtTconv0 = _struct("KtTconv0", TC_FIELDS, set("wav w bias tnorm out".split()))
KtTextVec = _struct("KtTextVec", TV_FIELDS, set("text maT ma mcT mc b2 a c0 c2".split()))
_SPEC = (("stft", KtStft), ("istft", KtIstft), ("tconv0", KtTconv0), ("textvec", KtTextVec))
for _n, _ in _SPEC:
    getattr(lib, "kt_sizeof_" + _n).restype = _I
for _n in ("stft", "istft_ola", "tconv0", "text_vec"):
    getattr(lib, "kt_" + _n).argtypes = [_P, _P]
lib.kt_stft_pad_plan.restype = None
lib.kt_stft_pad_plan.argtypes = [_I, _I, _P]
for _n in ("istft_nwg", "istft_frames"):
    getattr(lib, "kt_" + _n).restype = _I
    getattr(lib, "kt_" + _n).argtypes = [_I]
lib.kt_istft_part_floats.restype = _I
lib.kt_istft_part_floats.argtypes = [_I, _I]
lib.kt_pos2d.argtypes = [_P, _I, _I, _I, _P]
lib.kt_pos1d.argtypes = [_P, _I, _I, _P]


# ---- the forward's workspace layout (tests/test_workspace_refs.py, tests/test_gpu_workspace.py) ----
lib.kt_set_arena_gap.argtypes = [_P, _I]
lib.kt_forward_layout.restype = _I
lib.kt_forward_layout.argtypes = [ctypes.c_int, _I, _I, _I, ctypes.c_int, _I, _P, _I]
# the buffers of forward_plan.cpp plan(), in its order
LAYOUT_NAMES = ("stats specT snorm tnorm_div tnorm_std saved0 saved_t0 saved1 saved_t1 saved2 saved_t2 saved3 saved_t3 "
                "sk4 sk4t ybuf_t hbuf_t hbuf_b_t ybuf hbuf hbuf_b X XT H0 H1 H2 H3 QKV O F1 QKVt Ot F1t pos2d pos1d "
                "x_enc xt_enc x_enc_b xt_enc_b avec tc0 tc2 Hm Yb Hmt Ybt x_cond xt_cond G D Gt Dt S Z Zs FO FO2 ola_part "
                "lrsteps gram gramq skw0 skw1").split()
DEFAULT_DECODE_ITEMS = 64             # ctx.h athd_ctx::decode_items


def set_arena_gap(ctx, nbytes):
    """unused bytes after every workspace buffer of this native.Context's forwards (0: the product's layout)"""
    assert lib.kt_set_arena_gap(ctx.h, int(nbytes)) == 0


def forward_layout(bf16, B, T, P=1, decode_items=DEFAULT_DECODE_ITEMS, gap=0):
    """plan()'s workspace layout -> ([(name, offset, bytes)] in arena order, total bytes); bytes == 0: a null slot.
    No context and no device.  (make_dims reads ATHD_DECODE_ITEMS: callers that pass decode_items keep it unset.)"""
    cap = 2 * len(LAYOUT_NAMES) + 1
    out = (ctypes.c_int64 * cap)()
    n = lib.kt_forward_layout(int(bool(bf16)), decode_items, B, T, P, gap, out, cap)
    assert n == len(LAYOUT_NAMES), (n, len(LAYOUT_NAMES))
    return [(name, out[2 * i], out[2 * i + 1]) for i, name in enumerate(LAYOUT_NAMES)], out[2 * n]


def stft_pad_plan(T, Tspec):
    """kernels.h stft_pad_plan -> (L, left, ext_left, Lx)"""
    out = (ctypes.c_int64 * 4)()
    lib.kt_stft_pad_plan(T, Tspec, out)
    return tuple(out)


# one LrStep of kernels.h (fdec_lr_steps_launch writes Hd + 1 of them)
LRSTEP = np.dtype([("lz", "<f4"), ("lk", "<f4"), ("lj", "<f4"), ("zk", "<u4"), ("jj", "<u4"), ("flags", "<u4"),
                   ("pad", "<u4", (2,))])


CONVT_PAIR, CONVT_QUAD, CONVT4 = 0, 1, 2


def convt_rows(w, b, form, pi=0):
    """pack.h ConvT residue rows of a weight [cin][cout][8], bias [cout] -> (rows, bias): CONVT_PAIR (pair pi) float32
    [2 cout][2 cin], CONVT_QUAD float32 [4 cout][3 cin], CONVT4 bf16 bits [4 cout][2 cin] with bias None"""
    w = np.ascontiguousarray(w, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    cin, cout = w.shape[:2]
    assert w.shape == (cin, cout, 8) and b.shape == (cout,)
    nres, nrows = ((2, 2), (4, 3), (4, 2))[form]
    rows = np.zeros((nres * cout, nrows * cin), dtype=np.uint16 if form == CONVT4 else np.float32)
    bias = np.zeros(nres * cout, dtype=np.float32)
    n = lib.kt_convt_rows(w.ctypes.data, b.ctypes.data, cin, cout, form, pi, rows.ctypes.data, bias.ctypes.data)
    assert n == rows.size
    return rows, (None if form == CONVT4 else bias)


def dec_last_fold(w, b, P, pb, br):
    """pack.h dec_last_fold: ConvT weight [48][4][8], bias [4], projection [2][4], bias [2], branch -> float32 fold"""
    a = [np.ascontiguousarray(v, dtype=np.float32) for v in (w, b, P, pb)]
    assert a[0].shape == (48, 4, 8) and a[1].shape == (4,) and a[2].shape == (2, 4) and a[3].shape == (2,)
    n = lib.kt_dec_last_fold(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, br, None)
    out = np.zeros(n, dtype=np.float32)
    lib.kt_dec_last_fold(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, br, out.ctypes.data)
    return out


def conv1x1_moments(w, b, round_bf16):
    """pack.h conv1x1_moments of W [N][H], b [N] -> float32 [H*H + 2H + 2]"""
    w = np.ascontiguousarray(w, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    N, H = w.shape
    out = np.zeros(H * H + 2 * H + 2, dtype=np.float32)
    lib.kt_conv1x1_moments(w.ctypes.data, b.ctypes.data, N, H, int(round_bf16), out.ctypes.data)
    return out


PLAN_FIELDS = "ok valu conv3_mfma norm apply_mfma rewrite".split()
NORM_MOM, NORM_BF16, NORM_F32 = 0, 1, 2


def dconv_plan(mode, C, nb, L, rewrite_fusable):
    """kernels.h dconv_plan (mode 0 = f32, 1 = bf16) -> {field: int}; norm is one of NORM_*"""
    out = (ctypes.c_int64 * len(PLAN_FIELDS))()
    lib.kt_dconv_plan(mode, C, nb, L, int(rewrite_fusable), out)
    return dict(zip(PLAN_FIELDS, out))


def sizes_match():
    return {n: (getattr(lib, "kt_sizeof_" + n)(), ctypes.sizeof(s))
            for n, s in (("gemm", KtGemm), ("attn", KtAttn), ("ln", KtLn), ("convt4", KtConvT4)) + _NEW + _DEC + _SPEC}


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
    """wait for the device; a HIP error here (a fault in a kernel under test) ends the whole session, so that no
    further kernel is launched on a device that has faulted"""
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        import pytest
        pytest.exit("HIP error at synchronize; no further kernels are launched: %s" % e, returncode=3)


# ---- the parity report ----
# written to $ATHD_OUT (the measurement scripts' output directory, default bench_out/ in the repository root)
REPORT = os.path.join(os.environ.get("ATHD_OUT") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                 "bench_out"), "kernel_parity_report.json")
DCONV_REPORT = os.path.join(os.path.dirname(REPORT), "kernel_parity_dconv_report.json")
DEC_REPORT = os.path.join(os.path.dirname(REPORT), "kernel_parity_dec_report.json")
SPECTRAL_REPORT = os.path.join(os.path.dirname(REPORT), "kernel_parity_spectral_report.json")
TRACK_REPORT = os.path.join(os.path.dirname(REPORT), "kernel_parity_track_report.json")
WORKSPACE_REPORT = os.path.join(os.path.dirname(REPORT), "workspace_report.json")
_reports = {}


def record(case, report=None, **kw):
    """report: the file this case belongs to (default REPORT); each file holds the cases recorded into it"""
    report = report or REPORT
    rep = _reports.setdefault(report, {})
    rep[case] = kw
    try:
        os.makedirs(os.path.dirname(report), exist_ok=True)
        with open(report, "w") as f:
            json.dump(rep, f, indent=1, sort_keys=True)
    except OSError:
        pass
