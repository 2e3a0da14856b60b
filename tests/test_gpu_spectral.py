"""Kernel-level parity of the model's first and last kernels against the float64 references and derived tolerances of
tests/spectral_refs.py, through libathd_ktest.so: the STFT and the fused iSTFT with its boundary join (csrc/spectral.hip),
the time encoder's first conv (csrc/tconv0.hip), the prompt vectors and the position tables (csrc/norm.hip).

The rules of tests/test_gpu_dec.py hold: guard bands on every operand, sentinels in every output (samples past T, the
unused slots of `part` and the padding of specT stay untouched), neighbouring batches, segments and prompts scaled by
different powers of two (tests/spectral_cases.py), every element compared, a sync after each launch.  Both modes of the
transforms run: f32 (double FFT, exact mask arithmetic) and bf16 (float FFT with running-product twiddles, v_exp / v_rcp);
the bf16 mode also has to meet the per-frame / per-hop-block L2 criterion.  A repeated launch of the STFT and of the iSTFT
is bit-identical (they have no atomics but the fp64 statistics).  Each case records max(err / tol) and the L2 ratios in
$ATHD_OUT/kernel_parity_spectral_report.json.
"""
import ctypes

import numpy as np
import pytest

import kernel_refs as kr
import spectral_cases as sc
import spectral_refs as sr
from test_gpu_kernels import _ratio, kt  # noqa: F401  (kt: the module-scoped fixture)

pytestmark = pytest.mark.gpu

MODES = ["f32", "bf16"]


def _rec(kt, case, worst, **kw):
    print("%s: %s %s" % (case, worst, kw))
    kt.record(case, report=kt.SPECTRAL_REPORT, err_over_tol=worst, **kw)
    assert max(worst.values()) <= 1.0, (case, worst)


def _in(kt, vals, kind="f32", guard=4096):
    return kt.Buf(np.asarray(vals, dtype=np.float64 if kind == "f64" else np.float32), kind, guard)


def _out(kt, n, bf16=False, guard=4096):
    init = np.full(n, kt.BF16_SENTINEL_BITS, dtype=np.uint16) if bf16 else np.full(n, kt.F32_SENTINEL, dtype=np.float32)
    return kt.Buf(init, "bf16" if bf16 else "f32", guard, output=True)


def _get(buf, bf16=False):
    raw, bands = buf.host()
    assert bands, "guard band overwritten"
    return raw if bf16 else raw.copy()


@pytest.fixture(scope="module")
def tabs(kt):
    tb = sr.tables()
    tb.d = dict(tw=_in(kt, tb.tw), tw64=_in(kt, tb.tw64, "f64"), win=_in(kt, tb.win), win2=_in(kt, tb.win2))
    return tb


# ================================================================================================================ STFT
# (nb, T, plan): plan None = the product's (kernels.h stft_pad_plan).  (1, 1): a single sample; (2, 600): the zero
# extension (on the right only); the explicit plan: the ext_left branch of pad_sample, which no product plan reaches;
# (1, 1500): Tspec 2; (3, 4096): T a multiple of the hop; (2, 9999): a grid of 10 x 2, so xcd_remap has a remainder
STFT_CASES = [(1, 1, None), (2, 600, None), (2, 600, (600, 1236, 300, 1537)), (1, 1500, None), (3, 4096, None),
              (2, 9999, None)]
_stft_cache = {}


def _stft_case(kt, tabs, nb, T, plan, fast):
    key = (nb, T, plan)
    if key not in _stft_cache:
        _stft_cache.clear()
        Tspec = -(-T // 1024)
        pl = plan or kt.stft_pad_plan(T, Tspec)
        if plan is None:
            assert pl == sr.pad_plan_ref(T)
        _stft_cache[key] = (sc.stft_case(nb, T), Tspec, pl, {})
    wav, Tspec, pl, refs = _stft_cache[key]
    if fast not in refs:
        refs[fast] = sr.stft_ref(wav, pl, Tspec, tabs.win, fast)
    return wav, Tspec, pl, refs[fast]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", STFT_CASES, ids=lambda c: "%d-%d%s" % (c[0], c[1], "-ext_left" if c[2] else ""))
def test_stft(kt, tabs, case, mode):
    nb, T, plan = case
    fast = mode == "bf16"
    wav, Tspec, pl, r = _stft_case(kt, tabs, nb, T, plan, fast)
    bw = _in(kt, wav)
    runs = []
    for _ in range(2):
        bs = _out(kt, nb * Tspec * 2048 * 4)
        bst = kt.Buf(np.zeros(2 * nb), "f64", 64, output=True)
        d = kt.fill(kt.KtStft, wav=bw.ptr, nb=nb, T=T, Tspec=Tspec, tw=tabs.d["tw"].ptr,
                    tw64=None if fast else tabs.d["tw64"].ptr, win=tabs.d["win"].ptr, specT=bs.ptr, stats=bst.ptr,
                    pp_L=pl[0], pp_left=pl[1], pp_ext_left=pl[2], pp_Lx=pl[3])
        assert kt.lib.kt_stft(ctypes.byref(d), None) == 0
        kt.sync()
        st, bands = bst.host()
        assert bands, "guard band overwritten"
        runs.append((_get(bs), st))
    assert (runs[0][0].view(np.uint32) == runs[1][0].view(np.uint32)).all(), "repeat launch differs"
    got = runs[0][0].astype(np.float64).reshape(r.R.shape)
    worst = {"spec": _ratio(got, r.R, r.tol),
             "stats": _ratio(runs[0][1].reshape(nb, 2), r.stats, r.stats_tol)}
    l2 = float(sr.l2_ratio(got, r.R, (2, 3)).max())
    if fast:
        worst["l2"] = l2 / sr.L2_STFT
    _rec(kt, "stft[%s,%d,%d%s]" % (mode, nb, T, ",ext_left" if plan else ""), worst, l2=l2)


# =============================================================================================================== iSTFT
# (Tspec, T, segments, P): a single frame; two frames; T a multiple of the hop; one full workgroup; 17 | 16 with units = 4
# (the padded grid's early return); 22 | 22 | 21 with units = 9 (two XCD rounds, the P prompts of a unit on one XCD);
# 30 workgroups, the last with exactly 3 frames; the split's first rejected candidate: 34 x 29, the last 5
ISTFT_CASES = [(1, 1000, 1, 1), (2, 1500, 1, 1), (3, 3072, 2, 2), (32, 32768, 1, 1), (33, 33297, 2, 2), (65, 66000, 3, 2),
               (931, 931 * 1024 - 5, 1, 1), (962, 962 * 1024 - 700, 1, 1)]
_istft_cache = {}


def _istft_case(tabs, shape, fast):
    if shape not in _istft_cache:
        _istft_cache.clear()
        _istft_cache[shape] = (sc.istft_case(*shape), {})
    c, refs = _istft_cache[shape]
    if fast not in refs:
        refs[fast] = sr.istft_ref(c["fo"], c["spec"], c["xt2"], c["tnorm"], c["P"], c["T"], tabs.win, fast)
    return c, refs[fast]


def test_istft_split_of_cases(kt):
    """the splits the case list is chosen for"""
    sp = lambda t: (kt.lib.kt_istft_nwg(t), kt.lib.kt_istft_frames(t))
    assert sp(32) == (1, 32) and sp(33) == (2, 17) and sp(65) == (3, 22) and sp(931) == (30, 32) and sp(962) == (34, 29)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", ISTFT_CASES, ids=lambda s: "-".join(map(str, s)))
def test_istft(kt, tabs, shape, mode):
    fast = mode == "bf16"
    c, r = _istft_case(tabs, shape, fast)
    Tspec, T, P, NI = c["Tspec"], c["T"], c["P"], c["NI"]
    nwg = kt.lib.kt_istft_nwg(Tspec)
    npart = kt.lib.kt_istft_part_floats(NI, Tspec)
    assert npart == NI * nwg * 12288
    bfo, bsp, bx, bt = (_in(kt, c[k]) for k in ("fo", "spec", "xt2", "tnorm"))
    runs = []
    for _ in range(2):
        bo, bp = _out(kt, NI * 2 * T), _out(kt, npart)
        d = kt.fill(kt.KtIstft, fo=bfo.ptr, NI=NI, Tspec=Tspec, P=P, T=T, spec=bsp.ptr, tw=tabs.d["tw"].ptr,
                    tw64=None if fast else tabs.d["tw64"].ptr, win=tabs.d["win"].ptr, win2=tabs.d["win2"].ptr,
                    xt2=bx.ptr, tnorm=bt.ptr, out=bo.ptr, part=bp.ptr)
        assert kt.lib.kt_istft_ola(ctypes.byref(d), None) == 0
        kt.sync()
        runs.append((_get(bo), _get(bp)))
    assert (runs[0][0].view(np.uint32) == runs[1][0].view(np.uint32)).all(), "repeat launch differs"
    # part[item][k][head, tail][...]: written are the heads of k > 0 and the tails of k < nwg - 1, nothing else
    part = runs[0][1].reshape(NI, nwg, 2, 6144)
    sent = np.float32(kt.F32_SENTINEL)
    assert (part[:, 0, 0] == sent).all() and (part[:, nwg - 1, 1] == sent).all(), "unused partial slots written"
    if nwg > 1:
        assert np.isfinite(part[:, 1:, 0]).all() and (part[:, 1:, 0] != sent).all()
        assert np.isfinite(part[:, :-1, 1]).all() and (part[:, :-1, 1] != sent).all()
    got = runs[0][0].astype(np.float64).reshape(NI, 2, T)
    worst = {"out": _ratio(got, r.R, r.tol)}
    l2 = float(sr.block_l2(got, r.R, r.Rf, T).max())
    if fast:
        worst["l2"] = l2 / sr.L2_ISTFT
    _rec(kt, "istft[%s,%s]" % (mode, ",".join(map(str, shape))), worst, l2=l2, nwg=nwg)


# ============================================================================================================== tconv0
# (B, T): a single partial block with T % 4 = 1; 256 rows less one sample; 257 rows (a second block of one row); three
# blocks, T % 4 = 3
@pytest.mark.parametrize("bf16", [False, True], ids=MODES)
@pytest.mark.parametrize("shape", [(1, 5), (2, 1023), (2, 1025), (3, 2051)], ids=lambda s: "%d-%d" % s)
def test_tconv0(kt, shape, bf16):
    c = sc.tconv0_case(*shape)
    B, T, Lo = c["B"], c["T"], c["Lo"]
    R, tol = sr.tconv0_ref(c["wav"], c["tnorm"], c["w"], c["bias"], bf16)
    bw, bn, bwt, bb = (_in(kt, c[k]) for k in ("wav", "tnorm", "w", "bias"))
    bo = _out(kt, B * Lo * 48, bf16)
    d = kt.fill(kt.KtTconv0, wav=bw.ptr, nb=B, T=T, Lo=Lo, w=bwt.ptr, bias=bb.ptr, tnorm=bn.ptr, out=bo.ptr,
                out_bf16=int(bf16))
    assert kt.lib.kt_tconv0(ctypes.byref(d), None) == 0
    kt.sync()
    raw = _get(bo, bf16)
    got = (kr.bf16_value(raw) if bf16 else raw).astype(np.float64).reshape(R.shape)
    _rec(kt, "tconv0[%s,%d,%d]" % (MODES[bf16], B, T), {"out": _ratio(got, R, tol)})


# ============================================================================================================ text_vec
@pytest.mark.parametrize("shape", [(1, 1, 1), (8, 4, 0), (6, 3, 1)], ids=lambda s: "%d-%d-%d" % s)
def test_text_vec(kt, shape):
    NI, P, per_item = shape
    c = sc.textvec_case(*shape)
    (a, c0, c2), (ta, tc0, tc2) = sr.text_vec_ref(c["text"], NI, P, per_item, c["maT"], c["ma"], c["mcT"], c["mc"], c["b2"])
    ins = {k: _in(kt, c[k]) for k in ("text", "maT", "ma", "mcT", "mc", "b2")}
    for null_c0 in ([False, True] if shape == (8, 4, 0) else [False]):
        outs = [_out(kt, NI * 384, guard=1024) for _ in range(3)]
        d = kt.fill(kt.KtTextVec, NI=NI, P=P, per_item=per_item, a=outs[0].ptr, c0=None if null_c0 else outs[1].ptr,
                    c2=outs[2].ptr, **{k: v.ptr for k, v in ins.items()})
        assert kt.lib.kt_text_vec(ctypes.byref(d), None) == 0
        kt.sync()
        g = [_get(o).astype(np.float64).reshape(NI, 384) for o in outs]
        worst = {"a": _ratio(g[0], a, ta), "c2": _ratio(g[2], c2, tc2)}
        if null_c0:
            assert (g[1] == np.float32(kt.F32_SENTINEL)).all(), "c0 written through a null pointer's neighbour"
        else:
            worst["c0"] = _ratio(g[1], c0, tc0)
        _rec(kt, "text_vec[%d,%d,%d%s]" % (NI, P, per_item, ",c0=null" if null_c0 else ""), worst)


# ===================================================================================================== position tables
@pytest.mark.parametrize("T1", [1, 33, 293])
def test_pos2d(kt, T1):
    R, tol = sr.pos2d_ref(8, T1, 512)
    bo = _out(kt, 8 * T1 * 512)
    assert kt.lib.kt_pos2d(bo.ptr, 8, T1, 512, None) == 0
    kt.sync()
    _rec(kt, "pos2d[8,%d,512]" % T1, {"out": _ratio(_get(bo).astype(np.float64).reshape(R.shape), R, tol)})


@pytest.mark.parametrize("T2", [1, 259, 1145])
def test_pos1d(kt, T2):
    R, tol = sr.pos1d_ref(T2, 512)
    bo = _out(kt, T2 * 512)
    assert kt.lib.kt_pos1d(bo.ptr, T2, 512, None) == 0
    kt.sync()
    _rec(kt, "pos1d[%d,512]" % T2, {"out": _ratio(_get(bo).astype(np.float64).reshape(R.shape), R, tol)})
