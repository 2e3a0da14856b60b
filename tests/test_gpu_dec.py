"""Kernel-level parity of the decoder kernels against the float64 references and derived tolerances of
tests/kernel_refs.py, through libathd_ktest.so: the step table and the two passes of the low-rank level 1 (csrc/fdec_lr.hip),
the decoder merges (dec_merge_* of csrc/norm.hip) and the folded last level of both branches with and without the fused
level-2 merge (csrc/dec_last.hip; the fold itself is pack.h dec_last_fold, so fold and kernel are checked together).

The rules of tests/test_gpu_kernels.py and tests/test_gpu_dconv.py hold: guard bands on every operand, sentinels in every
output, neighbouring items and segments scaled by different powers of two (tests/dec_cases.py), |got - R| <= tol for every
element, a sync after each launch, every refusal returns its code with nothing written.  The low-rank passes are staged:
Z is the rounding of a float64 product, the merge pass reads exact statistics.  Shapes are the smallest that reach each
edge; the tile constants come from the library (kt_fl_dc, kt_ft_dc, kt_tl_in, kt_tt_rows, kt_dm_run, kt_merge_maxp), so a
retune moves the edge cases with it.  Each case records max(err / tol) in $ATHD_OUT/kernel_parity_dec_report.json.

The Gram statistics pass (csrc/fdec1f.hip) is checked against the reference on S and Wt themselves, against fdec_lr_stats
on the same operands, for its stored 4-tap Z and for bit-identical repeats.
"""
import ctypes

import numpy as np
import pytest

import dec_cases as dc
import kernel_refs as kr
from test_gpu_kernels import _ratio, kt  # noqa: F401  (kt: the module-scoped fixture)

pytestmark = pytest.mark.gpu


def _rec(kt, case, worst, **kw):
    print("%s: %s" % (case, worst))
    kt.record(case, report=kt.DEC_REPORT, err_over_tol=worst, **kw)
    assert max(worst.values()) <= 1.0, (case, worst)


def _in(kt, vals, bf16, guard=4096):
    v = np.asarray(vals, dtype=np.float32)
    return kt.Buf(kr.bf16_bits(v) if bf16 else v, "bf16" if bf16 else "f32", guard)


def _out(kt, n, bf16=False, guard=4096):
    init = np.full(n, kt.BF16_SENTINEL_BITS, dtype=np.uint16) if bf16 else np.full(n, kt.F32_SENTINEL, dtype=np.float32)
    return kt.Buf(init, "bf16" if bf16 else "f32", guard, output=True)


def _get(buf, bf16=False):
    raw, bands = buf.host()
    assert bands, "guard band overwritten"
    return kr.bf16_value(raw).astype(np.float64) if bf16 else raw.astype(np.float64)


def _untouched(kt, buf, bf16=False):
    raw, bands = buf.host()
    sent = np.uint16(kt.BF16_SENTINEL_BITS) if bf16 else np.float32(kt.F32_SENTINEL)
    return bands and bool((raw == sent).all())


# ===================================================================================================== fdec_lr_steps
# (Hd, Hs, Hk, H_skip): Hd = 1, 2 (the first / last step only), 31 .. 33 around Hs (down, identity, up: the v3 route's
# strict upsampling starts at 33), 49, 259 (the workload), 600 (more entries than the kernel's 256 threads, twice over)
STEP_SHAPES = [(hd, 32, 8, 32) for hd in (1, 2, 31, 32, 33, 49, 259, 600)] + [(33, 32, 8, 128)]


def _steps_run(kt, Hd, Hs, Hk, H_skip, null=False):
    n = max(Hd, 0) + 1
    buf = _out(kt, n * 8, guard=64)
    rc = kt.lib.kt_fdec_lr_steps(None if null else buf.ptr, Hd, Hs, Hk, H_skip, None)
    kt.sync()
    return rc, buf


@pytest.mark.parametrize("shape", STEP_SHAPES)
def test_fdec_lr_steps(kt, shape):
    """all Hd + 1 entries: indices and flags exact, lerp weights bit-equal to lin_index_ref"""
    Hd, Hs, Hk, H_skip = shape
    rc, buf = _steps_run(kt, *shape)
    assert rc == 0
    raw, bands = buf.host()
    assert bands, "guard band overwritten"
    got = raw.view(kt.LRSTEP)
    want = dc.lr_steps_pack(kr.lr_steps_ref(Hd, Hs, Hk, H_skip), kt.LRSTEP)
    for f in ("zk", "jj", "flags"):
        assert (got[f] == want[f]).all(), (f, np.flatnonzero(got[f] != want[f])[:8])
    for f in ("lz", "lk", "lj"):
        assert (got[f].view(np.uint32) == want[f].view(np.uint32)).all(), (f, np.flatnonzero(got[f] != want[f])[:8])
    kt.record("lr_steps[%d,%d,%d,%d]" % shape, report=kt.DEC_REPORT, exact=True)


@pytest.mark.parametrize("what", ["Hs257", "Hd0", "null"])
def test_fdec_lr_steps_refuses(kt, what):
    Hd, Hs = (0 if what == "Hd0" else 33), (257 if what == "Hs257" else 32)
    rc, buf = _steps_run(kt, Hd, Hs, 8, 32, null=what == "null")
    assert rc == -1 and _untouched(kt, buf)
    kt.record("lr_steps_refuses[%s]" % what, report=kt.DEC_REPORT, refused=True)


# ===================================================================================================== fdec_lr passes
# (Hd, W, NI, P, H_skip, C_skip, Co).  Route by dtype: f32 -> stats2<float>, merge2<float, false>; bf16: Hd <= 32 ->
# stats2<bf16>, merge2<bf16, true>; Hd > 32 -> stats3, and merge3 where also Hd > H_skip (8-tap and 4-tap Z), else
# merge2<bf16, true>.  W x Co / 2 threads per item: W = 5 -> 240 (one partial block), 6 -> 288 (the second block partial),
# 11 -> 528; (6, 3) and (8, 4): two segments, the Zs / skip segment mapping.  Hd = 1, 2: first / last step only; 8 = Hk,
# 32 = Hs: identities; 33, 49, 259: strict upsampling.
LR_SHAPES = [(1, 1, 1, 1, 32, 96, 96), (2, 5, 6, 3, 2, 192, 96), (8, 6, 8, 4, 128, 96, 96), (32, 11, 6, 3, 32, 192, 96),
             (33, 6, 6, 3, 33, 96, 96), (33, 11, 8, 4, 32, 192, 96), (49, 5, 8, 4, 128, 192, 96),
             (49, 6, 6, 3, 32, 96, 96), (259, 5, 1, 1, 32, 96, 96), (259, 1, 6, 3, 128, 192, 96),
             (33, 11, 6, 3, 32, 64, 32)]


def _lr_desc(kt, c, bufs, z_taps=8, fast=0, **over):
    kw = dict(steps=bufs["steps"].ptr, Z=bufs["Z"].ptr, Zs=bufs["Zs"].ptr, z_bf16=int(c["z_bf16"]), z_taps=z_taps,
              Hs=c["Hs"], Hk=c["Hk"], Hd=c["Hd"], W=c["W"], Co=c["Co"], P=c["P"], NI=c["NI"], bias=bufs["bias"].ptr,
              stats=bufs["stats"].ptr, gn_w=bufs["gn_w"].ptr, gn_b=bufs["gn_b"].ptr, fast_gelu=fast,
              skip=bufs["skip"].ptr, skip_bf16=int(c["skip_bf16"]), H_skip=c["H_skip"], C_skip=c["C_skip"],
              out=bufs["out"].ptr, out_bf16=int(c["out_bf16"]))
    kw.update(over)
    return kt.fill(kt.KtLowRank, **kw)


def _lr_bufs(kt, c, stats, z_taps=8):
    st = kr.lr_steps_ref(c["Hd"], c["Hs"], c["Hk"], c["H_skip"])
    b = {"steps": kt.Buf(dc.lr_steps_pack(st, kt.LRSTEP).view(np.float32), "f32", 64)}
    Z = dc.z4_pack(c["Z"]) if z_taps == 4 else c["Z"]
    row = c["W"] * 8 * c["Co"]
    b["Z"], b["Zs"] = _in(kt, Z, c["z_bf16"], 2 * row), _in(kt, c["Zs"], c["z_bf16"], 2 * row)
    b["bias"], b["gn_w"], b["gn_b"] = (_in(kt, c[k], False, 64) for k in ("bias", "gn_w", "gn_b"))
    b["skip"] = _in(kt, c["skip"], c["skip_bf16"], 2 * c["W"] * c["C_skip"])
    b["stats"] = kt.Buf(stats, "f64", 64, output=True)
    b["out"] = _out(kt, c["NI"] * c["Hd"] * c["W"] * c["Co"], c["out_bf16"], 2 * c["W"] * c["Co"])
    return b


def _lr_check(kt, c, case, fast, z_taps=8):
    NI, Hd, P = c["NI"], c["Hd"], c["P"]
    v3s, v3m = dc.lr_v3_stats(c), dc.lr_v3_merge(c, fast)
    assert z_taps == 8 or v3m
    Y, tY = kr.fdec_lr_ref(c["Z"], c["Zs"], c["bias"], Hd, P, v3=v3s)
    sref, stol = kr.fdec_lr_stats_ref(Y, tY, Hd)
    worst = {}
    if z_taps == 8:
        st0 = np.stack([1.5 * (np.arange(NI) + 1), -2.0 * (np.arange(NI) + 1)], -1)
        b = _lr_bufs(kt, c, st0)
        rc = kt.lib.kt_fdec_lr_stats(ctypes.byref(_lr_desc(kt, c, b, fast=fast)), None)
        kt.sync()
        assert rc == 0, rc
        st, bands = b["stats"].host()
        assert bands and _untouched(kt, b["out"], c["out_bf16"])
        worst["stats"] = _ratio(st.reshape(NI, 2) - st0, sref, stol + 2.0 ** -50 * np.abs(st0))
    # the merge pass reads its statistics from memory: exact inputs
    if v3m != v3s:
        Y, tY = kr.fdec_lr_ref(c["Z"], c["Zs"], c["bias"], Hd, P, v3=v3m)
    b = _lr_bufs(kt, c, sref, z_taps)
    rc = kt.lib.kt_fdec_lr_merge(ctypes.byref(_lr_desc(kt, c, b, z_taps=z_taps, fast=fast)), None)
    kt.sync()
    assert rc == 0, rc
    st, bands = b["stats"].host()
    assert bands and (st.reshape(NI, 2) == sref).all(), "the merge pass wrote the statistics"
    D1, tD = dc.lr_merge_ref(c, Y, tY, sref, fast=bool(fast), v3=v3m)
    worst["out"] = _ratio(_get(b["out"], c["out_bf16"]), D1.ravel(), tD.ravel())
    _rec(kt, case, worst, route=("stats3" if v3s else "stats2") + "/" + ("merge3" if v3m else "merge2") + "/z%d" % z_taps)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("shape", LR_SHAPES)
def test_fdec_lr(kt, shape, bf16):
    Hd, W, NI, P, H_skip, C_skip, Co = shape
    c = dc.lr_case(100 + Hd + W, NI, P, Hd, W, Co, H_skip, C_skip, bf16)
    _lr_check(kt, c, "fdec_lr[%s,%s]" % ("bf16" if bf16 else "f32", ",".join(map(str, shape))), int(bf16))


@pytest.mark.parametrize("shape", [s for s in LR_SHAPES if s[0] > 32 and s[0] > s[4] and s[6] % 16 == 0])
def test_fdec_lr_merge3_z4(kt, shape):
    """merge3 reading the 4-tap Z rows [w][Co / 16][4][16] (taps 0, 3, 4, 7) that the Gram pass writes"""
    Hd, W, NI, P, H_skip, C_skip, Co = shape
    c = dc.lr_case(100 + Hd + W, NI, P, Hd, W, Co, H_skip, C_skip, True)
    _lr_check(kt, c, "fdec_lr_z4[%s]" % ",".join(map(str, shape)), 1, z_taps=4)


@pytest.mark.parametrize("z_bf16,fast", [(False, 1), (True, 0)])
def test_fdec_lr_merge2_other(kt, z_bf16, fast):
    """the remaining merge2 instantiations: <float, true> (tanh GELU on f32 Z) and <bf16, false> (erf GELU on bf16 Z)"""
    c = dc.lr_case(77, 6, 3, 33, 6, 96, 33, 96, z_bf16)
    _lr_check(kt, c, "fdec_lr_merge2[z_bf16=%d,fast=%d]" % (z_bf16, fast), fast)


@pytest.mark.parametrize("what", ["z4_not_merge3", "C_skip", "odd_Co", "NI_P"])
def test_fdec_lr_refuses(kt, what):
    """-1 with nothing written: z_taps = 4 without the merge3 conditions (here f32 output), C_skip < Co, an odd Co,
    NI % P != 0"""
    c = dc.lr_case(5, 6, 3, 33, 2, 32, 32, 32, True)
    st0 = np.ones((6, 2))
    b = _lr_bufs(kt, c, st0)
    over = {"z4_not_merge3": dict(z_taps=4, out_bf16=0), "C_skip": dict(C_skip=30), "odd_Co": dict(Co=31),
            "NI_P": dict(NI=5)}[what]
    d = _lr_desc(kt, c, b, fast=1, **over)
    rcs = [kt.lib.kt_fdec_lr_merge(ctypes.byref(d), None)]
    if what in ("odd_Co", "NI_P", "z4_not_merge3"):
        rcs.append(kt.lib.kt_fdec_lr_stats(ctypes.byref(d), None))
    kt.sync()
    assert all(rc == -1 for rc in rcs), rcs
    st, bands = b["stats"].host()
    assert bands and (st.reshape(6, 2) == st0).all() and _untouched(kt, b["out"], True)
    kt.record("fdec_lr_refuses[%s]" % what, report=kt.DEC_REPORT, refused=True)


# ===================================================================================================== dec_merge
def _merge_run(kt, c, kept=0, fast=0, out_bf16=None, null_stats=False, **over):
    bf = c["bf16"]
    out_bf16 = bf if out_bf16 is None else out_bf16
    NI, W, C = c["NI"], c["W"], c["C"]
    src = c["src"]
    if kept:                                   # the kernel's buffer holds rows 4d + 1, 4d + 2 as slots 2d, 2d + 1
        rows = np.sort(np.concatenate([np.arange(1, c["H_src"], 4), np.arange(2, c["H_src"], 4)]))
        src = src[:, rows]
    b = dict(src=_in(kt, src, bf, 2 * W * C), skip=_in(kt, c["skip"], bf, 2 * W * c["C_skip"]),
             gn_w=_in(kt, c["gn_w"], False, 64), gn_b=_in(kt, c["gn_b"], False, 64))
    b["stats"] = kt.Buf(c["stats"] if c["stats"] is not None else np.zeros((NI, 2)), "f64", 64)
    proj = c["proj_w"] is not None
    if proj:
        b["pw"], b["pb"] = _in(kt, c["proj_w"], False, 64), _in(kt, c["proj_b"], False, 64)
    n_out = NI * c["H_out"] * W * (2 if proj else C)
    b["out"] = _out(kt, n_out, out_bf16 and not proj, 2 * W * max(C, 8))
    kw = dict(src=b["src"].ptr, src_bf16=int(bf), H_src=c["H_src"], kept=kept, C=C,
              stats=None if (null_stats or c["stats"] is None) else b["stats"].ptr, gn_count=c["gn_count"],
              gn_w=b["gn_w"].ptr, gn_b=b["gn_b"].ptr, skip=b["skip"].ptr, skip_bf16=int(bf), H_skip=c["H_skip"],
              C_skip=c["C_skip"], P=c["P"], out=b["out"].ptr, out_bf16=int(out_bf16 and not proj), H_out=c["H_out"], W=W,
              NI=NI, proj_w=b["pw"].ptr if proj else None, proj_b=b["pb"].ptr if proj else None, fast_gelu=fast)
    kw.update(over)
    rc = kt.lib.kt_dec_merge(ctypes.byref(kt.fill(kt.KtMerge, **kw)), None)
    kt.sync()
    return rc, b


def _merge_check(kt, c, case, kept=0, route=""):
    bf = c["bf16"]
    proj = c["proj_w"] is not None
    rc, b = _merge_run(kt, c, kept=kept, fast=int(bf))
    assert rc == 0, rc
    # the w1 route's tanh GELU runs on the folded affine; the generic route keeps (x - mean) rstd w + b
    w1 = route == "w1"
    R, tol = dc.merge_ref(c, kept=bool(kept), fast=bf, folded=bf and w1, out_bf16=bf and not proj)
    assert np.isfinite(R).all()
    _rec(kt, case, {"out": _ratio(_get(b["out"], bf and not proj), R.ravel(), tol.ravel())}, route=route)


def _dm(kt):
    return kt.lib.kt_dm_run()


# the w1 route (W = 1, P = 4, kept = 0, C % 8 == 0, C_skip >= C): runs of DM_RUN output rows per thread.  H_out = 1,
# DM_RUN - 1, DM_RUN, DM_RUN + 1, 2 DM_RUN + 1 (a last partial run; the run boundary reloads both cached rows); H_src
# above (downsampling: both rows change every step), equal (identity) and below H_out (upsampling: the cached row moves).
def _w1_shapes(dm):
    return [(1, 4, 3), (dm - 1, 4 * (dm - 1), dm - 1), (dm, dm, 5), (dm + 1, 7, 2 * dm), (2 * dm + 1, 40, 2 * dm + 1),
            (2 * dm + 1, 2 * dm + 1, 9)]            # (H_out, H_src, H_skip)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("C", [48, 96, 192])
@pytest.mark.parametrize("i", range(6))
def test_dec_merge_w1(kt, i, C, bf16):
    H_out, H_src, H_skip = _w1_shapes(_dm(kt))[i]
    c = dc.merge_case(200 + i, 8, 4, C, H_src, H_out, H_skip, 1, C + (8 if i % 2 else 0), bf16=bf16)
    _merge_check(kt, c, "dec_merge_w1[%s,C=%d,%d<-%d,skip %d]" % ("bf16" if bf16 else "f32", C, H_out, H_src, H_skip),
                 route="w1")


# the generic route (dec_merge_kernel<8>): (H_out, W, P, NI); P = 4 with W = 2 stays off the w1 route
GEN_SHAPES = [(1, 1, 1, 2), (7, 5, 3, 6), (33, 17, 1, 2), (33, 17, 3, 6), (7, 2, 4, 8)]


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("kept", [0, 1])
@pytest.mark.parametrize("shape", GEN_SHAPES)
def test_dec_merge_generic(kt, shape, kept, bf16):
    """kept = 1 (rows 4d + 1, 4d + 2 only, the exact /4 resize) is not reached from the forward"""
    H_out, W, P, NI = shape
    C = (48, 96, 192)[(H_out + W + kept) % 3]
    H_src = 4 * H_out if kept else (H_out + 3 if H_out % 2 else 2 * H_out + 1)
    c = dc.merge_case(300 + H_out + W, NI, P, C, H_src, H_out, max(1, 2 * H_out - 1), W, 2 * C if W % 2 else C, bf16=bf16)
    _merge_check(kt, c, "dec_merge[%s,C=%d,%dx%d,P=%d,kept=%d]" % ("bf16" if bf16 else "f32", C, H_out, W, P, kept),
                 kept=kept, route="generic")


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("proj", [False, True])
@pytest.mark.parametrize("kept", [0, 1])
def test_dec_merge_c4(kt, kept, proj, bf16):
    """C = 4 (dec_merge_kernel<4>) and the 4 -> 2 projection to FO^T [item][w][ho][2] (dec_merge_proj_kernel): neither is
    reached from the forward (the last level runs folded)"""
    H_out, W = 33, 17
    c = dc.merge_case(400 + kept, 6, 3, 4, 4 * H_out if kept else 50, H_out, 20, W, 8 if kept else 4, bf16=bf16, proj=proj)
    _merge_check(kt, c, "dec_merge_c4[%s,kept=%d,proj=%d]" % ("bf16" if bf16 else "f32", kept, int(proj)), kept=kept,
                 route="proj" if proj else "generic4")


def test_dec_merge_no_stats(kt):
    """stats == nullptr: no GroupNorm and no activation, the resize and the skip only"""
    c = dc.merge_case(500, 4, 2, 48, 9, 7, 5, 3, 48, gn=False)
    _merge_check(kt, c, "dec_merge[no_stats]", route="generic")
    c = dc.merge_case(501, 4, 4, 48, 9, 17, 5, 1, 48, gn=False)
    _merge_check(kt, c, "dec_merge_w1[no_stats]", route="w1")


def test_dec_merge_grid_stride(kt):
    """H_out = W = 300, C = 96, NI = 1: 300 x 300 x 12 threads are more than the 4096-block cap, so the grid-stride loop
    runs a second pass"""
    c = dc.merge_case(600, 1, 1, 96, 150, 300, 75, 300, 96)
    assert 300 * 300 * (96 // 8) > 4096 * 256
    _merge_check(kt, c, "dec_merge[grid_stride]", route="generic")


@pytest.mark.parametrize("what", ["maxp", "NI_P"])
def test_dec_merge_refuses(kt, what):
    maxp = kt.lib.kt_merge_maxp()
    c = dc.merge_case(700, 4, 2, 48, 9, 7, 5, 3, 48)
    over = dict(P=maxp + 1, NI=maxp + 1) if what == "maxp" else dict(NI=3)
    rc, b = _merge_run(kt, c, **over)
    assert rc == -1 and _untouched(kt, b["out"])
    kt.record("dec_merge_refuses[%s]" % what, report=kt.DEC_REPORT, refused=True)


# ===================================================================================================== last level, freq
def _fold_buf(kt, c):
    return _in(kt, kt.dec_last_fold(*c["wts"], c["br"]), False, 64)


def _last_run(kt, c, launcher, x=None, x_bf16=None, tail=False, **over):
    """fdec_last / tdec_last (in = x) or, tail, fdec_tail / tdec_tail (g, statistics, skip2)"""
    bf, br, NI, W = c["bf16"], c["br"], c["NI"], c["W"]
    x_bf16 = bf if x_bf16 is None else x_bf16
    n_out = NI * (W * c["H"] if br == 0 else int(c["T"])) * 2
    b = dict(fold=_fold_buf(kt, c), skip=_in(kt, c["skip"], bf, 2 * W * c["C_skip"]), out=_out(kt, n_out, guard=4096))
    kw = dict(in_bf16=int(x_bf16), NI=NI, P=c["P"], H=c["H"], W=W, T=int(c["T"] or 0), fold=b["fold"].ptr,
              skip=b["skip"].ptr, skip_bf16=int(bf), H_skip=c["H_skip"], C_skip=c["C_skip"], out=b["out"].ptr)
    if tail:
        m = c["merge"]
        g = m["src"]
        if br == 0:
            rows = np.sort(np.concatenate([np.arange(1, 4 * c["H"], 4), np.arange(2, 4 * c["H"], 4)]))
            g = g[:, rows]
        b["g"] = _in(kt, g, bf, 2 * W * 48)
        b["stats"] = kt.Buf(m["stats"], "f64", 64)
        b["gn_w"], b["gn_b"] = _in(kt, m["gn_w"], False, 64), _in(kt, m["gn_b"], False, 64)
        b["skip2"] = _in(kt, m["skip"], bf, 2 * W * m["C_skip"])
        kw.update(g=b["g"].ptr, g_bf16=int(bf), Hg=c["Hg"], stats=b["stats"].ptr, gn_count=m["gn_count"],
                  gn_w=b["gn_w"].ptr, gn_b=b["gn_b"].ptr, fast_gelu=int(bf), skip2=b["skip2"].ptr, skip2_bf16=int(bf),
                  H_skip2=m["H_skip"], C_skip2=m["C_skip"])
    else:
        b["x"] = _in(kt, c["x"] if x is None else x, x_bf16, 2 * W * 48)
        kw["in_"] = b["x"].ptr
    kw.update(over)
    rc = getattr(kt.lib, "kt_" + launcher)(ctypes.byref(kt.fill(kt.KtDecLast, **kw)), None)
    kt.sync()
    return rc, b


def _fl_shapes(fl, ft):
    """(H, W, NI, P, H_skip, C_skip, H_skip2, C_skip2): H = 1, FL_DC - 1, FL_DC, FL_DC + 1, FT_DC - 1, FT_DC, FT_DC + 1,
    2 FT_DC + 1 (chunk edges of fdec_last and fdec_tail, a last chunk of one row); W = 1, 15, 16, 17, 33, 129 (the 16-wide
    w tile of fdec_tail, partial and whole).  (FT_DC + 1, 129): a partial chunk and a partial tile together, 5 regions x 2
    segments = 10 (no multiple of 8: spare blocks return; more than 8: segments share an XCD lane).  nch x W crosses 256
    (fdec_last's second block) at the two W = 129 cases.  H_skip = H, 4 H, 512; H_skip2 = H, 128, 2 H + 1."""
    return [(1, 1, 1, 1, 1, 4, 1, 48), (fl - 1, 17, 3, 1, 4 * (fl - 1), 8, 128, 96), (fl, 15, 6, 3, 512, 4, 2 * fl + 1, 48),
            (fl + 1, 16, 12, 4, fl + 1, 8, fl + 1, 96), (ft - 1, 33, 6, 3, 4 * (ft - 1), 4, 2 * ft - 1, 48),
            (ft, 1, 3, 1, 512, 8, 128, 48), (ft + 1, 129, 6, 3, ft + 1, 4, 2 * ft + 3, 96),
            (2 * ft + 1, 129, 3, 1, 4 * (2 * ft + 1), 8, 2 * ft + 1, 48)]


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("i", range(8))
def test_fdec_last_and_tail(kt, i, bf16):
    """fdec_last (not reached from the forward: it runs fdec_tail) on a given 48-channel input; fdec_tail (the level-2
    merge fused in front) on the level-2 ConvT's kept rows; and the composition dec_merge(kept = 1) -> fdec_last against
    fdec_tail within the sum of both bounds (the two references are the same chain: |Rc - Rt| is float64 noise)"""
    H, W, NI, P, H_skip, C_skip, H_skip2, C_skip2 = _fl_shapes(kt.lib.kt_fl_dc(), kt.lib.kt_ft_dc())[i]
    c = dc.tail_case(800 + i, 0, NI, P, H, W, H_skip, C_skip, H_skip2, C_skip2, bf16=bf16)
    tag = "%s,%dx%d,NI=%d,P=%d" % ("bf16" if bf16 else "f32", H, W, NI, P)
    worst = {}
    rc, b = _last_run(kt, c, "fdec_last")
    assert rc == 0, rc
    R, tol = dc.last_ref(c)
    worst["last"] = _ratio(_get(b["out"]), R.ravel(), tol.ravel())
    rc, b = _last_run(kt, c, "fdec_tail", tail=True)
    assert rc == 0, rc
    Rt, tolt, x, tx = dc.tail_ref(c)
    got_tail = _get(b["out"])
    worst["tail"] = _ratio(got_tail, Rt.ravel(), tolt.ravel())
    # composition: the generic merge (float32 output, no bf16 rounding of x) then fdec_last
    rc, bm = _merge_run(kt, c["merge"], kept=1, fast=int(bf16), out_bf16=False)
    assert rc == 0, rc
    xm, txm = dc.merge_ref(c["merge"], kept=True, fast=bf16)
    xg = _get(bm["out"]).reshape(xm.shape)
    worst["merge"] = _ratio(xg, xm, txm)
    rc, b2 = _last_run(kt, c, "fdec_last", x=xg, x_bf16=False)
    assert rc == 0, rc
    Rc, tolc = dc.last_ref(c, x=xm, d_in=txm)
    worst["comp"] = _ratio(_get(b2["out"]), got_tail, (tolc + tolt + np.abs(Rc - Rt)).ravel())
    _rec(kt, "fdec_last_tail[%s]" % tag, worst)


@pytest.mark.parametrize("what", ["mixed", "C_skip2_40", "null_g", "NI_P"])
def test_fdec_tail_refuses(kt, what):
    c = dc.tail_case(850, 0, 4, 2, 5, 3, 5, 4, 5, 48, bf16=True)
    over = {"mixed": dict(skip2_bf16=0), "C_skip2_40": dict(C_skip2=40), "null_g": dict(g=None), "NI_P": dict(NI=3)}[what]
    rc, b = _last_run(kt, c, "fdec_tail", tail=True, **over)
    assert rc == -1 and _untouched(kt, b["out"])
    if what == "NI_P":
        rc, b = _last_run(kt, c, "fdec_last", **over)
        assert rc == -1 and _untouched(kt, b["out"])
    kt.record("fdec_tail_refuses[%s]" % what, report=kt.DEC_REPORT, refused=True)


# ===================================================================================================== last level, time
def _tl_exact(tl):
    """(H, NI, P, H_skip, C_skip): T = 4 H (tdec_last_kernel: blocks of TL_IN rows + a halo row each side): H = 1, 2,
    TL_IN - 1, TL_IN (one full block), TL_IN + 1 (a second block of one row), 2 TL_IN + 1"""
    return [(1, 1, 1, 4, 4), (2, 3, 1, 3, 8), (tl - 1, 6, 3, 4 * (tl - 1), 4), (tl, 12, 4, 700, 8), (tl + 1, 6, 3, 333, 4),
            (2 * tl + 1, 3, 1, 4 * (2 * tl + 1), 8)]


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("i", range(6))
def test_tdec_last_exact(kt, i, bf16):
    H, NI, P, H_skip, C_skip = _tl_exact(kt.lib.kt_tl_in())[i]
    c = dc.last_case(900 + i, 1, NI, P, H, 1, H_skip, C_skip, bf16=bf16, T=4 * H)
    rc, b = _last_run(kt, c, "tdec_last")
    assert rc == 0, rc
    R, tol = dc.last_ref(c)
    _rec(kt, "tdec_last[%s,H=%d,NI=%d,P=%d]" % ("bf16" if bf16 else "f32", H, NI, P),
         {"out": _ratio(_get(b["out"]), R.ravel(), tol.ravel())}, route="exact")


# the generic kernel (4 H != T, one thread per output sample): T = 4 H - 3, 4 H + 1, 4 H + 5 at H = 1, 64, 255; T = 1 is
# 4 H - 3 at H = 1; 4 x 255 + 5 = 1025 crosses the 256-thread block four times
TG_SHAPES = [(H, 4 * H + dT) for H in (1, 64, 255) for dT in (-3, 1, 5)]


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("H,T", TG_SHAPES)
def test_tdec_last_generic(kt, H, T, bf16):
    NI, P = ((1, 1), (3, 1), (6, 3), (12, 4))[(H + T) % 4]
    c = dc.last_case(950 + H + T, 1, NI, P, H, 1, (T, 4 * T, 77)[T % 3], 4 + 4 * (T % 2), bf16=bf16, T=T)
    rc, b = _last_run(kt, c, "tdec_last")
    assert rc == 0, rc
    R, tol = dc.last_ref(c)
    _rec(kt, "tdec_last[%s,H=%d,T=%d,NI=%d,P=%d]" % ("bf16" if bf16 else "f32", H, T, NI, P),
         {"out": _ratio(_get(b["out"]), R.ravel(), tol.ravel())}, route="generic")


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("dg", [0, 3])
@pytest.mark.parametrize("i", range(6))
def test_tdec_tail(kt, i, dg, bf16):
    """tdec_tail on Hg = H and H + 3 rows of the level-2 ConvT output (Hg = 4 at H = 1), H_skip2 and H_skip off their model
    ratios; the composition dec_merge -> tdec_last against tdec_tail within the sum of both bounds"""
    H, NI, P, H_skip, C_skip = _tl_exact(kt.lib.kt_tl_in())[i]
    Hg = 4 if (H == 1 and dg) else H + dg
    c = dc.tail_case(1000 + i, 1, NI, P, H, 1, H_skip + 1, C_skip, (H + 2, 2 * H + 1)[i % 2], (48, 96)[i % 2], bf16=bf16,
                     Hg=Hg)
    rc, b = _last_run(kt, c, "tdec_tail", tail=True)
    assert rc == 0, rc
    Rt, tolt, x, tx = dc.tail_ref(c)
    got_tail = _get(b["out"])
    worst = {"tail": _ratio(got_tail, Rt.ravel(), tolt.ravel())}
    # composition (P = 4: the w1 merge, else the generic one; float32 x)
    m = c["merge"]
    rc, bm = _merge_run(kt, m, fast=int(bf16), out_bf16=False)
    assert rc == 0, rc
    xm, txm = dc.merge_ref(m, fast=bf16, folded=bf16 and P == 4)
    xg = _get(bm["out"]).reshape(xm.shape)
    worst["merge"] = _ratio(xg, xm, txm)
    rc, b2 = _last_run(kt, c, "tdec_last", x=xg[:, :, 0], x_bf16=False)
    assert rc == 0, rc
    Rc, tolc = dc.last_ref(c, x=xm[:, :, 0], d_in=txm[:, :, 0])
    # (bf16: tdec_tail rounds the activated rows to bf16 in LDS and the composition does not, so the two references
    # differ by that documented rounding: |comp - tail| <= tolc + tolt + |Rc - Rt|; f32: Rc == Rt)
    worst["comp"] = _ratio(_get(b2["out"]), got_tail, (tolc + tolt + np.abs(Rc - Rt)).ravel())
    _rec(kt, "tdec_tail[%s,H=%d,Hg=%d,NI=%d,P=%d]" % ("bf16" if bf16 else "f32", H, Hg, NI, P), worst)


@pytest.mark.parametrize("what", ["T", "span", "mixed"])
def test_tdec_tail_refuses(kt, what):
    """an unsupported shape returns -1 and leaves out at its sentinel: 4 H != T; a block whose g rows exceed TT_ROWS
    (Hg = 2 H at H = 300); mixed dtypes"""
    H = 300 if what == "span" else 9
    Hg = 2 * H if what == "span" else H
    c = dc.tail_case(1100, 1, 4, 2, H, 1, 11, 4, 7, 48, bf16=True, Hg=Hg)
    over = {"T": dict(T=4 * H + 1), "span": {}, "mixed": dict(g_bf16=0)}[what]
    if what == "T":
        c["T"] = 4 * H + 1                     # (the output buffer is sized for it)
    rc, b = _last_run(kt, c, "tdec_tail", tail=True, **over)
    assert rc == -1 and _untouched(kt, b["out"])
    kt.record("tdec_tail_refuses[%s]" % what, report=kt.DEC_REPORT, refused=True)


# ===================================================================================================== fdec1_gram
# (Hd, W, NI, P, w_ld, mean): W = G_WB (one tile per item), G_WB + 1 and 11 (the last tile shifted left, its shared
# columns masked), 2 G_WB, 6 G_WB; (1, 1) at W = G_WB: one tile, most workgroup ranges empty; (8, 4) at W = 6 G_WB: more
# tiles than ranges (asserted from kt_fdec1_gram_blocks), so ranges hold parts of several items; w_ld = 192 and 200;
# mean 30: the large-mean regime
def _gram_shapes(wb):
    return [(33, wb, 1, 1, 192, 0.0), (49, wb + 1, 6, 3, 200, 0.0), (259, 11, 1, 1, 192, 0.0), (33, 2 * wb, 6, 3, 192, 0.0),
            (33, 6 * wb, 8, 4, 200, 0.0), (49, wb + 1, 6, 3, 192, 30.0)]


def _gram_run(kt, c, w_ld):
    NI, W = c["NI"], c["W"]
    wt = np.zeros((8 * 96, w_ld))
    wt[:, :192] = c["Wt"].reshape(8 * 96, 192)
    b = dict(S=_in(kt, c["S"], True, 2 * W * 192), Wt=_in(kt, wt, True, 2 * w_ld), Zs=_in(kt, c["Zs"], True, 2 * W * 768),
             bias=_in(kt, c["bias"], False, 64), z4=_out(kt, NI * 32 * W * 384, True, 2 * W * 384),
             gram=_out(kt, kt.lib.kt_fdec1_gram_floats(NI, W), guard=4096))
    b["stats"] = kt.Buf(np.full((NI, 2), -7.0e22), "f64", 64, output=True)
    b["gq"] = kt.Buf(np.zeros(kt.lib.kt_fdec1_gram_q_doubles()), "f64", 64)
    d = kt.fill(kt.KtLowRank, S=b["S"].ptr, Wt=b["Wt"].ptr, w_ld=w_ld, Ci=192, Zs=b["Zs"].ptr, z_bf16=1, z_taps=4, Hs=32,
                Hk=8, Hd=c["Hd"], W=W, Co=96, P=c["P"], NI=NI, bias=b["bias"].ptr, stats=b["stats"].ptr, z4=b["z4"].ptr,
                gram=b["gram"].ptr, gq=b["gq"].ptr)
    assert kt.lib.kt_fdec1_gram_supported(ctypes.byref(d)) == 1
    rc = kt.lib.kt_fdec1_gram(ctypes.byref(d), None)
    kt.sync()
    assert rc == 0, rc
    st, ok1 = b["stats"].host()
    z4, ok2 = b["z4"].host()
    _, ok3 = b["gram"].host()
    assert ok1 and ok2 and ok3, "guard band overwritten"
    return st.reshape(NI, 2), z4


@pytest.mark.parametrize("i", range(6))
def test_fdec1_gram(kt, i):
    """the statistics against fdec_lr_ref on S and Wt themselves (kernel_refs.fdec1_gram_stats_ref) and against
    fdec_lr_stats on the same operands within the sum of both bounds; the stored 4-tap Z against the GEMM reference
    (equal wherever no rounding tie lies within the K = 192 accumulation bound); two launches bit-identical"""
    wb = kt.lib.kt_g_wb()
    Hd, W, NI, P, w_ld, mean = _gram_shapes(wb)[i]
    tiles, ranges = NI * ((W + wb - 1) // wb), kt.lib.kt_fdec1_gram_blocks() // 6
    if i == 0:
        assert tiles == 1 < ranges
    if i == 4:
        assert tiles > ranges, (tiles, ranges)
    c = dc.gram_case(1200 + i, NI, P, Hd, W, mean=mean)
    st, z4 = _gram_run(kt, c, w_ld)
    sref, stol, _ = kr.fdec1_gram_stats_ref(c["Z"], c["amb"], c["Zs"], c["bias"], Hd, P)
    worst = {"stats": _ratio(st, sref, stol)}
    zr, za = dc.z4_pack(c["Z"]).ravel(), dc.z4_pack(c["amb"]).ravel()
    dz = np.abs(kr.bf16_value(z4).astype(np.float64) - zr)
    assert (dz <= za).all(), "z4: %d elements off the GEMM reference" % int((dz > za).sum())
    worst["z4"] = float((dz / np.maximum(za, 1e-300)).max())
    st2, z4b = _gram_run(kt, c, w_ld)
    assert (st2 == st).all() and (z4b == z4).all(), "two launches differ"
    if i == 4:           # (the largest case: the cross-check below runs at the other five)
        return _rec(kt, "fdec1_gram[Hd=%d,W=%d,NI=%d,P=%d,w_ld=%d,mean=%g]" % (Hd, W, NI, P, w_ld, mean), worst,
                    tiles=tiles, ranges=ranges)
    # fdec_lr_stats (stats3) on the same operands: Z as the 8-tap bf16 rows
    st0 = np.zeros((NI, 2))
    b = _lr_bufs(kt, c, st0)
    rc = kt.lib.kt_fdec_lr_stats(ctypes.byref(_lr_desc(kt, c, b, fast=1)), None)
    kt.sync()
    assert rc == 0, rc
    lr, bands = b["stats"].host()
    Y, tY = kr.fdec_lr_ref(c["Z"], c["Zs"], c["bias"], Hd, P, v3=True)
    s3, t3 = kr.fdec_lr_stats_ref(Y, tY, Hd)
    worst["lr_stats"] = _ratio(lr.reshape(NI, 2), s3, t3)
    worst["gram_vs_lr"] = _ratio(st, lr.reshape(NI, 2), stol + t3)
    _rec(kt, "fdec1_gram[Hd=%d,W=%d,NI=%d,P=%d,w_ld=%d,mean=%g]" % (Hd, W, NI, P, w_ld, mean), worst,
         tiles=tiles, ranges=ranges)


@pytest.mark.parametrize("what", ["W7", "Hd32", "z_taps8", "null_ws"])
def test_fdec1_gram_refuses(kt, what):
    wb = kt.lib.kt_g_wb()
    c = dc.gram_case(1300, 2, 1, 33, wb, mean=0.0)
    over = {"W7": dict(W=wb - 1), "Hd32": dict(Hd=32), "z_taps8": dict(z_taps=8), "null_ws": dict(gram=None)}[what]
    st = kt.Buf(np.full((2, 2), -7.0e22), "f64", 64, output=True)
    z4 = _out(kt, 2 * 32 * wb * 384, True, 4096)
    ins = dict(S=_in(kt, c["S"], True), Wt=_in(kt, c["Wt"], True), Zs=_in(kt, c["Zs"], True), bias=_in(kt, c["bias"], False))
    gram = _out(kt, kt.lib.kt_fdec1_gram_floats(2, wb))
    gq = kt.Buf(np.zeros(kt.lib.kt_fdec1_gram_q_doubles()), "f64", 64)
    kw = dict(S=ins["S"].ptr, Wt=ins["Wt"].ptr, w_ld=192, Ci=192, Zs=ins["Zs"].ptr, z_bf16=1, z_taps=4, Hs=32, Hk=8, Hd=33,
              W=wb, Co=96, P=1, NI=2, bias=ins["bias"].ptr, stats=st.ptr, z4=z4.ptr, gram=gram.ptr, gq=gq.ptr)
    kw.update(over)
    rc = kt.lib.kt_fdec1_gram(ctypes.byref(kt.fill(kt.KtLowRank, **kw)), None)
    kt.sync()
    raw, bands = st.host()
    assert rc == -1 and bands and (raw == -7.0e22).all() and _untouched(kt, z4, True) and _untouched(kt, gram)
    kt.record("fdec1_gram_refuses[%s]" % what, report=kt.DEC_REPORT, refused=True)
