"""Kernel-level parity of the encoder's DConv kernels (csrc/dconv.hip, csrc/dconv_small.hip, gn_gelu_bf16in of csrc/norm.hip)
and the fused encoder rows (csrc/fenc_row.hip) against the float64 references and derived tolerances of
tests/kernel_refs.py, through libathd_ktest.so.

The rules of tests/test_gpu_kernels.py hold: guard bands on every buffer, sentinels in every output and in rows the
kernel must not touch, neighbouring GroupNorm rows scaled by different powers of two (a value taken from the wrong row
is off by at least 2x), every comparison |got - R| <= tol elementwise, every shape computed or refused with its code
and nothing written.  Where a launcher leaves its intermediates in memory the check is staged: each stage's reference
runs on the kernel's own previous-stage output, so no bound has to carry an earlier stage's error.  LayerScale is
U(0.5, 1.5) per channel (the model's 0.05 .. 0.3 would hide the branch), GroupNorm weights 1 + 0.25 N, biases 0.1 N.
Each case records max(err / tol) in $ATHD_OUT/kernel_parity_dconv_report.json (default bench_out/).
"""
import ctypes

import numpy as np
import pytest

import kernel_refs as kr
from test_gpu_kernels import _ratio, _roundup, _vals, kt  # noqa: F401  (kt: the module-scoped fixture)

pytestmark = pytest.mark.gpu

SENT16 = 0xF2F2


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _rowscale(n):
    """a different power of two for neighbouring GroupNorm rows (period 5)"""
    return 2.0 ** (np.arange(n) % 5)


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _rec(kt, case, worst, **kw):
    print("%s: %s" % (case, worst))
    kt.record(case, report=kt.DCONV_REPORT, err_over_tol=worst, **kw)
    assert max(worst.values()) <= 1.0, (case, worst)


def _out16(kt, n, guard):
    init = np.full(n, SENT16, dtype=np.uint16)
    return kt.Buf(init, "bf16", guard, output=True), init


# ===================================================================================================== dconv_conv3
C3_SHAPES = [(1, 16), (3, 17), (5, 31), (2, 64), (3, 259)]
# workgroups per CU and waves per workgroup of dconv_conv3_launch / dconv_apply_launch (csrc/dconv.hip: the tables
# kConv3Grid / kApplyGrid, and kApplyRewriteGrid for the fused rewrite).
# A copy: when a launcher's grid changes, change it here too, or the two-units-per-wave cases stop reaching their path.
DC_GRID = {48: (3, 8), 96: (3, 8), 192: (2, 8), 384: (1, 16)}
RW_GRID = {48: (3, 8), 96: (2, 8)}


def _conv3_weights(C, seed):
    rng = np.random.default_rng(seed)
    H = C // 8
    w3 = kr.bf16_round(rng.standard_normal((H, C, 3)) / np.sqrt(3.0 * C))
    bias = _f32(0.5 * rng.standard_normal(H))
    return w3, bias


def _conv3_run(kt, x, w3, bias, dil, C, L, kp=None, M=None):
    """-> (rc, h [M][HF] raw f32, st [nb][2], st0, h untouched?, bands ok)"""
    H = C // 8
    HF = H if H % 4 == 0 else 8
    rows = _roundup(H, 16)
    kp = kp if kp is not None else _roundup(3 * C, 64)
    wp = np.zeros((rows, max(kp, 3 * C)))
    wp[:, :3 * C] = kr.conv3_pack(w3, rows)
    Mx = x.shape[0] * x.shape[1]
    M = Mx if M is None else M
    nb = max(Mx // L, 1)
    bx = kt.Buf(kr.bf16_bits(x.astype(np.float32)), "bf16", 64 * C)
    bw = kt.Buf(kr.bf16_bits(wp.astype(np.float32)), "bf16", 4096)
    bb = kt.Buf(bias, "f32", 64)
    h0 = np.full(Mx * HF, kt.F32_SENTINEL, dtype=np.float32)
    bh = kt.Buf(h0, "f32", 64 * HF, output=True)
    st0 = np.stack([1.5 * (np.arange(nb) + 1), -2.0 * (np.arange(nb) + 1)], -1)
    bs = kt.Buf(st0, "f64", 64, output=True)
    d = kt.fill(kt.KtConv3, x=bx.ptr, w=bw.ptr, kp=kp, bias=bb.ptr, h=bh.ptr, st=bs.ptr, M=M, L=L, C=C, dil=dil)
    rc = kt.lib.kt_dconv_conv3(ctypes.byref(d), None)
    kt.sync()
    h, b1 = bh.host()
    st, b2 = bs.host()
    assert b1 and b2, "guard band overwritten"
    return rc, h.reshape(Mx, HF), st.reshape(nb, 2), st0


def _conv3_check(kt, C, dil, nb, L, case):
    H = C // 8
    rng = np.random.default_rng(1000 * C + 10 * L + dil + nb)
    w3, bias = _conv3_weights(C, C)
    x = kr.bf16_round((rng.standard_normal((nb, L, C)) + 0.5) * _rowscale(nb)[:, None, None])
    rc, h, st, st0 = _conv3_run(kt, x, w3, bias, dil, C, L)
    assert rc == 0, rc
    R, tol = kr.dconv_conv3_ref(x, w3, bias, dil)
    got = h.astype(np.float64)
    worst = {"h": _ratio(got[:, :H], R.reshape(-1, H), tol.reshape(-1, H))}
    if C == 48:
        assert (h[:, 6:] == 0).all(), "channels 6, 7 of the padded hidden row are not exact zeros"
    sref, stol = kr.conv3_stats_ref(got[:, :H], L)
    worst["st"] = _ratio(st - st0, sref, stol + 2.0 ** -50 * np.abs(st0))
    _rec(kt, case, worst)


@pytest.mark.parametrize("nb,L", C3_SHAPES)
@pytest.mark.parametrize("dil", [1, 2])
@pytest.mark.parametrize("C", [48, 96, 192, 384])
def test_dconv_conv3(kt, C, dil, nb, L):
    """h against conv3 of the input ((3C + 16) e S, the GEMM rule: bf16 operands, f32 accumulation) and the fp64
    {sum, sumsq} per row against sums of the stored h (12 f32 additions per lane, then fp64).  L = 16: every 16-row
    unit is one whole row; L = 17, 31: every unit straddles a row end at a moving offset; M is no multiple of 16."""
    _conv3_check(kt, C, dil, nb, L, "conv3[C=%d,dil=%d,nb=%d,L=%d]" % (C, dil, nb, L))


@pytest.mark.parametrize("C", [48, 96, 192, 384])
def test_dconv_conv3_two_units_per_wave(kt, C):
    """units >= 1.5 x the grid's waves + 5: the launch is capped at its CU-count grid and a wave's contiguous range
    holds one or two units (C = 96, 192: the ping-pong loop prefetches the next unit's first tap across the boundary)"""
    per_cu, nw = DC_GRID[C]
    L = 259
    waves = per_cu * _cus() * nw
    units = (3 * waves + 1) // 2 + 5
    nb = (16 * units + L - 1) // L
    units = (nb * L + 15) // 16
    assert units >= 1.5 * waves + 5 and (units + nw - 1) // nw >= per_cu * _cus() and units < 2 * waves
    _conv3_check(kt, C, 2, nb, L, "conv3_walk[C=%d,units=%d,waves=%d]" % (C, units, waves))


@pytest.mark.parametrize("what", ["L15", "C64", "kp", "M0"])
def test_dconv_conv3_refuses(kt, what):
    """-1 and nothing written: L < 16 (a unit would span three rows), an unsupported C, kp < 3C, M = 0"""
    C, L, kp, M = 48, 16, None, None
    if what == "L15":
        L = 15
    elif what == "C64":
        C = 64
    elif what == "kp":
        kp = 128
    else:
        M = 0
    assert kt.lib.kt_dconv_conv3_supported(C, C // 8, kp or _roundup(3 * C, 64), L) == (1 if what == "M0" else 0)
    w3, bias = _conv3_weights(C, 1)
    x = np.ones((2, L, C))
    rc, h, st, st0 = _conv3_run(kt, x, w3, bias, 1, C, L, kp=kp, M=M)
    assert rc == -1
    assert (h == np.float32(kt.F32_SENTINEL)).all() and (st == st0).all()
    kt.record("conv3_refuses[%s]" % what, report=kt.DCONV_REPORT, refused=True)


# ===================================================================================================== gn_gelu_mom
MOM_SHAPES = [(1, 64), (3, 65), (5, 100), (2, 259)]


def _mom_weights(H, rng):
    """1x1 weights [16 H][H] and a bias with a component along the weights' row sums, so that v = W^T b weighs in the
    second moment (with an uncorrelated bias the 2 v.x term is lost beside x^T G x at H = 48)"""
    w1 = _f32(rng.standard_normal((16 * H, H)) / np.sqrt(H))
    b1 = _f32(0.3 * rng.standard_normal(16 * H) + 0.5 * w1.sum(1) / np.sqrt(H))
    return w1, b1


def _mom_check(kt, H, nb, L, case):
    rng = np.random.default_rng(100 * H + L + nb)
    HF = H if H % 4 == 0 else 8
    OS = H if H % 8 == 0 else 16
    C = 8 * H
    npos = nb * L
    h = (rng.standard_normal((nb, L, H), dtype=np.float32) * _rowscale(nb)[:, None, None].astype(np.float32)
         + np.float32(0.5)).reshape(npos, H)
    h64 = h.astype(np.float64)
    hp = np.full((npos, HF), 1.0e30, dtype=np.float32)        # the padding channels are read but must not be used
    hp[:, :H] = h
    st = kr.group_sums(h64, L)
    w, b = _f32(1 + 0.25 * rng.standard_normal(H)), _f32(0.1 * rng.standard_normal(H))
    w1, b1 = _mom_weights(H, rng)
    gram = kt.conv1x1_moments(w1, b1, True)
    bh = kt.Buf(hp, "f32", 256 * HF)
    bo, _ = _out16(kt, npos * OS, 256 * OS)
    bs, bw, bb, bg = kt.Buf(st, "f64", 64), kt.Buf(w, "f32", 64), kt.Buf(b, "f32", 64), kt.Buf(gram, "f32", 64)
    sy0 = np.stack([0.5 * (np.arange(nb) + 1), -1.0 * (np.arange(nb) + 1)], -1)
    by = kt.Buf(sy0, "f64", 64, output=True)
    d = kt.fill(kt.KtGnMom, h=bh.ptr, out=bo.ptr, nb=nb, L=L, H=H, stats=bs.ptr, w=bw.ptr, b=bb.ptr, gram=bg.ptr,
                st_y=by.ptr)
    rc = kt.lib.kt_gn_gelu_mom(ctypes.byref(d), None)
    kt.sync()
    assert rc == 0, rc
    out, b1ok = bo.host()
    sy, b2ok = by.host()
    assert b1ok and b2ok, "guard band overwritten"
    out = out.reshape(npos, OS)
    assert (out[:, H:] == 0).all(), "output row padding is not exact zeros"
    x = _vals(out[:, :H], True)
    R, tol = kr.gn_gelu_ref(h64, L, st, w, b)
    worst = {"out": _ratio(x, R, tol)}
    sref, stol = kr.moment_stats_ref(x, L, kr.bf16_round(w1), b1)
    worst["st_y"] = _ratio(sy.reshape(nb, 2) - sy0, sref, stol + 2.0 ** -50 * np.abs(sy0))
    _rec(kt, case, worst)


@pytest.mark.parametrize("nb,L", MOM_SHAPES)
@pytest.mark.parametrize("H", [6, 12, 24, 48])
def test_gn_gelu_mom(kt, H, nb, L):
    """out = bf16(GELU_fast(GN(h))) (input stride 8 / 12 / 24 / 48, output stride 16 / 16 / 24 / 48 with exact zero
    padding) with the parent's gn_gelu_bf16 rule, and st_y against the statistics of y = W1 x + b1 evaluated from the
    stored bf16 row x (moment-form rule).  Row ends fall inside waves; npos is a multiple of neither 64 nor 256."""
    _mom_check(kt, H, nb, L, "gn_gelu_mom[H=%d,nb=%d,L=%d]" % (H, nb, L))


@pytest.mark.parametrize("H,R", [(6, 2), (12, 2), (6, 4)])
def test_gn_gelu_mom_multipass(kt, H, R):
    """npos >= R 2048 256 + 100: the launcher gives every workgroup R passes of 256 positions (R = 4 is the workload's)"""
    L = 4099
    nb = (R * 2048 * 256 + 100 + L - 1) // L
    passes = (nb * L + 255) // 256
    assert max(1, min(4, passes // 2048)) == R           # gn_gelu_mom_launch's own formula
    _mom_check(kt, H, nb, L, "gn_gelu_mom_R[H=%d,R=%d]" % (H, R))


@pytest.mark.parametrize("H,L", [(6, 63), (8, 64)])
def test_gn_gelu_mom_refuses(kt, H, L):
    """-1 and nothing written: L < 64 (a wave would span three rows), H outside {6, 12, 24, 48}"""
    npos = 2 * L
    bh = kt.Buf(np.ones(npos * 8), "f32", 256)
    bo, init = _out16(kt, npos * 16, 256)
    one = kt.Buf(np.ones(4096), "f32", 64)
    bs = kt.Buf(np.ones(4), "f64", 64)
    sy0 = np.ones(4)
    by = kt.Buf(sy0, "f64", 64, output=True)
    d = kt.fill(kt.KtGnMom, h=bh.ptr, out=bo.ptr, nb=2, L=L, H=H, stats=bs.ptr, w=one.ptr, b=one.ptr, gram=one.ptr,
                st_y=by.ptr)
    assert kt.lib.kt_gn_gelu_mom(ctypes.byref(d), None) == -1
    kt.sync()
    out, b1 = bo.host()
    sy, b2 = by.host()
    assert b1 and b2 and (out == init).all() and (sy == sy0).all()
    kt.record("gn_gelu_mom_refuses[H=%d,L=%d]" % (H, L), report=kt.DCONV_REPORT, refused=True)


@pytest.mark.parametrize("rows", [8 * 31, 8 * 257])
def test_gn_gelu_bf16in(kt, rows):
    """gn_gelu_bf16's rule with the bf16 input exact; H = 192 over [nb][rows / 8 ... ][24 x 8] as the forward uses it
    (per_batch = 8 x {31, 257} x 24)"""
    nb, H = 3, 192
    per = rows * 24
    rng = np.random.default_rng(rows)
    h = kr.bf16_round((rng.standard_normal((nb, per // H, H)) + 0.5) * _rowscale(nb)[:, None, None]).reshape(nb, per)
    st = np.stack([h.sum(1), (h * h).sum(1)], -1)
    w, b = _f32(1 + 0.25 * rng.standard_normal(H)), _f32(0.1 * rng.standard_normal(H))
    bh = kt.Buf(kr.bf16_bits(h.astype(np.float32)), "bf16", 4096)
    bo, _ = _out16(kt, nb * per, 4096)
    bs, bw, bb = kt.Buf(st, "f64", 64), kt.Buf(w, "f32", 64), kt.Buf(b, "f32", 64)
    assert kt.lib.kt_gn_gelu_bf16in(bh.ptr, bo.ptr, nb, per, H, bs.ptr, bw.ptr, bb.ptr, None) == 0
    kt.sync()
    out, ok = bo.host()
    assert ok, "guard band overwritten"
    m, r = kr.gn_params(st, per)
    hv = h.reshape(nb, per // H, H)
    c = (hv - m[:, None, None]) * r[:, None, None] * w
    v = c + b
    vt = 4 * kr.E32 * (np.abs(c) + np.abs(b) + np.abs(m[:, None, None]) * r[:, None, None] * np.abs(w))
    y, tol = kr.gelu_step(v, vt, True)
    tol = tol + kr.hulp16(np.abs(y) + tol)
    _rec(kt, "gn_gelu_bf16in[%d]" % rows, {"out": _ratio(_vals(out, True), y.ravel(), tol.ravel())})


# ===================================================================================================== dconv_apply
def _apply_weights(C, seed, rewrite=False):
    rng = np.random.default_rng(seed)
    H = C // 8
    p = dict(w1=kr.bf16_round(rng.standard_normal((2 * C, H)) / np.sqrt(H)), b1=_f32(0.3 * rng.standard_normal(2 * C)),
             g2w=_f32(1 + 0.25 * rng.standard_normal(2 * C)), g2b=_f32(0.1 * rng.standard_normal(2 * C)),
             scale=_f32(rng.uniform(0.5, 1.5, C)))
    if rewrite:
        p["wr"] = kr.bf16_round(rng.standard_normal((2 * C, C)) / np.sqrt(C))
        p["br"] = _f32(0.3 * rng.standard_normal(2 * C))
    return p


def _apply_inputs(C, M, L, seed):
    rng = np.random.default_rng(seed)
    H = C // 8
    rs = _rowscale((M + L - 1) // L)[np.arange(M) // L][:, None]
    hb = kr.bf16_round(kr.gelu(rng.standard_normal((M, H)) + 0.3) * rs)
    x = kr.bf16_round((rng.standard_normal((M, C)) + 0.25) * rs)
    return hb, x


def _apply_run(kt, C, M, L, p, hb, x, st, kp=64, rewrite=None, c4=False, M_arg=None):
    """rewrite: None or the rw.kp to pass.  -> (rc, x bits [M + 16][C], x init, out bits, out init, c4 bits, c4 init)"""
    H = C // 8
    HS = H if H % 8 == 0 else 16
    hp = np.zeros((M, HS))
    hp[:, :H] = hb
    bhb = kt.Buf(kr.bf16_bits(hp.astype(np.float32)), "bf16", 64 * HS)
    wp = np.zeros((2 * C, max(kp, 64)))
    wp[:, :64] = kr.conv1x1_pack(p["w1"])
    bw = kt.Buf(kr.bf16_bits(wp.astype(np.float32)), "bf16", 4096)
    f = lambda a: kt.Buf(a, "f32", 64)
    bb, bgw, bgb, bsc = f(kr.glu_order(p["b1"])), f(kr.glu_order(p["g2w"])), f(kr.glu_order(p["g2b"])), f(p["scale"])
    bst = kt.Buf(st, "f64", 64)
    x0 = np.full((M + 16, C), SENT16, dtype=np.uint16)          # rows >= M: sentinels the kernel must not touch
    x0[:M] = kr.bf16_bits(x.astype(np.float32))
    bx = kt.Buf(x0, "bf16", 64 * C, output=True)
    d = dict(hb=bhb.ptr, w=bw.ptr, kp=kp, bias=bb.ptr, st=bst.ptr, gn_w=bgw.ptr, gn_b=bgb.ptr, scale=bsc.ptr, x=bx.ptr,
             M=M if M_arg is None else M_arg, L=L, C=C)
    bo = bc = None
    o0 = c0 = None
    keep = []
    if rewrite is not None:
        rp = kr.rewrite_pack(p["wr"])
        rkp = max(rewrite, rp.shape[1])
        rpp = np.zeros((2 * C, rkp))
        rpp[:, :rp.shape[1]] = rp
        brw = kt.Buf(kr.bf16_bits(rpp.astype(np.float32)), "bf16", 4096)
        brb = f(kr.glu_order(p["br"]))
        bo, o0 = _out16(kt, (M + 16) * C, 64 * C)
        d.update(rewrite=1, rw_w=brw.ptr, rw_kp=rewrite, rw_bias=brb.ptr, rw_out=bo.ptr)
        keep += [brw, brb]
        if c4:
            bc, c0 = _out16(kt, (M + 16) * 4, 256)
            d.update(rw_c4=bc.ptr)
    rc = kt.lib.kt_dconv_apply(ctypes.byref(kt.fill(kt.KtApply, **d)), None)
    kt.sync()
    xg, ok = bx.host()
    assert ok, "guard band of x overwritten"
    og = cg = None
    if bo is not None:
        og, ok = bo.host()
        assert ok, "guard band of out overwritten"
    if bc is not None:
        cg, ok = bc.host()
        assert ok, "guard band of c4 overwritten"
    return rc, xg.reshape(M + 16, C), x0, og, o0, cg, c0


def _apply_check(kt, C, M, L, case, rewrite=False, c4=False):
    p = _apply_weights(C, C, rewrite)
    hb, x = _apply_inputs(C, M, L, 7 * C + 1000 * L + M)
    st = kr.group_sums(hb @ p["w1"].T + p["b1"], L)           # the 1x1 output's statistics, as the pass before writes
    rc, xg, x0, og, o0, cg, c0 = _apply_run(kt, C, M, L, p, hb, x, st, rewrite=_roundup(C, 64) if rewrite else None,
                                            c4=c4)
    assert rc == 0, rc
    R, tv, ts = kr.dconv_apply_ref(hb, None, p["w1"], p["b1"], st, L, p["g2w"], p["g2b"], p["scale"], x, True, True)
    assert (xg[M:] == SENT16).all(), "rows >= M of x were written"
    worst = {}
    if not rewrite:
        worst["x"] = _ratio(_vals(xg[:M], True), R, ts)
    else:
        assert (xg == x0).all(), "the fused form must leave x as it is"
        Ro, to = kr.dconv_rewrite_ref(R, tv, p["wr"], p["br"])
        og = og.reshape(M + 16, C)
        assert (og[M:] == SENT16).all(), "rows >= M of out were written"
        worst["out"] = _ratio(_vals(og[:M], True), Ro, to)
        if c4:
            cg = cg.reshape(M + 16, 4)
            assert (cg[M:] == SENT16).all() and np.array_equal(cg[:M], og[:M, :4]), "c4 != channels 0..3 of out"
    _rec(kt, case, worst)


@pytest.mark.parametrize("L", [1, 5, 16, 17, 64])
@pytest.mark.parametrize("C", [48, 96, 192, 384])
def test_dconv_apply(kt, C, L):
    """x += scale GLU(GN(W1 hb + b1)) in place for M in {1, 15, 16, 17, 100}; the GroupNorm row index is per lane, so
    rows of L = 1 and 5 positions work too.  Rows >= M keep their sentinels."""
    for M in (1, 15, 16, 17, 100):
        _apply_check(kt, C, M, L, "apply[C=%d,L=%d,M=%d]" % (C, L, M))


@pytest.mark.parametrize("C", [48, 96, 192, 384])
def test_dconv_apply_two_units_per_wave(kt, C):
    """units >= 1.5 x the grid's waves + 5: waves take one and two units of the grid-stride loop"""
    per_cu, nw = DC_GRID[C]
    waves = per_cu * _cus() * nw
    units = (3 * waves + 1) // 2 + 5
    M = 16 * units - 3
    assert (M + 15) // 16 >= 1.5 * waves + 5 and (units + nw - 1) // nw >= per_cu * _cus()
    _apply_check(kt, C, M, 64, "apply_walk[C=%d,units=%d,waves=%d]" % (C, units, waves))


@pytest.mark.parametrize("c4", [0, 1])
@pytest.mark.parametrize("L,M", [(1, 1), (5, 17), (16, 100), (17, 15), (64, 16)])
@pytest.mark.parametrize("C", [48, 96])
def test_dconv_apply_rewrite(kt, C, L, M, c4):
    """the fused rewrite: x unchanged, out = GLU(Wr bf16(x_new) + br) with x_new known to the apply bound (an element
    within that bound of a bf16 tie gets one ulp times |Wr|), c4 = channels 0..3 of out bit for bit"""
    _apply_check(kt, C, M, L, "apply_rw[C=%d,L=%d,M=%d,c4=%d]" % (C, L, M, c4), rewrite=True, c4=bool(c4))


@pytest.mark.parametrize("C", [48, 96])
def test_dconv_apply_rewrite_two_units_per_wave(kt, C):
    per_cu, nw = RW_GRID[C]
    waves = per_cu * _cus() * nw
    units = (3 * waves + 1) // 2 + 5
    M = 16 * units - 5
    assert (M + 15) // 16 >= 1.5 * waves + 5 and (units + nw - 1) // nw >= per_cu * _cus()
    _apply_check(kt, C, M, 17, "apply_rw_walk[C=%d,units=%d,waves=%d]" % (C, units, waves), rewrite=True, c4=True)


@pytest.mark.parametrize("what", ["kp", "rw192", "rwkp", "M0"])
def test_dconv_apply_refuses(kt, what):
    """-1 and nothing written: kp != 64, the rewrite at C = 192, rw.kp < roundup(C, 32), M = 0"""
    C, kp, rewrite, M_arg = 48, 64, None, None
    if what == "kp":
        kp = 128
    elif what == "rw192":
        C, rewrite = 192, 192
    elif what == "rwkp":
        rewrite = 32
    else:
        M_arg = 0
    M, L = 20, 16
    assert kt.lib.kt_dconv_apply_supported(C, C // 8, kp, M if M_arg is None else M_arg) == (1 if what in ("rw192", "rwkp") else 0)
    p = _apply_weights(C, 1, rewrite is not None)
    hb, x = _apply_inputs(C, M, L, 1)
    st = kr.group_sums(hb @ p["w1"].T + p["b1"], L)
    rc, xg, x0, og, o0, cg, c0 = _apply_run(kt, C, M, L, p, hb, x, st, kp=kp, rewrite=rewrite, c4=rewrite is not None,
                                            M_arg=M_arg)
    assert rc == -1
    assert (xg == x0).all()
    if og is not None:
        assert (og == o0).all() and (cg == c0).all()
    kt.record("apply_refuses[%s]" % what, report=kt.DCONV_REPORT, refused=True)


# ===================================================================================================== dconv_small
DS_SHAPES = [(7, 1), (5, 2), (40, 7), (9, 31), (3, 255), (2, 256), (3, 257), (2, 300)]


def _small_run(kt, C, xb, fast, dil, x, L, p, gram=True):
    nb = x.shape[0]
    H = C // 8
    P = nb * L
    f = lambda a: kt.Buf(a, "f32", 256)
    if xb:
        x0 = kr.bf16_bits(x.astype(np.float32)).ravel()
        bx = kt.Buf(x0, "bf16", 260 * C, output=True)
    else:
        x0 = x.astype(np.float32).ravel()
        bx = kt.Buf(x0, "f32", 132 * C, output=True)
    h0 = np.full(P * H, kt.F32_SENTINEL, dtype=np.float32)
    bh = kt.Buf(h0, "f32", 256 * H, output=True)
    bw3, bb3, bg1w, bg1b = f(kr.conv3_pack(p["w3"])), f(p["b3"]), f(p["g1w"]), f(p["g1b"])
    bw1, bb1, bg2w, bg2b, bsc = f(p["w1"]), f(p["b1"]), f(p["g2w"]), f(p["g2b"]), f(p["scale"])
    bgr = f(kt.conv1x1_moments(p["w1"], p["b1"], False))
    bsh = kt.Buf(np.zeros(2 * nb), "f64", 64, output=True)
    bsy = kt.Buf(np.zeros(2 * nb), "f64", 64, output=True)
    d = kt.fill(kt.KtDcSmall, x=bx.ptr, x_bf16=int(xb), h=bh.ptr, nb=nb, L=L, C=C, dil=dil, w3=bw3.ptr, b3=bb3.ptr,
                g1w=bg1w.ptr, g1b=bg1b.ptr, w1=bw1.ptr, b1=bb1.ptr, gram1=bgr.ptr if gram else None, g2w=bg2w.ptr,
                g2b=bg2b.ptr, scale=bsc.ptr, st_h=bsh.ptr, st_y=bsy.ptr, fast=int(fast))
    rc = kt.lib.kt_dconv_small(ctypes.byref(d), None)
    kt.sync()
    outs = []
    for b in (bx, bh, bsh, bsy):
        v, ok = b.host()
        assert ok, "guard band overwritten"
        outs.append(v)
    return rc, outs, x0, h0


def _small_weights(C, seed):
    rng = np.random.default_rng(seed)
    H = C // 8
    return dict(w3=_f32(rng.standard_normal((H, C, 3)) / np.sqrt(3.0 * C)), b3=_f32(0.5 * rng.standard_normal(H)),
                g1w=_f32(1 + 0.25 * rng.standard_normal(H)), g1b=_f32(0.1 * rng.standard_normal(H)),
                w1=_f32(rng.standard_normal((2 * C, H)) / np.sqrt(H)), b1=_f32(0.3 * rng.standard_normal(2 * C)),
                g2w=_f32(1 + 0.25 * rng.standard_normal(2 * C)), g2b=_f32(0.1 * rng.standard_normal(2 * C)),
                scale=_f32(rng.uniform(0.5, 1.5, C)))


@pytest.mark.parametrize("dil", [1, 2])
@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("xb", [0, 1])
@pytest.mark.parametrize("C", [48, 96])
def test_dconv_small(kt, C, xb, fast, dil):
    """One DConv layer of the narrow levels, staged on the launcher's own intermediates: h against conv3 of the input
    ((3C + 16) e S), st_h against sums of the stored h, st_y against the 1x1 output's statistics of GELU(GN(stored h;
    stored st_h)) (moment-form rule with the hidden values' bound), x from stored h, st_h, st_y.  L = 1, 2: every tap
    but the centre is padding at dil = 2; L <= 31: more than GN_TAB rows per block (per-thread parameters); L < 256:
    per-thread atomics; L >= 256: the two-row block reduction with a row end inside a block; nb L is no multiple of
    the tile."""
    H = C // 8
    p = _small_weights(C, C + fast)
    for nb, L in DS_SHAPES:
        rng = np.random.default_rng(100 * L + nb + dil)
        x = (rng.standard_normal((nb, L, C)) + 0.25) * _rowscale(nb)[:, None, None]
        x = kr.bf16_round(x) if xb else _f32(x)
        rc, (xg, hg, sh, sy), x0, h0 = _small_run(kt, C, xb, fast, dil, x, L, p)
        assert rc == 0, rc
        P = nb * L
        h = hg.astype(np.float64).reshape(P, H)
        R, tol = kr.dconv_conv3_ref(x, p["w3"], p["b3"], dil)
        worst = {"h": _ratio(h, R.reshape(P, H), tol.reshape(P, H))}
        sref, stol = kr.conv3_stats_ref(h, L)
        sh = sh.reshape(nb, 2)
        worst["st_h"] = _ratio(sh, sref, stol)
        hv, dh = kr.gn_gelu_ref(h, L, sh, p["g1w"], p["g1b"], fast=bool(fast), out_bf16=False)
        yref, ytol = kr.moment_stats_ref(hv, L, p["w1"], p["b1"], d=dh)
        sy = sy.reshape(nb, 2)
        worst["st_y"] = _ratio(sy, yref, ytol)
        Rx, tv, ts = kr.dconv_apply_ref(hv, dh, p["w1"], p["b1"], sy, L, p["g2w"], p["g2b"], p["scale"],
                                        x.reshape(P, C), bool(fast), bool(xb))
        worst["x"] = _ratio(_vals(xg, bool(xb)).reshape(P, C), Rx, ts)
        _rec(kt, "small[C=%d,bf16=%d,fast=%d,dil=%d,nb=%d,L=%d]" % (C, xb, fast, dil, nb, L), worst)


@pytest.mark.parametrize("what", ["dil3", "C192", "gram"])
def test_dconv_small_refuses(kt, what):
    """-2 and nothing written: dil outside {1, 2}, C outside {48, 96}, no moments"""
    C, dil, gram = 48, 1, True
    if what == "dil3":
        dil = 3
    elif what == "C192":
        C = 192
    else:
        gram = False
    p = _small_weights(C, 1)
    x = np.ones((2, 16, C))
    rc, (xg, hg, sh, sy), x0, h0 = _small_run(kt, C, 1, 1, dil, x, 16, p, gram=gram)
    assert rc == -2
    assert (xg == x0).all() and (hg == h0).all() and (sh == 0).all() and (sy == 0).all()
    kt.record("small_refuses[%s]" % what, report=kt.DCONV_REPORT, refused=True)


# ===================================================================================================== fenc_row
FENC_T = [1, 2, 3, 15, 16, 17, 47, 49, 259, 271, 272]
FENC_BF = [(1, 1), (1, 3), (2, 4), (3, 3), (1, 17)]
FENC_DIMS = {0: (4, 48), 1: (48, 96)}
# every T at one (B, Fout), every (B, Fout) at T in {17, 259}, row_add / out4 off once each (level 0; on elsewhere)
FENC_CASES = ([(T, 2, 4, 1, 1) for T in FENC_T] + [(T, B, Fo, 1, 1) for T in (17, 259) for (B, Fo) in FENC_BF
                                                    if (B, Fo) != (2, 4)] + [(17, 1, 3, 0, 1), (17, 1, 3, 1, 0)])


def _fenc_weights(level, seed=0):
    """natural-order weights of one level (bf16-valued where the kernel reads bf16)"""
    cin, C = FENC_DIMS[level]
    H = C // 8
    rng = np.random.default_rng(1000 + level + seed)
    p = dict(wc=kr.bf16_round(rng.standard_normal((C, cin, 8)) / np.sqrt(8.0 * cin)), bc=_f32(0.3 * rng.standard_normal(C)),
             wr=kr.bf16_round(rng.standard_normal((2 * C, C)) / np.sqrt(C)), br=_f32(0.3 * rng.standard_normal(2 * C)), dc=[])
    for dd in range(2):
        w1, b1 = _mom_weights(H, rng)
        p["dc"].append(dict(w3=kr.bf16_round(rng.standard_normal((H, C, 3)) / np.sqrt(3.0 * C)),
                            b3=_f32(0.5 * rng.standard_normal(H)), g1w=_f32(1 + 0.25 * rng.standard_normal(H)),
                            g1b=_f32(0.1 * rng.standard_normal(H)), w1=kr.bf16_round(w1), b1=b1,
                            g2w=_f32(1 + 0.25 * rng.standard_normal(2 * C)), g2b=_f32(0.1 * rng.standard_normal(2 * C)),
                            scale=_f32(rng.uniform(0.5, 1.5, C))))
    return p


def _fenc_inputs(level, B, Fout, T, seed):
    """x [B][Fin][T][Cin] (level 0: raw f32 values with a non-zero mean; level 1: bf16 values), a_norm [B][2], row_add
    [Fout][C]; the four input rows under output row (b, f) carry that row's power of two"""
    cin, C = FENC_DIMS[level]
    rng = np.random.default_rng(seed)
    Fin = 4 * Fout
    rs = _rowscale(B * Fout).reshape(B, Fout)
    x = rng.standard_normal((B, Fin, T, cin)) * np.repeat(rs, 4, axis=1)[:, :, None, None]
    if level == 0:
        x = _f32(x + 0.7)
        a_norm = _f32(np.stack([0.7 + 0.1 * np.arange(B), 1.5 + 0.25 * np.arange(B)], -1))
    else:
        x = kr.bf16_round(x + 0.25)
        a_norm = None
    return x, a_norm, _f32(0.5 * rng.standard_normal((Fout, C)))


def _fenc_ref(level, p, x, a_norm, row_add, mut=None):
    """(R, tol) [B][Fout][T][C]"""
    B, Fin, T, _ = x.shape
    Fout = Fin // 4
    C = FENC_DIMS[level][1]
    R, tol = np.empty((B, Fout, T, C)), np.empty((B, Fout, T, C))
    for b in range(B):
        for f in range(Fout):
            R[b, f], tol[b, f] = kr.fenc_row_ref(level, p, x[b], None if a_norm is None else a_norm[b], f, Fin,
                                                 row_add=row_add, mut=mut)
    return R, tol


def _fenc_run(kt, level, p, x, a_norm, row_add, out4):
    """-> (rc, out bits [R + 1][T][C], out4 bits [R + 1][T][4] or None): one sentinel row behind the R rows"""
    cin, C = FENC_DIMS[level]
    H = C // 8
    B, Fin, T, _ = x.shape
    Fout = Fin // 4
    R = B * Fout
    G = 8192                                                    # guard bands: more than one LDS-DMA piece
    keep = []

    def f(a):
        keep.append(kt.Buf(a, "f32", G))
        return keep[-1].ptr

    def h(a, ld):
        w = np.zeros((a.shape[0], ld))
        w[:, :a.shape[1]] = a
        keep.append(kt.Buf(kr.bf16_bits(w.astype(np.float32)), "bf16", G))
        return keep[-1].ptr

    if level == 0:
        keep.append(kt.Buf(np.transpose(x, (0, 2, 1, 3)), "f32", G))          # [B][T][Fin][4]
    else:
        keep.append(kt.Buf(kr.bf16_bits(x.astype(np.float32)), "bf16", G))    # [B][Fin][T][48]
    d = dict(in_=keep[-1].ptr, B=B, Fin=Fin, Fout=Fout, T=T, cin=cin, c=C)
    if level == 0:
        d["a_norm"] = f(a_norm)
    wc = np.transpose(p["wc"], (0, 2, 1)).reshape(C, 8 * cin)
    d.update(wc=h(wc, _roundup(8 * cin, 64)), wc_ld=_roundup(8 * cin, 64), bc=f(p["bc"]), w3_ld=_roundup(3 * C, 64),
             w1_ld=64, wr=h(kr.glu_order(p["wr"]), _roundup(C, 64)), wr_ld=_roundup(C, 64), br=f(kr.glu_order(p["br"])))
    for dd in range(2):
        q = p["dc"][dd]
        s = str(dd)
        d.update({"w3" + s: h(kr.conv3_pack(q["w3"], 16), _roundup(3 * C, 64)), "b3" + s: f(q["b3"]),
                  "g1w" + s: f(q["g1w"]), "g1b" + s: f(q["g1b"]), "w1" + s: h(kr.conv1x1_pack(q["w1"]), 64),
                  "b1" + s: f(kr.glu_order(q["b1"])), "g2w" + s: f(kr.glu_order(q["g2w"])),
                  "g2b" + s: f(kr.glu_order(q["g2b"])), "gram" + s: f(kt.conv1x1_moments(q["w1"], q["b1"], True)),
                  "scale" + s: f(q["scale"])})
    if row_add is not None:
        d["row_add"] = f(row_add)
    bo, _ = _out16(kt, (R + 1) * T * C, G)
    d["out"] = bo.ptr
    b4 = None
    if out4:
        b4, _ = _out16(kt, (R + 1) * T * 4, G)
        d["out4"] = b4.ptr
    rc = kt.lib.kt_fenc_row(ctypes.byref(kt.fill(kt.KtFencRow, **d)), None)
    kt.sync()
    out, ok = bo.host()
    assert ok, "guard band of out overwritten"
    o4 = None
    if b4 is not None:
        o4, ok = b4.host()
        assert ok, "guard band of out4 overwritten"
        o4 = o4.reshape(R + 1, T, 4)
    return rc, out.reshape(R + 1, T, C), o4


@pytest.mark.parametrize("T,B,Fout,radd,o4", FENC_CASES)
@pytest.mark.parametrize("level", [0, 1])
def test_fenc_row(kt, level, T, B, Fout, radd, o4):
    """A whole frequency-encoder level per (b, f) row against the whole-level tanh-form reference with the end-to-end
    bound (kernel_refs.fenc_row_ref).  R = B Fout below, at and above a multiple of 8 (the grid is rounded up to 8 and
    rows are dealt out as (block & 7) per + (block >> 3)); the first and last frequency rows have taps outside
    [0, Fin); T from one position to FR_MT_MAX tiles.  The bound is worst case through five bf16 roundings: at level 0
    it separates wrong taps, rows, embeddings and channels but not a statistics count off by 5 %; at level 1 it is
    vacuous (about 1e3) and the comparison only shows finite values of the right order (figures:
    tests/test_dconv_refs.py FENC_SEPARATED).  test_fenc_row_structure holds what can be asserted exactly."""
    cin, C = FENC_DIMS[level]
    p = _fenc_weights(level)
    x, a_norm, row_add = _fenc_inputs(level, B, Fout, T, 31 * T + 7 * B + Fout + level)
    if level == 1 or not radd:
        row_add = None
    o4 = bool(o4) and level == 0
    rc, out, out4 = _fenc_run(kt, level, p, x, a_norm, row_add, o4)
    assert rc == 0, rc
    R = B * Fout
    assert (out[R:] == SENT16).all(), "rows >= R of out were written"
    Rr, tol = _fenc_ref(level, p, x, a_norm, row_add)
    worst = {"out": _ratio(_vals(out[:R], True).reshape(B, Fout, T, C), Rr, tol)}
    if o4:
        assert (out4[R:] == SENT16).all() and np.array_equal(out4[:R], out[:R, :, :4]), "out4 != channels 0..3 of out"
    _rec(kt, "fenc_row[level=%d,T=%d,B=%d,Fout=%d,row_add=%d,out4=%d]" % (level, T, B, Fout, radd, o4), worst)


@pytest.mark.parametrize("T,B,Fout,radd,o4", FENC_CASES)
@pytest.mark.parametrize("level", [0, 1])
def test_fenc_row_structure(kt, level, T, B, Fout, radd, o4):
    """What of a fused level can be asserted exactly, with no error bound: every element of the R = B Fout rows of T
    positions is written with a finite value and nothing else is (the row behind the last one and the guard bands
    keep their sentinels), out4 (level 0) equals channels 0..3 of out bit for bit, and a row does not depend on where
    the grid puts it: row (b, f) of a batch of B items equals the same row computed with that item alone (B = 1), bit
    for bit, as does the whole output of a second launch.  R sits below, at and above a multiple of 8 (the grid is
    rounded up to 8 and rows are dealt out as (block & 7) per + (block >> 3)); T runs from one position to FR_MT_MAX
    tiles.  (test_fenc_row compares the values with the reference.)"""
    cin, C = FENC_DIMS[level]
    p = _fenc_weights(level)
    x, a_norm, row_add = _fenc_inputs(level, B, Fout, T, 31 * T + 7 * B + Fout + level)
    if level == 1 or not radd:
        row_add = None
    o4 = bool(o4) and level == 0
    rc, out, out4 = _fenc_run(kt, level, p, x, a_norm, row_add, o4)
    assert rc == 0, rc
    R = B * Fout
    assert (out[R:] == SENT16).all(), "rows >= R of out were written"
    vals = _vals(out[:R], True)
    assert np.isfinite(vals).all()
    # (a computed value equal to the sentinel's bit pattern, -9.6e30, cannot come out of these inputs)
    assert (out[:R] != SENT16).all(), "%d elements of the R rows were not written" % int((out[:R] == SENT16).sum())
    if o4:
        assert (out4[R:] == SENT16).all() and np.array_equal(out4[:R], out[:R, :, :4]), "out4 != channels 0..3 of out"
    rc2, again, _ = _fenc_run(kt, level, p, x, a_norm, row_add, False)
    assert rc2 == 0 and np.array_equal(again, out), "a second launch differs"
    if B > 1:
        b = B - 1
        rc1, one, _ = _fenc_run(kt, level, p, x[b:b + 1], None if a_norm is None else a_norm[b:b + 1], row_add, False)
        assert rc1 == 0 and np.array_equal(one[:Fout], out[b * Fout:(b + 1) * Fout]), "a row depends on its grid slot"
    kt.record("fenc_row_structure[level=%d,T=%d,B=%d,Fout=%d,row_add=%d,out4=%d]" % (level, T, B, Fout, radd, o4),
              report=kt.DCONV_REPORT, exact=True, rms=float(np.sqrt((vals * vals).mean())))


@pytest.mark.parametrize("what", ["T273", "Fin", "gram", "c96"])
def test_fenc_row_refuses(kt, what):
    """fenc_row_launch's refusals: -1 and nothing written for T = 273 (more than FR_MT_MAX tiles), Fin != 4 Fout, a
    null moments pointer, (cin, c) = (4, 96)"""
    B, Fout, T, cin, c = 1, 2, 17, 4, 48
    Fin, gram1 = 4 * Fout, True
    if what == "T273":
        T = 273
    elif what == "Fin":
        Fin = 4 * Fout + 1
    elif what == "gram":
        gram1 = False
    else:
        c = 96
    assert kt.lib.kt_fenc_row_supported(cin, c, T) == (1 if what in ("Fin", "gram") else 0)
    dummy = kt.Buf(np.zeros(1 << 16), "f32", 1024)
    bo, o0 = _out16(kt, B * Fout * T * 96, 4096)
    b4, c0 = _out16(kt, B * Fout * T * 4, 4096)
    names = [f for f, _ in kt.KtFencRow._fields_]
    d = {f: dummy.ptr for f in names if f not in "B Fin Fout T wc_ld w3_ld w1_ld wr_ld cin c".split()}
    d.update(B=B, Fin=Fin, Fout=Fout, T=T, wc_ld=64, w3_ld=192, w1_ld=64, wr_ld=64, cin=cin, c=c, out=bo.ptr,
             out4=b4.ptr)
    if not gram1:
        d["gram1"] = None
    assert kt.lib.kt_fenc_row(ctypes.byref(kt.fill(kt.KtFencRow, **d)), None) == -1
    kt.sync()
    out, ok1 = bo.host()
    out4, ok2 = b4.host()
    assert ok1 and ok2 and (out == o0).all() and (out4 == c0).all()
    kt.record("fenc_row_refuses[%s]" % what, report=kt.DCONV_REPORT, refused=True)
