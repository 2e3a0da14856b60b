"""CPU checks of the decoder references of tests/kernel_refs.py (lin_index_ref, resize_h_ref, dec_merge_ref, dec_last_ref,
fdec_lr_ref) and of the host code behind tests/test_gpu_dec.py: the struct sizes of libathd_ktest.so, the last level's
fold (pack.h dec_last_fold) and the host-only shape predicates.  No GPU.

* Every reference equals the same chain of torch.nn.functional (conv_transpose2d / 1d, interpolate, group_norm, gelu) in
  float64: the resize to 1e-6 relative (float32 lambda against float64 lambda), the rest to 1e-12.
* The bounds are not vacuous.  For every case family an honest float32 emulation in the documented operation order
  (tests/dec_cases.py; bf16 at the documented rounding points, the tanh GELU where fast_gelu) stays inside tol
  everywhere, and every deliberate mutation lands more than 10x outside tol on at least one element.  SEPARATION records
  the smallest mutation-to-tol ratio per family measured at these shapes (the assertion is the 10x bar, not the figure):
  dec_merge 2.3e4, fdec_last 374, tdec_last 374, fdec_tail 24.8 (the w tile duplicated from W - 1), tdec_tail 252,
  fdec_lr rows 1.1e6, statistics 487, merge 24.6 (GroupNorm count one row short), fdec1_gram 11.6 (the statistics one
  row short, beside the bf16 rounding-tie term of Z).
* Mutations that are identities are left out where they are, with the reason: taps 3 and 4 under an exact /4 resize
  (rows 4d + 1 and 4d + 2 are added with equal weights: A0 = P (W3 + W4) / 2), Am / Ap at a single row, i1 for i0 where
  lambda is 0.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import dec_cases as dc
import kernel_refs as kr


@pytest.fixture(scope="module")
def ktl():
    import ktest
    return ktest


# smallest max|mutated - R| / tol per family at the shapes of this file (measured; every one is asserted > 10)
SEPARATION = {}


def _inside(got, R, tol):
    return float((np.abs(got - R) / np.maximum(tol, 1e-300)).max())


def _outside(Rm, R, tol, family, name):
    ok = np.isfinite(Rm) & np.isfinite(R)
    r = float((np.abs(Rm - R)[ok] / np.maximum(tol[ok], 1e-300)).max())
    SEPARATION[family] = min(SEPARATION.get(family, np.inf), r)
    assert r > 10.0, (family, name, r)
    return r


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ============================================================================================ structs, fold, predicates
def test_struct_sizes(ktl):
    for name, (a, b) in ktl.sizes_match().items():
        assert a == b, (name, a, b)
    assert ktl.lib.kt_sizeof_lrstep() == ktl.LRSTEP.itemsize == 32
    assert {"merge", "lowrank", "declast"} <= set(ktl.sizes_match())


def test_constants_exported(ktl):
    """the tile constants the GPU shape lists are built from"""
    vals = {n: getattr(ktl.lib, "kt_" + n)() for n in ("fl_dc", "ft_dc", "tl_in", "tt_rows", "dm_run", "merge_maxp", "g_wb")}
    assert all(v > 0 for v in vals.values()), vals
    assert vals["tt_rows"] >= vals["tl_in"] + 2
    assert ktl.lib.kt_fdec1_gram_q_doubles() > 0


@pytest.mark.parametrize("br", [0, 1])
def test_dec_last_fold(ktl, br):
    """the product's fold equals the float64 fold of dec_last.hip's header to 1 float32 ulp, in the documented layout:
    freq [Am | A0 | Ap] (3 x [2][48]), P b + pb, 0.1 P; time Q_k (8 x [2][48]), P b, pb, 0.1 P"""
    w, b, P, pb = dc.last_weights(11 + br)
    got = ktl.dec_last_fold(w, b, P, pb, br).astype(np.float64)
    ref = kr.dec_last_fold_ref(w, b, P, pb, br)
    assert got.shape == ref.shape == ((298,) if br == 0 else (780,))
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    assert (np.abs(got - ref) <= ulp).all()
    # layout, from the formulas and single entries
    Q = lambda k, j, ci: float(P[j] @ w[ci, :, k])
    if br == 0:
        assert abs(got[0 * 96 + 1 * 48 + 5] - 0.5 * Q(7, 1, 5)) < 1e-6            # Am[1][5]
        assert abs(got[1 * 96 + 0 * 48 + 47] - 0.5 * (Q(3, 0, 47) + Q(4, 0, 47))) < 1e-6
        assert abs(got[2 * 96 + 1 * 48 + 0] - 0.5 * Q(0, 1, 0)) < 1e-6
        assert np.allclose(got[288:290], P @ b + pb, atol=1e-6) and np.allclose(got[290:], (0.1 * P).ravel(), atol=1e-7)
    else:
        assert abs(got[(3 * 2 + 1) * 48 + 7] - Q(3, 1, 7)) < 1e-6                 # Q_3[1][7]
        assert np.allclose(got[768:770], P @ b, atol=1e-6) and (got[770:772] == pb).all()
        assert np.allclose(got[772:], (0.1 * P).ravel(), atol=1e-7)


def _bf16_bits(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().view(torch.int16).numpy().view(np.uint16)


# (cin, cout, H): a first row with no u - 1, a last row with no u + 1, an interior row, the product's channel counts
@pytest.mark.parametrize("cin,cout,H", [(1, 1, 1), (3, 2, 2), (3, 2, 5), (96, 48, 3)])
def test_convt_rows(ktl, cin, cout, H):
    """the packed ConvTranspose (k8, s4, p2) residue rows of pack.h, applied to their window of input rows (rows outside
    [0, H) are zero), reproduce torch's conv_transpose1d in float64 at output rows 4u + rho to 1e-12 relative (only the
    summation order differs): the two pairs (residues {2pi, 2pi+1} over rows u + RES_OFF[2pi], +1), the quad (all four
    over u-1, u, u+1) and the convt4 form (residue rho over its own rows u + RES_OFF[rho], +1; its rows are bf16, so the
    convolution it reproduces is the one with the bf16-rounded weights, and its bias is the layer's own).  Every packed
    entry is bit-equal to a source weight (convt4: to its bf16 rounding) or exactly +0, and the convt4 rows are bit-equal
    to the product's host_f2bf of the quad's columns of those rows."""
    rng = np.random.default_rng(1000 * cin + 10 * cout + H)
    w = rng.standard_normal((cin, cout, 8)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    x = rng.standard_normal((H, cin))
    wb = torch.from_numpy(w).bfloat16().double().numpy()          # the weights the convt4 rows hold

    def conv(wt):       # [4 H][cout]
        y = Fn.conv_transpose1d(torch.from_numpy(x.T[None]), torch.from_numpy(wt).double(), torch.from_numpy(b).double(),
                                stride=4, padding=2)
        assert y.shape == (1, cout, 4 * H)
        return y[0].T.numpy()

    ref, ref_b = conv(w), conv(wb)
    xp = np.zeros((H + 2, cin))
    xp[1:H + 1] = x                                               # input row r at xp[r + 1]

    def apply(rows, bias, row_lo, nrows):     # [H][rows]: the rows times the window u + row_lo .. + nrows - 1
        win = np.concatenate([xp[1 + row_lo + j:1 + row_lo + j + H] for j in range(nrows)], axis=1)
        return win @ rows.astype(np.float64).T + bias.astype(np.float64)

    wbits = np.append(w.view(np.uint32).ravel(), np.uint32(0))
    for pi in range(2):
        rows, bias = ktl.convt_rows(w, b, ktl.CONVT_PAIR, pi)
        assert np.isin(rows.view(np.uint32), wbits).all() and (bias == np.tile(b, 2)).all()
        got = apply(rows, bias, kr.RES_OFF[2 * pi], 2)
        for h in range(2):
            assert _rel(got[:, h * cout:(h + 1) * cout], ref[2 * pi + h::4]) <= 1e-12, (pi, h)
    quad, qbias = ktl.convt_rows(w, b, ktl.CONVT_QUAD)
    assert np.isin(quad.view(np.uint32), wbits).all() and (qbias == np.tile(b, 4)).all()
    got = apply(quad, qbias, -1, 3)
    for rho in range(4):
        assert _rel(got[:, rho * cout:(rho + 1) * cout], ref[rho::4]) <= 1e-12, rho
    ct4, none = ktl.convt_rows(w, b, ktl.CONVT4)
    assert none is None and np.isin(ct4, np.append(_bf16_bits(w).ravel(), np.uint16(0))).all()
    ct4f = (ct4.astype(np.uint32) << 16).view(np.float32)
    for rho in range(4):
        sl = slice(rho * cout, (rho + 1) * cout)
        qwin = quad[sl, (kr.RES_OFF[rho] + 1) * cin:(kr.RES_OFF[rho] + 3) * cin]
        f2bf = np.array([ktl.lib.kt_host_f2bf(int(v)) for v in qwin.view(np.uint32).ravel()], dtype=np.uint16)
        assert (ct4[sl].ravel() == f2bf).all(), rho
        assert _rel(apply(ct4f[sl], b, kr.RES_OFF[rho], 2), ref_b[rho::4]) <= 1e-12, rho


def _dl(ktl, **kw):
    one = ctypes.c_double(0.0)
    base = dict(in_=ctypes.addressof(one), g=ctypes.addressof(one), stats=ctypes.addressof(one), NI=4, P=4, W=1,
                H_skip=8, C_skip=4, H_skip2=8, C_skip2=48)
    base.update(kw)
    d = ktl.fill(ktl.KtDecLast, **base)
    d._keep = one
    return d


def test_tdec_tail_supported(ktl):
    """4 H == T and every block's span of g rows fits the LDS tile (kernels.h): Hg in H .. H + 3 and the model's 4 H
    pass; 4 H != T, a span over TT_ROWS (Hg = 2 H at H = 300), null g and C_skip2 < 48 are refused"""
    sup = lambda **kw: ktl.lib.kt_tdec_tail_supported(ctypes.byref(_dl(ktl, **kw)))
    tl_in, tt_rows = ktl.lib.kt_tl_in(), ktl.lib.kt_tt_rows()
    for H in (1, 2, 64, tl_in - 1, tl_in, tl_in + 1, 2 * tl_in + 1):
        for Hg in range(H, H + 4):
            assert sup(H=H, T=4 * H, Hg=Hg) == 1, (H, Hg)
    assert sup(H=64, T=4 * 64, Hg=4 * 64) == 1 and sup(H=1, T=4, Hg=4) == 1
    assert sup(H=64, T=4 * 64 + 1, Hg=64) == 0 and sup(H=64, T=4 * 64 - 3, Hg=64) == 0
    assert 2 * (tl_in + 2) > tt_rows
    assert sup(H=300, T=1200, Hg=600) == 0
    assert sup(H=64, T=256, Hg=64, g=None) == 0 and sup(H=64, T=256, Hg=64, stats=None) == 0
    assert sup(H=64, T=256, Hg=64, C_skip2=40) == 0 and sup(H=64, T=256, Hg=0) == 0


def test_fdec1_gram_supported(ktl):
    """the Gram statistics pass covers bf16 Z, Co = 96, Ci = 192, Hs = 32, Hk = 8, Hd > 32, W >= G_WB (kernels.h)"""
    one = ctypes.c_double(0.0)
    p = ctypes.addressof(one)
    wb = ktl.lib.kt_g_wb()
    base = dict(S=p, Wt=p, Zs=p, bias=p, stats=p, w_ld=192, Ci=192, Co=96, Hs=32, Hk=8, z_bf16=1, Hd=33, W=wb, P=1, NI=1)
    sup = lambda **kw: ktl.lib.kt_fdec1_gram_supported(ctypes.byref(ktl.fill(ktl.KtLowRank, **{**base, **kw})))
    assert sup() == 1 and sup(W=48, NI=8, P=4, Hd=259, w_ld=200) == 1
    assert sup(W=wb - 1) == 0 and sup(W=7 if wb > 7 else wb - 1) == 0
    assert sup(Hd=32) == 0 and sup(Ci=96) == 0 and sup(z_bf16=0) == 0
    assert sup(Co=48) == 0 and sup(w_ld=196) == 0 and sup(NI=6, P=4) == 0 and sup(S=None) == 0


# ===================================================================================================== resize
@pytest.mark.parametrize("hin,hout", [(8, 33), (32, 259), (512, 259), (7, 7), (5, 1)])
def test_resize_equals_interpolate(hin, hout):
    rng = np.random.default_rng(hin * 1000 + hout)
    x = rng.standard_normal((2, hin, 3, 4))
    R, T = kr.resize_h_ref(x, hout, axis=1)
    t = torch.from_numpy(np.transpose(x, (0, 3, 1, 2)).copy())
    ref = np.transpose(Fn.interpolate(t, size=(hout, 3), mode="bilinear", align_corners=False).numpy(), (0, 2, 3, 1))
    # 1e-6 relative to the source coordinate: lambda is the fraction of src = scale (dst + 0.5) - 0.5 < hin, evaluated in
    # float32 (e = 6e-8 of src; measured 4.2e-8 .. 4.6e-8 of hin at these sizes).  An absolute 1e-6 on lambda cannot hold
    # for a bit-exact float32 rule: at 512 -> 259 one float32 rounding of src is already 3e-5.
    eye = torch.eye(hin, dtype=torch.float64).reshape(1, 1, hin, hin)
    m = Fn.interpolate(eye, size=(hout, hin), mode="bilinear", align_corners=False)[0, 0].numpy()
    M, _ = kr.resize_h_ref(np.eye(hin), hout, axis=0)
    assert np.abs(M - m).max() <= 1e-6 * hin
    assert np.abs(R - ref).max() <= 1e-6 * hin * 2 * np.abs(x).max()
    i0, i1, l0, l1 = kr.lin_index_ref(hin, hout)
    assert i0.min() >= 0 and i1.max() <= hin - 1 and ((i1 == i0) | (i1 == i0 + 1)).all()
    assert l0.dtype == l1.dtype == np.float32 and ((l0 + l1) == 1).all()
    # the two evaluation orders of the source index agree within lin_slack
    _, _, _, l1b = kr.lin_index_ref(hin, hout, fma=False)
    assert (kr.lin_index_ref(hin, hout, fma=False)[0] == i0).all()
    assert np.abs(l1b.astype(np.float64) - l1).max() <= kr.lin_slack(hin, hout)


# ===================================================================================================== dec_merge
def _torch_merge(c, kept=False):
    src = torch.from_numpy(np.transpose(c["src"], (0, 3, 1, 2)).copy())
    a = src
    if c["stats"] is not None:
        a = Fn.gelu(Fn.group_norm(src, 1, torch.from_numpy(c["gn_w"]), torch.from_numpy(c["gn_b"]), eps=1e-5))
    a = Fn.interpolate(a, size=(c["H_out"], c["W"]), mode="bilinear", align_corners=False)
    sk = torch.from_numpy(np.transpose(c["skip"][..., :c["C"]], (0, 3, 1, 2)).copy())
    sk = Fn.interpolate(sk, size=(c["H_out"], c["W"]), mode="bilinear", align_corners=False)
    v = a + 0.1 * sk.repeat_interleave(c["P"], dim=0)
    if c["proj_w"] is not None:
        v = Fn.conv2d(v, torch.from_numpy(c["proj_w"])[:, :, None, None], torch.from_numpy(c["proj_b"]))
        return np.transpose(v.numpy(), (0, 3, 2, 1))          # [NI][W][H][2]
    return np.transpose(v.numpy(), (0, 2, 3, 1))


MERGE_CPU = [  # NI, P, C, H_src, H_out, H_skip, W, C_skip, kept, proj
    (6, 3, 48, 12, 7, 9, 5, 56, False, False),
    (8, 4, 48, 40, 33, 16, 1, 48, False, False),
    (4, 2, 96, 28, 7, 7, 3, 96, True, False),
    (4, 2, 4, 20, 5, 11, 6, 8, True, True),
    (2, 1, 4, 9, 9, 4, 5, 4, False, False),
]


# power-of-two ratios and identities: lambda is exact in float32, so the float64 chain is met to 1e-12 (the ragged
# resize itself is test_resize_equals_interpolate)
MERGE_EXACT = [(6, 3, 48, 28, 7, 7, 5, 56, True, False), (8, 4, 48, 16, 32, 8, 1, 48, False, False),
               (4, 2, 4, 20, 5, 10, 6, 8, True, True), (2, 1, 4, 9, 9, 36, 5, 4, False, False),
               (2, 2, 96, 8, 4, 4, 2, 96, False, False)]


@pytest.mark.parametrize("gn", [True, False])
@pytest.mark.parametrize("shape", MERGE_EXACT)
def test_dec_merge_ref_equals_torch(shape, gn):
    NI, P, C, H_src, H_out, H_skip, W, C_skip, kept, proj = shape
    c = dc.merge_case(3, NI, P, C, H_src, H_out, H_skip, W, C_skip, gn=gn, proj=proj)
    R, tol = dc.merge_ref(c, kept=kept)
    assert np.isfinite(R).all() and _rel(R, _torch_merge(c)) < 1e-12


MERGE_MUTS = ["i1_as_i0", "skip_next_seg", "skip_prompt", "no_gain", "gn_next_item"]


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("shape", MERGE_CPU)
def test_dec_merge_bounds(shape, bf16):
    NI, P, C, H_src, H_out, H_skip, W, C_skip, kept, proj = shape
    c = dc.merge_case(5, NI, P, C, H_src, H_out, H_skip, W, C_skip, bf16=bf16, proj=proj)
    for folded in ([False, True] if bf16 else [False]):
        kw = dict(kept=kept, fast=bf16, folded=folded, out_bf16=bf16 and not proj)
        R, tol = dc.merge_ref(c, **kw)
        assert _inside(dc.merge_emulate(c, **kw), R, tol) <= 1.0
    for mut in MERGE_MUTS:
        if mut == "i1_as_i0" and H_src == H_out:
            continue
        _outside(dc.merge_ref(c, mut=mut, **kw)[0], R, tol, "dec_merge", mut)


# ===================================================================================================== dec_last
def _torch_last(c, x=None):
    w, b, Pm, pb = (torch.from_numpy(v) for v in c["wts"])
    x = c["x"] if x is None else x
    P = c["P"]
    if c["br"] == 0:
        t = torch.from_numpy(np.transpose(x, (0, 3, 1, 2)).copy())
        y = Fn.conv_transpose2d(t, w[:, :, :, None], b, stride=(4, 1), padding=(2, 0))
        y = Fn.interpolate(y, size=(c["H"], c["W"]), mode="bilinear", align_corners=False)
        sk = torch.from_numpy(np.transpose(c["skip"][..., :4], (0, 3, 1, 2)).copy())
        sk = Fn.interpolate(sk, size=(c["H"], c["W"]), mode="bilinear", align_corners=False)
        o = Fn.conv2d(y + 0.1 * sk.repeat_interleave(P, dim=0), Pm[:, :, None, None], pb)
        return np.transpose(o.numpy(), (0, 3, 2, 1))
    t = torch.from_numpy(np.transpose(x, (0, 2, 1)).copy())
    y = Fn.conv_transpose1d(t, w, b, stride=4, padding=2)
    y = Fn.interpolate(y, size=c["T"], mode="linear", align_corners=False)
    sk = torch.from_numpy(np.transpose(c["skip"][..., :4], (0, 2, 1)).copy())
    sk = Fn.interpolate(sk, size=c["T"], mode="linear", align_corners=False)
    o = Fn.conv1d(y + 0.1 * sk.repeat_interleave(P, dim=0), Pm[:, :, None], pb)
    return np.transpose(o.numpy(), (0, 2, 1))


LAST_CPU = [  # br, NI, P, H, W, H_skip, C_skip, T
    (0, 6, 3, 17, 5, 17, 4, None), (0, 4, 2, 33, 3, 70, 8, None), (0, 2, 1, 1, 2, 4, 4, None),
    (1, 6, 3, 9, 1, 36, 4, 36), (1, 4, 2, 30, 1, 50, 8, 117), (1, 2, 1, 1, 1, 3, 4, 1), (1, 4, 2, 7, 1, 20, 4, 33),
]


LAST_EXACT = [(0, 6, 3, 17, 5, 17, 4, None), (0, 4, 2, 8, 3, 32, 8, None), (0, 2, 1, 1, 2, 4, 4, None),
              (1, 6, 3, 9, 1, 36, 4, 36), (1, 4, 2, 8, 1, 64, 8, 16), (1, 2, 1, 1, 1, 1, 4, 1), (1, 4, 2, 4, 1, 8, 4, 32)]


@pytest.mark.parametrize("shape", LAST_EXACT)
def test_dec_last_ref_equals_torch(shape):
    br, NI, P, H, W, H_skip, C_skip, T = shape
    c = dc.last_case(21, br, NI, P, H, W, H_skip, C_skip, T=T)
    assert _rel(dc.last_ref(c)[0], _torch_last(c)) < 1e-12


LAST_MUTS = ["taps34", "am_ap", "no_bias", "no_gain", "skip_next_seg", "skip_prompt", "i1_as_i0"]


def _halo_mutants(c, edge, R, last_ref):
    """rows next to a chunk / block edge computed with the row across the edge replaced by zero, and by the row on the
    near side (its neighbour): `edge` is the first input row of the second chunk"""
    x = c["x"]
    out = []
    for how in ("zero", "neighbour"):
        for side in (0, 1):                     # 0: the chunk above reads row `edge` wrong; 1: the chunk below reads edge - 1
            xa = x.copy()
            row, near = (edge, edge - 1) if side == 0 else (edge - 1, edge)
            xa[:, row] = 0.0 if how == "zero" else x[:, near]
            Ra = last_ref(xa)
            Rm = R.copy()
            if c["br"] == 0:                    # out [NI][W][H][2]: output row d reads x[d - 1 .. d + 1]
                d = edge - 1 if side == 0 else edge
                Rm[:, :, d] = Ra[:, :, d]
            else:                               # out [NI][T][2], T = 4 H: rows 4u .. 4u + 3 of input row u
                u = edge - 1 if side == 0 else edge
                Rm[:, 4 * u:4 * u + 4] = Ra[:, 4 * u:4 * u + 4]
            out.append((how + str(side), Rm))
    return out


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("shape", LAST_CPU)
def test_dec_last_bounds(ktl, shape, bf16):
    br, NI, P, H, W, H_skip, C_skip, T = shape
    c = dc.last_case(23, br, NI, P, H, W, H_skip, C_skip, bf16=bf16, T=T)
    fold = ktl.dec_last_fold(*c["wts"], br)
    R, tol = dc.last_ref(c)
    assert _inside(dc.last_emulate(c, fold), R, tol) <= 1.0
    fam = "fdec_last" if br == 0 else "tdec_last"
    for mut in LAST_MUTS:
        if mut == "i1_as_i0" and (H_skip == (H if br == 0 else T) or T == 1):
            continue                            # (an identity; 3 -> 1 has src = 1.0: lambda is 0)
        if mut == "am_ap" and H == 1:
            continue                            # (a single row has neither neighbour: Am, Ap multiply zero rows)
        if mut == "taps34" and (br == 0 or T == H):
            continue                            # (an exact /4 resize adds rows 4d + 1, 4d + 2: A0 = P (W3 + W4) / 2)
        _outside(dc.last_ref(c, mut=mut)[0], R, tol, fam, mut)
    edge = {0: ktl.lib.kt_fl_dc(), 1: ktl.lib.kt_tl_in()}[br]
    if br == 0 and H > edge or br == 1 and H > 4 and T == 4 * H:
        e = edge if br == 0 else H // 2         # (time: any row is some shape's block edge; the block size is a GPU matter)
        for name, Rm in _halo_mutants(c, e, R, lambda xa: dc.last_ref(c, x=xa)[0]):
            _outside(Rm, R, tol, fam, "halo_" + name)


# ===================================================================================================== dec_tail
TAIL_CPU = [  # br, NI, P, H, W, H_skip, C_skip, H_skip2, C_skip2, Hg
    (0, 6, 3, 33, 5, 33, 4, 67, 48, None), (0, 4, 2, 17, 18, 68, 8, 17, 96, None),
    (1, 6, 3, 12, 1, 48, 4, 20, 48, 15), (1, 4, 2, 9, 1, 30, 8, 9, 96, 9),
]


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("shape", TAIL_CPU)
def test_dec_tail_bounds(ktl, shape, bf16):
    br, NI, P, H, W, H_skip, C_skip, H_skip2, C_skip2, Hg = shape
    c = dc.tail_case(31, br, NI, P, H, W, H_skip, C_skip, H_skip2, C_skip2, bf16=bf16, Hg=Hg)
    fold = ktl.dec_last_fold(*c["wts"], br)
    R, tol, x, tx = dc.tail_ref(c)
    assert _inside(dc.tail_emulate(c, fold), R, tol) <= 1.0
    fam = "fdec_tail" if br == 0 else "tdec_tail"
    for mut in ["skip_next_seg", "skip_prompt", "no_gain", "gn_next_item"] + (["i1_as_i0"] if H_skip2 != H else []):
        _outside(dc.tail_ref(c, mut=mut)[0], R, tol, fam, "merge_" + mut)
    for mut in ["am_ap", "no_bias", "no_gain", "skip_next_seg", "skip_prompt"] + (["taps34"] if br else []):
        _outside(dc.tail_ref(c, mut_last=mut)[0], R, tol, fam, "last_" + mut)
    # GroupNorm count off by one row
    m = dict(c["merge"])
    m["gn_count"] = c["merge"]["gn_count"] - W * 48
    c2 = dict(c, merge=m)
    _outside(dc.tail_ref(c2)[0], R, tol, fam, "count_row")
    if br == 0:
        e = ktl.lib.kt_ft_dc()
        if H > e:
            for name, Rm in _halo_mutants(dict(c, x=x), e, R, lambda xa: dc.last_ref(c, x=xa)[0]):
                _outside(Rm, R, tol, fam, "halo_" + name)
        if W % 16:                               # the last partial w tile's spare lanes are clamped to W - 1
            Rm = R.copy()
            Rm[:, W // 16 * 16:] = R[:, W - 1:W]
            _outside(Rm, R, tol, fam, "w_tile_dup")
    else:
        for name, Rm in _halo_mutants(dict(c, x=x), H // 2, R, lambda xa: dc.last_ref(c, x=xa)[0]):
            _outside(Rm, R, tol, fam, "halo_" + name)


# ===================================================================================================== fdec_lr
def _torch_lr(c):
    """ConvTranspose2d of D0 = resize(S) + 0.1 resize(skip3) with the tap weights themselves (float64)"""
    S = torch.from_numpy(np.transpose(c["S"], (0, 3, 1, 2)).copy())
    K3 = torch.from_numpy(np.transpose(c["K3"], (0, 3, 1, 2)).copy())
    size = (c["Hd"], c["W"])
    D0 = Fn.interpolate(S, size=size, mode="bilinear", align_corners=False) + \
        0.1 * Fn.interpolate(K3, size=size, mode="bilinear", align_corners=False).repeat_interleave(c["P"], dim=0)
    w = torch.from_numpy(np.transpose(c["Wt"], (2, 1, 0)).copy())[:, :, :, None]         # [Ci][Co][8][1]
    y = Fn.conv_transpose2d(D0, w, torch.from_numpy(c["bias"]), stride=(4, 1), padding=(2, 0))
    return np.transpose(y.numpy(), (0, 2, 3, 1))


LR_CPU = [  # NI, P, Hd, W, Co, H_skip, C_skip
    (4, 2, 33, 3, 8, 32, 8), (6, 3, 49, 2, 6, 49, 12), (2, 1, 8, 2, 4, 20, 4), (2, 2, 1, 2, 4, 3, 4), (2, 1, 2, 1, 4, 2, 6),
]


@pytest.mark.parametrize("shape", [(4, 2, 64, 3, 8, 32, 8), (6, 3, 8, 2, 6, 8, 12), (2, 1, 16, 2, 4, 64, 4)])
def test_fdec_lr_ref_equals_torch(shape):
    """Hd = 8, 16, 64: every lerp weight (32 -> Hd, 8 -> Hd, H_skip -> Hd) is exact in float32"""
    NI, P, Hd, W, Co, H_skip, C_skip = shape
    c = dc.lr_case(41, NI, P, Hd, W, Co, H_skip, C_skip, False)
    Zx = np.einsum("nhwi,kci->nhwkc", c["S"], c["Wt"])                 # unrounded products: the identity under test
    Zsx = np.einsum("nhwi,kci->nhwkc", c["K3"], c["Wt"])
    Y, _ = kr.fdec_lr_ref(Zx, Zsx, c["bias"], Hd, P)
    ref = _torch_lr(c)
    assert _rel(Y, ref) < 1e-12
    st = dc.true_stats(Y)
    D1, _ = dc.lr_merge_ref(dict(c, out_bf16=False), Y, np.zeros_like(Y), st, fast=False, v3=False)
    m = dict(src=ref, skip=c["skip"], H_out=Hd, W=W, C=Co, P=P, stats=st, gn_w=c["gn_w"], gn_b=c["gn_b"], proj_w=None,
             proj_b=None)
    assert _rel(D1, _torch_merge(m)) < 1e-12


def test_lr_steps_ref():
    """the step table's documented content at a downsampling and an upsampling shape"""
    for Hd, Hs, Hk, Hj in ((33, 32, 8, 128), (5, 32, 8, 5), (1, 32, 8, 32)):
        st = kr.lr_steps_ref(Hd, Hs, Hk, Hj)
        z0, z1, _, lz = kr.lin_index_ref(Hs, Hd)
        j0, j1, _, lj = kr.lin_index_ref(Hj, Hd)
        assert (st["z0"][:Hd] == z0).all() and (st["lz"][:Hd] == lz).all() and (st["j1"][1:] == j1).all()
        assert (st["lj"][1:] == lj).all() and st["flags"][0] & 3 == 3 and st["flags"][min(1, Hd)] & 4
        assert st["flags"][Hd] & 3 == 0 and len(st["flags"]) == Hd + 1


@pytest.mark.parametrize("z_bf16", [False, True])
@pytest.mark.parametrize("shape", LR_CPU)
def test_fdec_lr_bounds(shape, z_bf16):
    NI, P, Hd, W, Co, H_skip, C_skip = shape
    c = dc.lr_case(43, NI, P, Hd, W, Co, H_skip, C_skip, z_bf16)
    v3s, v3m = dc.lr_v3_stats(c), dc.lr_v3_merge(c, z_bf16)
    Y, tY = kr.fdec_lr_ref(c["Z"], c["Zs"], c["bias"], Hd, P, v3=v3s)
    Y32 = dc.lr_emulate(c, v3s)
    assert _inside(Y32.astype(np.float64), Y, tY) <= 1.0
    st, tst = kr.fdec_lr_stats_ref(Y, tY, Hd)
    assert _inside(dc.lr_stats_emulate(Y32), st, tst) <= 1.0
    # the merge pass reads statistics from memory: exact inputs (here the exact sums)
    Ym, tYm = (Y, tY) if v3m == v3s else kr.fdec_lr_ref(c["Z"], c["Zs"], c["bias"], Hd, P, v3=v3m)
    D1, tD = dc.lr_merge_ref(c, Ym, tYm, st, fast=z_bf16, v3=v3m)
    assert _inside(dc.lr_merge_emulate(c, dc.lr_emulate(c, v3m), st, z_bf16, v3m), D1, tD) <= 1.0

    def mutated(**kw):
        Z, Zs, bias = kw.get("Z", c["Z"]), kw.get("Zs", c["Zs"]), kw.get("bias", c["bias"])
        return kr.fdec_lr_ref(Z, Zs, bias, Hd, P, v3=v3s)[0]

    muts = {}
    nseg = NI // P
    if nseg > 1:
        muts["skip_next_seg"] = mutated(Zs=np.roll(c["Zs"], -1, axis=0))
    muts["taps34"] = mutated(Z=c["Z"][:, :, :, [0, 1, 2, 4, 3, 5, 6, 7]], Zs=c["Zs"][:, :, :, [0, 1, 2, 4, 3, 5, 6, 7]])
    muts["no_bias"] = mutated(bias=0 * c["bias"])
    muts["no_gain"] = mutated(Zs=c["Zs"] * 10.0)
    if Hd != c["Hs"]:
        i0, i1, l0, l1 = kr.lin_index_ref(c["Hs"], Hd)
        a = np.take(c["Z"], i0, axis=1)
        s, _ = kr.resize_h_ref(c["Zs"], Hd)
        D0 = a + kr.SKIP_GAIN * s[np.arange(NI) // P]                # i1 taken as i0: the lerp collapses to row i0
        Ym2 = np.zeros_like(Y)
        for k in range(8):
            o = 4 * np.arange(Hd) - 2 + k
            ok = (o >= 0) & (o < 4 * Hd)
            Ym2[:, o[ok]] += D0[:, :, :, k][:, ok]
        muts["i1_as_i0"] = Ym2 + c["bias"]
    for name, Ymut in muts.items():
        _outside(Ymut, Y, tY, "fdec_lr_rows", name)
        if not (name == "taps34" and Hd == 1):      # (one step: the swap only permutes its four rows)
            _outside(dc.true_stats(Ymut), st, tst, "fdec_lr_stats", name)
    # statistics: one row short, and residues 0 and 3 left out
    _outside(dc.true_stats(Y[:, :-1]), st, tst, "fdec_lr_stats", "count_row")
    _outside(dc.true_stats(Y[:, np.arange(4 * Hd) % 4 % 3 != 0]), st, tst, "fdec_lr_stats", "res03")
    # merge pass
    for mut in ["skip_next_seg", "skip_prompt", "no_gain", "gn_next_item"]:
        if mut in ("skip_next_seg", "skip_prompt") and nseg == 1:
            continue
        _outside(dc.lr_merge_ref(c, Ym, tYm, st, fast=z_bf16, v3=v3m, mut=mut)[0], D1, tD, "fdec_lr_merge", mut)
    for name in ("taps34", "no_bias")[Hd == 1:]:       # (one step: rows 1 and 2 swap under the 0.5 / 0.5 resize)
        _outside(dc.lr_merge_ref(c, muts[name], tYm, st, fast=z_bf16, v3=v3m)[0], D1, tD, "fdec_lr_merge", name)
    m2 = kr.dec_merge_ref(Ym, c["skip"], Hd, P, stats=st, gn_count=(4 * Hd - 1) * W * Co, gn_w=c["gn_w"], gn_b=c["gn_b"],
                          fast=z_bf16, folded=v3m, kept=True, out_bf16=c["out_bf16"])[0]
    _outside(m2, D1, tD, "fdec_lr_merge", "count_row")


# ===================================================================================================== fdec1_gram
@pytest.mark.parametrize("mean", [0.0, 30.0])
def test_fdec1_gram_bounds(mean):
    """the Gram form of the level-1 statistics: the emulation (float32 Gram matrices, fp64 quadratic forms) stays inside
    fdec1_gram_stats_ref's bound at mean 0 and in the large-mean regime; mutations of the rows, of the statistics' row
    set and of the last w tile's column mask land outside"""
    NI, P, Hd, W = 4, 2, 33, 11
    c = dc.gram_case(61, NI, P, Hd, W, mean=mean)
    st, tol, Y = kr.fdec1_gram_stats_ref(c["Z"], c["amb"], c["Zs"], c["bias"], Hd, P)
    assert _inside(dc.gram_emulate(c), st, tol) <= 1.0
    fam = "fdec1_gram"
    _outside(dc.gram_emulate(c, double_count=True), st, tol, fam, "w_tile_double_count")
    _outside(dc.true_stats(Y[:, :-1]), st, tol, fam, "count_row")
    _outside(dc.true_stats(Y[:, np.arange(4 * Hd) % 4 % 3 != 0]), st, tol, fam, "res03")
    mut = lambda **kw: dc.true_stats(kr.fdec_lr_ref(kw.get("Z", c["Z"]), kw.get("Zs", c["Zs"]), kw.get("bias", c["bias"]),
                                                    Hd, P)[0])
    if mean == 0.0:          # (at mean 30 the skip branch and the bias are below one rounding of the main term)
        _outside(mut(Zs=np.roll(c["Zs"], -1, axis=0)), st, tol, fam, "skip_next_seg")
        _outside(mut(Zs=10.0 * c["Zs"]), st, tol, fam, "no_gain")
        _outside(mut(bias=0 * c["bias"]), st, tol, fam, "no_bias")
    _outside(mut(Z=c["Z"][:, :, :, [0, 1, 2, 4, 3, 5, 6, 7]], Zs=c["Zs"][:, :, :, [0, 1, 2, 4, 3, 5, 6, 7]]), st, tol, fam,
             "taps34")
    _outside(mut(Z=np.roll(c["Z"], 1, axis=0)), st, tol, fam, "item_next")


def test_zz_separation_report(capsys):
    """prints the smallest mutation-to-tol ratio per family (the figures quoted with the GPU report)"""
    with capsys.disabled():
        for fam in sorted(SEPARATION):
            print("separation %-14s %.3g" % (fam, SEPARATION[fam]))
    assert all(v > 10.0 for v in SEPARATION.values())
