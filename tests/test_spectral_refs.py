"""CPU checks of tests/spectral_refs.py and of the host code behind tests/test_gpu_spectral.py: the struct sizes of
libathd_ktest.so, the product's pad plan (kernels.h stft_pad_plan) and the iSTFT's frame split (spectral.hip
istft_ola_split).  No GPU.

* Every reference equals torch / the oracle in float64 to 1e-10 relative: oracle.htdemucs_ref pad1d and torch.stft with
  the same window (HTDemucsHot._spec builds torch's own float32 window: 1e-6), torch.istft(normalized=True, center=True)
  on the reference's masked spectrum, F.conv1d + F.gelu, the oracle's embedding functions.
* stft_pad_plan equals the pad1d rule for every T in 1 .. 5000 and a sample of larger T, and ext_left is 0 for all of
  them (the right pad is never smaller than the left one, so pad1d's zero extension never reaches the left side): the
  `ext_left` branch of pad_sample needs the explicit plan of the GPU test.
* The frame split for every Tspec in 1 .. 20000: (n - 1) g < Tspec <= n g, g <= 32, for n > 1 g >= 3 and the last
  workgroup >= 3 frames, part floats = NI n 12288; first rejected candidate at Tspec = 962.
* torch's float32 transforms against float64 on these inputs, |x32 - x64|_2 / |x64|_2 (worst frame / hop block):
  stft r32 = 1.29e-7, istft r32i = 1.50e-7 (measured; spectral_refs.R32 = R32I = 2.0e-7 is asserted to lie above them by less
  than a factor 2).
* The running-product twiddles: the float32 chains of all 256 threads and both bases stay inside
  d_r e = (r + (r - 1) sqrt 5) e; the largest error measured over all of them is 11.0 e (asserted < 15 e: the "<= 15 ulp"
  of spectral.hip holds as a measurement; the derived worst case is d_15 = 46.3 e).
* The bounds are not vacuous: the float32 emulations of tests/spectral_cases.py stay inside every criterion (both L2
  criteria included) and every mutation lands more than 10x outside at least one.  SEPARATION records the smallest
  ratio per family (the assertion is the 10x bar): stft 134, istft 8.9e3, tconv0 3.0e3.
* Identities, left out as mutations: dropping the 1e-8 of the phase division (with |Re L|, |Im L| >= 0.25 it is below
  half a float32 ulp of the denominator: asserted bit-identical in the emulation).
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import spectral_cases as sc
import spectral_refs as sr
from oracle import htdemucs_ref as orc


@pytest.fixture(scope="module")
def ktl():
    import ktest
    return ktest


@pytest.fixture(scope="module")
def tb():
    return sr.tables()


# smallest mutation-to-bound ratio per family at the shapes of this file (measured; every one is asserted > 10)
SEPARATION = {}


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _ew(got, R, tol):
    return float((np.abs(got - R) / np.maximum(tol, 1e-300)).max())


def _sep(family, name, *ratios):
    r = max(ratios)
    SEPARATION[family] = min(SEPARATION.get(family, np.inf), r)
    assert r > 10.0, (family, name, ratios)


# ============================================================================================ host code
def test_struct_sizes(ktl):
    m = ktl.sizes_match()
    assert {"stft", "istft", "tconv0", "textvec"} <= set(m)
    for name, (a, b) in m.items():
        assert a == b, (name, a, b)


def test_pad_plan(ktl):
    Ts = list(range(1, 5001)) + [5119, 5120, 5121, 44100, 264600, 2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1, 10 ** 7 + 3]
    for T in Ts:
        le = -(-T // 1024)
        got = ktl.stft_pad_plan(T, le)
        assert got == sr.pad_plan_ref(T), (T, got)
        assert got[2] == 0 and got[0] == T
    for T in (1, 2, 600, 1023, 1024, 1025, 1536, 1537, 2559, 2560, 2561, 4097):
        le = -(-T // 1024)
        x = torch.arange(1, T + 1, dtype=torch.float64)[None]
        want = orc.pad1d(x, (1536, 1536 + le * 1024 - T), mode="reflect")[0].numpy()
        got = sr.pad1d_ref(x.numpy()[0], ktl.stft_pad_plan(T, le), np.arange(want.size))
        assert (got == want).all(), T


def test_handmade_plan():
    """the explicit plan of the GPU test (zero extension on both sides) is pad1d's composition of the two pads"""
    T, left, el, Lx = 600, 1236, 300, 1537
    x = torch.arange(1, T + 1, dtype=torch.float64)[None]
    want = Fn.pad(Fn.pad(x, (el, Lx - T - el)), (left, 4096 - left - Lx), mode="reflect")[0].numpy()
    got = sr.pad1d_ref(x.numpy()[0], (T, left, el, Lx), np.arange(4096))
    assert (got == want).all()
    assert got[left + el] == 1 and got[left + el - 1] == 0 and got[left - el] == 1


def test_frame_split(ktl):
    first_reject = None
    for Ts in range(1, 20001):
        n, g = ktl.lib.kt_istft_nwg(Ts), ktl.lib.kt_istft_frames(Ts)
        assert (n, g) == sr.ola_split_ref(Ts), Ts
        assert (n - 1) * g < Ts <= n * g and g <= 32, (Ts, n, g)
        if n > 1:
            assert g >= 3 and Ts - (n - 1) * g >= 3, (Ts, n, g)
        if first_reject is None and n != (Ts + 31) // 32:
            first_reject = Ts
        if Ts % 97 == 0 or Ts < 70:
            assert ktl.lib.kt_istft_part_floats(3, Ts) == 3 * n * 12288
    assert first_reject == 962
    assert sr.ola_split_ref(33) == (2, 17) and sr.ola_split_ref(65) == (3, 22) and sr.ola_split_ref(931) == (30, 32)
    assert 931 - 29 * 32 == 3 and sr.ola_split_ref(962) == (34, 29) and 962 - 33 * 29 == 5


# ============================================================================================ references vs torch
def test_window(tb):
    """torch evaluates its float32 window in float32 (2e-7 absolute from the double formula the product rounds once), so
    the oracle's own _spec is compared at 1e-6 and the 1e-10 comparisons pass the product's window to torch"""
    w = torch.hann_window(4096).numpy()
    assert np.abs(w.astype(np.float64) - tb.win).max() <= 2.0 ** -21
    k = np.arange(4096)
    assert (tb.win == (0.5 - 0.5 * np.cos(2 * np.pi * k / 4096)).astype(np.float32)).all()
    assert (tb.win2 == tb.win * tb.win).all() and tb.win2.dtype == np.float32


def _torch_spec(wav, win, dtype):
    """HTDemucs._spec with the given window"""
    x = torch.as_tensor(wav).to(dtype)
    T = x.shape[-1]
    le = -(-T // 1024)
    xp = orc.pad1d(x, (1536, 1536 + le * 1024 - T), mode="reflect")
    z = torch.stft(xp.reshape(-1, xp.shape[-1]), 4096, 1024, window=torch.as_tensor(win).to(dtype), win_length=4096,
                   normalized=True, center=True, return_complex=True, pad_mode="reflect")
    z = z[:, :-1, 2:2 + le].reshape(x.shape[0], 2, 2048, le)
    z = z.permute(0, 3, 2, 1).numpy()                        # [nb][t][f][channel]
    return np.stack([z[..., 0].real, z[..., 0].imag, z[..., 1].real, z[..., 1].imag], axis=-1).astype(np.float64)


@pytest.mark.parametrize("shape", [(1, 1), (2, 600), (1, 1500), (2, 9999)])
def test_stft_ref(tb, shape):
    nb, T = shape
    wav = sc.stft_case(nb, T)
    le = -(-T // 1024)
    R = sr.stft_ref(wav, sr.pad_plan_ref(T), le, tb.win, False, round_frame=False).R
    assert _rel(R, _torch_spec(wav, tb.win, torch.float64)) < 1e-10
    m = SimpleNamespace(hop_length=1024, nfft=4096)
    z = orc.HTDemucsHot._spec(m, torch.as_tensor(wav).double()).permute(0, 3, 2, 1).numpy()
    assert _rel(R[..., 0] + 1j * R[..., 1], z[..., 0]) < 1e-6 and _rel(R[..., 2] + 1j * R[..., 3], z[..., 1]) < 1e-6
    # the float32 frame product the kernel documents moves the result by no more than e |frame|_2
    r = sr.stft_ref(wav, sr.pad_plan_ref(T), le, tb.win, False)
    assert (np.abs(r.R - R) <= sr.E32 * r.fn[..., None, None] * 1.01 + 1e-300).all()


def test_r32(tb):
    wav = sc.stft_case(2, 9999)
    a, b = _torch_spec(wav, tb.win, torch.float32), _torch_spec(wav, tb.win, torch.float64)
    r = float(sr.l2_ratio(a, b, (2, 3)).max())
    print("r32 = %.3g" % r)
    assert sr.R32 / 2 < r <= sr.R32


def _split_lr(Pk):
    k = np.arange(sr.NB)
    a, b = Pk[:, k], np.conj(Pk[:, (sr.NFFT - k) % sr.NFFT])
    return (a + b) / 2, (a - b) / 2j


def _torch_ispec(Pk, T, win, cdtype):
    """HTDemucs._ispec of the two channels packed in Pk [Tspec][4096]"""
    z = torch.as_tensor(np.stack(_split_lr(Pk))).permute(0, 2, 1).to(cdtype)          # [2][2048][Tspec]
    z = Fn.pad(Fn.pad(z, (0, 0, 0, 1)), (2, 2))
    le = 1024 * -(-T // 1024) + 3072
    x = torch.istft(z, 4096, 1024, window=torch.as_tensor(win).to(z.real.dtype), win_length=4096, normalized=True,
                    length=le, center=True)
    return x[:, 1536:1536 + T].numpy().astype(np.float64)


ISTFT_CPU = [(1, 1000, 1, 1), (3, 3072, 2, 2), (33, 33297, 2, 2)]


@pytest.fixture(scope="module")
def istft_refs(tb):
    out = {}
    for shp in ISTFT_CPU:
        c = sc.istft_case(*shp)
        out[shp] = (c, {f: sr.istft_ref(c["fo"], c["spec"], c["xt2"], c["tnorm"], c["P"], c["T"], tb.win, f)
                        for f in (False, True)})
    return out


@pytest.mark.parametrize("shape", ISTFT_CPU)
def test_istft_ref(tb, istft_refs, shape):
    c, refs = istft_refs[shape]
    r = refs[False]
    want = _torch_ispec(r.Pk, c["T"], tb.win, torch.complex128)
    assert _rel(r.Rf[0], want) < 1e-10
    mean, std = c["tnorm"][0].astype(np.float64)
    assert _rel(r.R[0], want + c["xt2"][0].T.astype(np.float64) * std + mean) < 1e-10
    # the masked spectrum itself, from the formula of ATHTDemucs_v2.py:297-309 in torch
    fo = torch.as_tensor(c["fo"][0]).double().permute(2, 1, 0)[None]                  # (1, 2, rows, t)
    mask = torch.sigmoid(Fn.interpolate(fo, size=(2048, c["Tspec"]), mode="bilinear", align_corners=False))[0]
    sp = torch.as_tensor(c["spec"][0]).double().permute(2, 1, 0)                      # (4, f, t)
    zs = torch.complex(sp[[0, 2]], sp[[1, 3]])
    mz = (sp[:2] * mask) * (zs / (sp[:2] + 1e-8))
    SL, SR = _split_lr(r.Pk)
    got = np.stack([SL, SR]).transpose(0, 2, 1)
    want = mz.numpy().copy()
    want[:, 0, :] = want[:, 0, :].real                       # torch.istft ignores the DC bin's imaginary part
    assert _rel(got, want) < 1e-6                            # (float32 lerp weights against float64 ones)


def test_r32i(tb, istft_refs):
    c, refs = istft_refs[(33, 33297, 2, 2)]
    Pk = refs[False].Pk
    SL, SR = _split_lr(Pk)
    Pk32 = np.zeros_like(Pk)
    # (the float32 input spectrum for both, so that only the transform's arithmetic differs)
    SL32, SR32 = SL.astype(np.complex64).astype(np.complex128), SR.astype(np.complex64).astype(np.complex128)
    Pk32[:, :sr.NB] = SL32 + 1j * SR32
    Pk32[:, sr.NFFT - 1:sr.NB:-1] = (np.conj(SL32) + 1j * np.conj(SR32))[:, 1:]
    a = _torch_ispec(Pk32, c["T"], tb.win, torch.complex64)[None]
    b = _torch_ispec(Pk32, c["T"], tb.win, torch.complex128)[None]
    r = float(sr.block_l2(a, b, b, c["T"]).max())
    print("r32i = %.3g" % r)
    assert sr.R32I / 2 < r <= sr.R32I


@pytest.mark.parametrize("bf16", [False, True])
def test_tconv0_ref(bf16):
    c = sc.tconv0_case(2, 1023)
    R, tol = sr.tconv0_ref(c["wav"], c["tnorm"], c["w"], c["bias"], bf16)       # (R is the value before a bf16 store)
    x = (torch.as_tensor(c["wav"]).double() - torch.as_tensor(c["tnorm"][:, 0]).double()[:, None, None]) / \
        torch.as_tensor(c["tnorm"][:, 1]).double()[:, None, None]
    x = Fn.pad(x, (0, 4 * c["Lo"] - c["T"]))
    w = torch.as_tensor(c["w"]).double().reshape(48, 8, 2).permute(0, 2, 1)            # [48][c][tap]
    y = Fn.conv1d(x, w, torch.as_tensor(c["bias"]).double(), stride=4, padding=2)
    assert y.shape[-1] == c["Lo"]
    want = Fn.gelu(y, approximate="tanh") if bf16 else Fn.gelu(y)
    assert _rel(R, want.permute(0, 2, 1).numpy()) < 1e-10


def test_text_vec_ref():
    c = sc.textvec_case(6, 3, 0)
    (a, c0, c2), (ta, tc0, tc2) = sr.text_vec_ref(c["text"], 6, 3, 0, c["maT"], c["ma"], c["mcT"], c["mc"], c["b2"])
    t = torch.as_tensor(c["text"]).double()
    want = t @ torch.as_tensor(c["maT"]).double() + torch.as_tensor(c["ma"]).double()
    assert _rel(a[:3], want.numpy()) < 1e-12 and (a[3:] == a[:3]).all() and (c2 == a + c["b2"].astype(np.float64)).all()
    (a1, _, _), _ = sr.text_vec_ref(np.tile(c["text"], (2, 1)), 6, 3, 1, c["maT"], c["ma"], c["mcT"], c["mc"], c["b2"])
    assert (a1 == a).all() and (tc2 >= ta).all() and ta.min() > 0


def test_pos_refs():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        for T1 in (1, 33):
            want = orc.create_2d_sin_embedding(512, 8, T1)[0].permute(1, 2, 0).reshape(8 * T1, 512).numpy()
            assert np.abs(sr.pos2d_ref(8, T1, 512, exact=True)[0] - want).max() < 1e-10
        for T2 in (1, 259):
            want = orc.create_sin_embedding(T2, 512)[:, 0, :].numpy()
            assert np.abs(sr.pos1d_ref(T2, 512, exact=True)[0] - want).max() < 1e-10
    finally:
        torch.set_default_dtype(old)
    # the float32 roundings of k, cc k and a / (half - 1) move the exponent by up to 2e ln(1e4) = 18e, i.e. the phase
    # by 18e |ph|: more than the kernels' bound of 3e |ph|, which is why the references reproduce them
    for (R, tol), Rx in ((sr.pos2d_ref(8, 293, 512), sr.pos2d_ref(8, 293, 512, True)[0]),
                         (sr.pos1d_ref(1145, 512), sr.pos1d_ref(1145, 512, True)[0])):
        assert (np.abs(R - Rx) <= 7 * tol).all() and not (np.abs(R - Rx) <= tol).all()


# ============================================================================================ the bounds are not vacuous
def test_fft_emulation_structure(tb):
    """the emulated pass structure in float64 with table twiddles is the DFT"""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3, 4096)) + 1j * rng.standard_normal((3, 4096))
    assert _rel(sc.fft4096_emu(x, sc._ctab(tb.tw64), False), np.fft.fft(x, axis=-1)) < 1e-12


def test_running_twiddles(tb):
    tw, j = sc._ctab(tb.tw), np.arange(256)
    worst = 0.0
    for idx in (16 * (j & 15), j):
        p = sc.tw_powers(tw, idx, True)
        for r in range(1, 16):
            ex = np.exp(-2j * np.pi * (idx * r) / 4096.0)
            err = float(np.abs(p[r].astype(np.complex128) - ex).max()) / sr.E32
            assert err <= max(sr.tw_err(r), 1.0), (r, err)
            worst = max(worst, err)
    print("running twiddles: worst error %.2f e" % worst)
    assert worst < 15.0


STFT_EMU = (2, 9999)


@pytest.mark.parametrize("fast", [False, True])
def test_stft_bounds(tb, fast):
    nb, T = STFT_EMU
    wav, plan, le = sc.stft_case(nb, T), sr.pad_plan_ref(T), -(-T // 1024)
    r = sr.stft_ref(wav, plan, le, tb.win, fast)
    crit = lambda got: (_ew(got, r.R, r.tol), float(sr.l2_ratio(got, r.R, (2, 3)).max()) / sr.L2_STFT if fast else 0.0)
    got = sc.stft_emu(wav, plan, le, tb, fast)
    inside = crit(got)
    print("stft emulation fast=%d: err/tol %.3g, L2/bound %.3g" % (fast, *inside))
    assert max(inside) <= 1.0
    st, _ = sr.kr.stats_of(got, np.zeros_like(got), n_part=0)
    assert (np.abs(st - r.stats) <= r.stats_tol).all()
    for mut in ("window", "frame", "reflect", "im_sign"):
        _sep("stft", mut, *crit(sr.stft_ref(wav, plan, le, tb.win, fast, mut=mut).R))
    if fast:
        for mut in ("entry", "base"):
            _sep("stft", mut, *crit(sc.stft_emu(wav, plan, le, tb, True, mut=mut)))


def test_istft_bounds(tb, istft_refs, ktl):
    shape = (33, 33297, 2, 2)
    c, refs = istft_refs[shape]
    split = sr.ola_split_ref(c["Tspec"])
    assert split == (2, 17)
    got = sc.istft_emu(c, tb, split)
    assert (sc.istft_emu(c, tb, split, mut="no_eps") == got).all()       # dropping the 1e-8: an identity at these inputs
    crit = {}
    for fast in (False, True):
        r = refs[fast]
        crit[fast] = lambda g, r=r, fast=fast: (
            _ew(g, r.R, r.tol), float(sr.block_l2(g, r.R, r.Rf, c["T"]).max()) / sr.L2_ISTFT if fast else 0.0)
    inside = crit[True](got)
    print("istft emulation: err/tol %.3g, L2/bound %.3g" % inside)
    assert max(inside) <= 1.0
    inside = crit[False](sc.istft_emu(c, tb, split, fast=False))        # the f32 mode: double FFT, exact mask arithmetic
    print("istft emulation, f32 mode: err/tol %.3g" % inside[0])
    assert inside[0] <= 1.0
    for mut in ("env3", "tail", "head", "edge"):
        gm = sc.istft_emu(c, tb, split, mut=mut)
        _sep("istft", mut, *crit[True](gm))
    kw = dict(P=c["P"], T=c["T"], win=tb.win, fast=True)
    for mut in ("nyquist", "dc_imag", "l_swap"):
        _sep("istft", mut, *crit[True](sr.istft_ref(c["fo"], c["spec"], c["xt2"], c["tnorm"], mut=mut, **kw).R))
    fo_b = c["fo"][np.arange(c["NI"]) // c["P"]]                          # `b` instead of `item` for fo
    _sep("istft", "fo_b", *crit[True](sr.istft_ref(fo_b, c["spec"], c["xt2"], c["tnorm"], **kw).R))
    _sep("istft", "tnorm", *crit[True](sr.istft_ref(c["fo"], c["spec"], c["xt2"], c["tnorm"][::-1], **kw).R))


@pytest.mark.parametrize("bf16", [False, True])
def test_tconv0_bounds(bf16):
    c = sc.tconv0_case(2, 1023)
    R, tol = sr.tconv0_ref(c["wav"], c["tnorm"], c["w"], c["bias"], bf16)
    inside = _ew(sc.tconv0_emu(c, bf16), R, tol)
    print("tconv0 emulation bf16=%d: err/tol %.3g" % (bf16, inside))
    assert inside <= 1.0
    Rm, _ = sr.tconv0_ref(c["wav"], c["tnorm"], c["w"], c["bias"], bf16, mut="pad_sub")
    assert (Rm[:, 1:-1] == R[:, 1:-1]).all()                 # only the rows that touch the padding move
    _sep("tconv0", "pad_sub", _ew(Rm, R, tol))


def test_separation_complete():
    """runs last in this file: every family that ran (all three in a full run) has a figure above 10"""
    assert set(SEPARATION) <= {"stft", "istft", "tconv0"}, SEPARATION
    print("SEPARATION", {k: float("%.3g" % v) for k, v in SEPARATION.items()})
    assert all(v > 10.0 for v in SEPARATION.values()), SEPARATION
