"""Kernel-level parity of the track level (csrc/track.hip) through the product ABI: ola_kernel (athd_overlap_add),
ola_weighted_kernel (athd_overlap_add_weighted), ola_normalize_kernel (athd_ola_normalize) and the sdr_* / sisdr_*
kernels (athd_sdr, athd_sisdr), against the float64 references, derived bounds and float32 restatements of
tests/track_refs.py at the small shapes where these kernels can break (tests/test_gpu_track.py and
tests/test_gpu_benchmark.py run them at the workload's one plan per mode).

Overlap-add, all 130 (chunk, overlap, L) cases of track_refs.cases() with 1 and 3 stems:
* every window's samples at j >= len_k are NaN, the windows sit between guard bands, and the output has one more row
  and a band of sentinels: the result must be finite and the sentinels untouched;
* |got - ref64| <= the per-sample bound (mode 0 where the reference exists, mode 1 on acc, wsum and the normalised
  output);
* got is bit-equal to the float32 restatement: the kernels promise the reference's float32 operations in the
  reference's order, with no fma contraction.  This is an equality, not a tolerance;
* window ranges [0, a) and [a, n) for every cut of every case with n <= 12 windows, each call seeing only its own
  windows (NaN elsewhere): each span is bit-equal to the restatement of its range, and the spans added in rank order
  (mode 1: then athd_ola_normalize) are bit-equal to the one-range result at every sample of track_refs.rank_mask and
  within the float64 bound everywhere.  rank_mask is every sample when overlap <= hop (asserted), which is every plan
  the product runs; with hop < overlap a sample can have several covering windows in the second range, whose terms
  are then added among themselves before the first range's sum: float addition does not re-associate, so no kernel
  that returns per-range sums can be bit-equal there (measured: 18 % to 38 % of such samples differ in the last bits);
* refused calls return ATHD_EINVAL and write nothing.

SDR / SI-SDR, every family of track_refs.FAMILIES and 'mixed' at rows {1, 3} x n {1, 63, 64, 65, 255, 256, 257, 1000,
262144 + 257} and 65535 rows of 2: |got - ref64| <= 4e-6 dB (track_refs.TOL_DB), calls whose rows all clamp equal +-30.0
exactly, silence gives exactly 0.0, `out` and the scratch (filled with sentinels, banded past the documented size)
are touched nowhere else; no run-to-run bit equality is asked (fp64 atomics order the block sums).

Each case's worst err / bound (metrics: worst |err| in dB) goes to $ATHD_OUT/kernel_parity_track_report.json.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import track_refs as tr
from test_gpu_kernels import kt  # noqa: F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu

EINVAL = -1
PAIR_IDS = ["%d-%d" % p for p in tr.PAIRS]
BY_PAIR = {p: [c for c in tr.cases() if c[:2] == p] for p in tr.PAIRS}


def _lib():
    import athd.native as native
    return native.lib


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _sent(kt, n):
    return np.full(n, kt.F32_SENTINEL, dtype=np.float32)


def _out(kt, n, guard=1024):
    return kt.Buf(_sent(kt, n), "f32", guard, output=True)


def _untouched(kt, buf):
    raw, bands = buf.host()
    return bands and bool((raw == np.float32(kt.F32_SENTINEL)).all())


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def _ratio(got, ref, bound):
    got = got.astype(np.float64)
    r = np.abs(got - ref) / np.maximum(bound, 1e-300)
    r[(bound == 0) & (got == ref)] = 0.0
    r[~np.isfinite(got)] = np.inf
    return float(r.max())


@functools.lru_cache(maxsize=None)
def _case(c, o, L, S):
    """data, references and restatements of one case: computed once, shared by the tests below, never modified"""
    win = tr.ola_windows(c, o, L, S, poison=True)
    r = SimpleNamespace(win=win, n=win.shape[0], r1=tr.ola1_ref(win, L, c, o), f1=tr.ola1_f32(win, L, c, o),
                        r0=tr.ola0_ref(win, L, c, o) if tr.in_domain0(L, c, o) else None, f0=tr.ola0_f32(win, L, c, o))
    for a in (win, r.f0) + tuple(r.f1):
        a.setflags(write=False)
    return r


def _ola(kt, mode, wbuf, first, c, o, L, S, k0, k1, partial=False):
    """one launch over windows [k0, k1); wbuf holds window `first` at its start.  -> (out [S][2][span], wsum or None)
    after checking the extra output row, the tail of wsum and all bands"""
    span = tr.span_of(L, c, o, k0, k1)[1]
    bo = _out(kt, (2 * S + 1) * span)
    bw = _out(kt, 2 * span) if partial else None
    wptr = wbuf.ptr + 4 * (k0 - first) * S * 2 * c
    lib = _lib()
    if mode == 0:
        rc = lib.athd_overlap_add(wptr, L, c, o, S, k0, k1, bo.ptr, _stream())
    else:
        rc = lib.athd_overlap_add_weighted(wptr, L, c, o, S, k0, k1, bo.ptr, bw.ptr if partial else None, _stream())
    assert rc == 0, rc
    kt.sync()
    raw, bands = bo.host()
    assert bands, "output band overwritten"
    assert (raw[2 * S * span:] == np.float32(kt.F32_SENTINEL)).all(), "row past the output written"
    out = raw[:2 * S * span].reshape(S, 2, span)
    assert np.isfinite(out).all(), "a sample past len_k or of a window outside [k0, k1) was read"
    ws = None
    if partial:
        raw, bands = bw.host()
        assert bands and (raw[span:] == np.float32(kt.F32_SENTINEL)).all(), "wsum written past the span"
        ws = raw[:span]
        assert np.isfinite(ws).all()
    return out, ws


def _rec(kt, case, **kw):
    kt.record(case, report=kt.TRACK_REPORT, **kw)


# ========================================================================================================== overlap-add
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("pair", tr.PAIRS, ids=PAIR_IDS)
def test_overlap_add(kt, pair, S):
    c, o = pair
    fails, in_domain = [], 0
    for _, _, L in BY_PAIR[pair]:
        r = _case(c, o, L, S)
        got, _ = _ola(kt, 0, kt.Buf(r.win, "f32", 4096), 0, c, o, L, S, 0, r.n)
        bits = _bits(got, r.f0)
        ratio = _ratio(got, r.r0.out, r.r0.bound) if r.r0 is not None else None
        in_domain += r.r0 is not None
        print("ola0[%d,%d,%d,S%d]: err/bound %s bits %s" % (c, o, L, S, ratio, bits))
        _rec(kt, "ola0[%d,%d,%d,S%d]" % (c, o, L, S), err_over_bound=ratio, bit_equal=bits, windows=r.n)
        if not bits or (ratio is not None and ratio > 1.0):
            fails.append((L, ratio, bits))
    assert not fails, fails
    assert in_domain == sum(tr.in_domain0(L, c, o) for _, _, L in BY_PAIR[pair])


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("pair", tr.PAIRS, ids=PAIR_IDS)
def test_overlap_add_weighted(kt, pair, S):
    c, o = pair
    fails = []
    for _, _, L in BY_PAIR[pair]:
        r = _case(c, o, L, S)
        wbuf = kt.Buf(r.win, "f32", 4096)
        q, _ = _ola(kt, 1, wbuf, 0, c, o, L, S, 0, r.n)
        acc, ws = _ola(kt, 1, wbuf, 0, c, o, L, S, 0, r.n, partial=True)
        bits = {"acc": _bits(acc, r.f1[0]), "wsum": _bits(ws, r.f1[1]), "q": _bits(q, r.f1[2])}
        ratio = {"acc": _ratio(acc, r.r1.acc, r.r1.b_acc), "wsum": _ratio(ws, r.r1.ws, r.r1.b_ws),
                 "q": _ratio(q, r.r1.q, r.r1.b_q)}
        print("ola1[%d,%d,%d,S%d]: err/bound %s bits %s" % (c, o, L, S, ratio, bits))
        _rec(kt, "ola1[%d,%d,%d,S%d]" % (c, o, L, S), err_over_bound=ratio, bit_equal=bits, windows=r.n,
             max_cover=int(r.r1.m.max()))
        if not all(bits.values()) or max(ratio.values()) > 1.0:
            fails.append((L, ratio, bits))
    assert not fails, fails


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("pair", tr.PAIRS, ids=PAIR_IDS)
def test_window_ranges(kt, pair, S):
    c, o = pair
    lib = _lib()
    fails, cuts, reassoc = [], 0, [0, 0]
    for _, _, L in BY_PAIR[pair]:
        r = _case(c, o, L, S)
        if not 2 <= r.n <= 12:
            continue
        full = kt.Buf(r.win, "f32", 4096)
        one0, _ = _ola(kt, 0, full, 0, c, o, L, S, 0, r.n)
        one1, _ = _ola(kt, 1, full, 0, c, o, L, S, 0, r.n)
        for a in range(1, r.n):
            cuts += 1
            mask = tr.rank_mask(L, c, o, a)
            assert mask.all() or o > c - o
            track = np.zeros((S, 2, L), dtype=np.float32)
            acc = np.zeros((S, 2, L), dtype=np.float32)
            wsum = np.zeros(L, dtype=np.float32)
            why = []
            for k0, k1 in ((0, a), (a, r.n)):
                own = np.full_like(r.win, np.nan)
                own[k0:k1] = r.win[k0:k1]
                wb = kt.Buf(own, "f32", 4096)
                t0, span = tr.span_of(L, c, o, k0, k1)
                s0, _ = _ola(kt, 0, wb, 0, c, o, L, S, k0, k1)
                s1, w1 = _ola(kt, 1, wb, 0, c, o, L, S, k0, k1, partial=True)
                f1 = tr.ola1_f32(r.win, L, c, o, k0, k1)
                if not (_bits(s0, tr.ola0_f32(r.win, L, c, o, k0, k1)) and _bits(s1, f1[0]) and _bits(w1, f1[1])):
                    why.append("span [%d,%d) differs from its restatement" % (k0, k1))
                track[:, :, t0:t0 + span] += s0
                acc[:, :, t0:t0 + span] += s1
                wsum[t0:t0 + span] += w1
            # finish on the device: athd_ola_normalize over the 2 S rows, one sentinel row behind them
            bq = kt.Buf(np.concatenate([acc.ravel(), _sent(kt, L)]), "f32", 1024, output=True)
            bw = kt.Buf(wsum, "f32", 1024)
            assert lib.athd_ola_normalize(bq.ptr, bw.ptr, 2 * S, L, _stream()) == 0
            kt.sync()
            raw, bands = bq.host()
            assert bands and (raw[2 * S * L:] == np.float32(kt.F32_SENTINEL)).all()
            q = raw[:2 * S * L].reshape(S, 2, L)
            if not _bits(track[..., mask], one0[..., mask]):
                why.append("mode 0 spans do not recombine bit for bit")
            if not _bits(q[..., mask], one1[..., mask]):
                why.append("mode 1 spans do not recombine bit for bit")
            if _ratio(q, r.r1.q, r.r1.b_q) > 1.0 or (r.r0 is not None and _ratio(track, r.r0.out, r.r0.bound) > 1.0):
                why.append("recombined track outside the float64 bound")
            reassoc[0] += int((~mask).sum()) * 2 * S
            reassoc[1] += int((q[..., ~mask].view(np.uint32) != one1[..., ~mask].view(np.uint32)).sum())
            if why:
                fails.append((L, a, why))
    print("ranges[%d,%d,S%d]: %d cuts, %d samples outside rank_mask, %d of them differ" % (c, o, S, cuts, *reassoc))
    _rec(kt, "ranges[%d,%d,S%d]" % (c, o, S), cuts=cuts, failed=len(fails), outside_rank_mask=reassoc[0],
         outside_rank_mask_differ=reassoc[1])
    assert not fails, fails
    assert cuts > 0


def test_ola_normalize_zero_weights(kt):
    """exact zeros (and a weight below 1e-8) divide by 1e-8f; 3 rows of 300 (two blocks), a sentinel row behind"""
    rows, n = 3, 300
    rng = np.random.default_rng(5)
    x = rng.standard_normal((rows, n)).astype(np.float32) * np.float32(1e-6)
    w = rng.uniform(0.0, 2.0, n).astype(np.float32)
    w[[0, 7, 255, 256, 299]] = 0.0
    w[100] = np.float32(1e-9)
    bx = kt.Buf(np.concatenate([x.ravel(), _sent(kt, n)]), "f32", 1024, output=True)
    bw = kt.Buf(w, "f32", 1024)
    assert _lib().athd_ola_normalize(bx.ptr, bw.ptr, rows, n, _stream()) == 0
    kt.sync()
    raw, bands = bx.host()
    assert bands and (raw[rows * n:] == np.float32(kt.F32_SENTINEL)).all()
    want = x / np.maximum(w, tr.EPS32)[None, :]
    assert (want[:, 0] == x[:, 0] / tr.EPS32).all() and np.isfinite(want).all()
    assert _bits(raw[:rows * n].reshape(rows, n), want)
    _rec(kt, "ola_normalize[zero weights]", bit_equal=True)


def test_overlap_add_refusals_write_nothing(kt):
    lib = _lib()
    c, o, L, S = 8, 3, 24, 1                      # 5 windows
    n = len(tr.plan(L, c, o))
    wbuf = kt.Buf(tr.ola_windows(c, o, L, S), "f32", 4096)
    # (L, chunk, overlap, n_stems, k0, k1)
    bad = {"overlap == chunk": (L, c, c, S, 0, 1), "overlap < 0": (L, c, -1, S, 0, n), "k0 == k1": (L, c, o, S, 2, 2),
           "k1 > n": (L, c, o, S, 0, n + 1), "L == 0": (0, c, o, S, 0, 1), "n_stems == 0": (L, c, o, 0, 0, n),
           "2 n_stems > 65535": (L, c, o, 32768, 0, n)}
    for name, (l, ch, ov, s, k0, k1) in bad.items():
        for mode in (0, 1, 2):                    # additive, weighted, weighted with a weight row
            bo, bw = _out(kt, 4096), _out(kt, 4096)
            if mode == 0:
                rc = lib.athd_overlap_add(wbuf.ptr, l, ch, ov, s, k0, k1, bo.ptr, _stream())
            else:
                rc = lib.athd_overlap_add_weighted(wbuf.ptr, l, ch, ov, s, k0, k1, bo.ptr, bw.ptr if mode == 2 else None,
                                                   _stream())
            kt.sync()
            assert rc == EINVAL, (name, mode, rc)
            assert _untouched(kt, bo) and _untouched(kt, bw), (name, mode)
    bo, bw = _out(kt, 4096), kt.Buf(np.ones(8, dtype=np.float32), "f32", 64)
    for rows, cols in ((65536, 1), (0, 8), (2, 0)):
        assert lib.athd_ola_normalize(bo.ptr, bw.ptr, rows, cols, _stream()) == EINVAL, (rows, cols)
    kt.sync()
    assert _untouched(kt, bo)
    _rec(kt, "ola refusals", cases=3 * len(bad) + 3)


# ========================================================================================================= SDR / SI-SDR
def _metric(kt, fn, per_row, est, tgt):
    rows, n = est.shape
    be, bt = kt.Buf(est, "f32", 4096), kt.Buf(tgt, "f32", 4096)
    bs = kt.Buf(np.full(per_row * rows, kt.F32_SENTINEL), "f64", 64, output=True)
    bo = _out(kt, 1, guard=64)
    assert fn(be.ptr, bt.ptr, rows, n, bs.ptr, bo.ptr, _stream()) == 0
    kt.sync()
    raw, bands = bo.host()
    assert bands, "band around out overwritten"
    assert bs.host()[1], "scratch written past its documented size"
    return float(raw[0])


@pytest.mark.parametrize("family", tr.FAMILIES + ["mixed"])
def test_sdr_sisdr(kt, family):
    lib = _lib()
    fails, worst = [], {"sdr": 0.0, "sisdr": 0.0}
    shapes = {}
    for rows, n in tr.metric_shapes(family):
        est, tgt = tr.metric_case(family, rows, n)
        for name, fn, per_row, ref_rows in (("sdr", lib.athd_sdr, 2, tr.sdr_rows64), ("sisdr", lib.athd_sisdr, 5, tr.sisdr_rows64)):
            rr = ref_rows(est, tgt)
            ref = float(rr.mean())
            got = _metric(kt, fn, per_row, est, tgt)
            err = abs(got - ref) if np.isfinite(got) else np.inf
            exact = None
            if (rr == 30.0).all() or (rr == -30.0).all():
                exact = got == float(rr[0])
            elif family == "silence":
                exact = got == 0.0
            worst[name] = max(worst[name], err)
            shapes["%s[%d,%d]" % (name, rows, n)] = err
            print("%s %s[%d,%d]: got %.9g ref %.12g err %.3g exact %s" % (family, name, rows, n, got, ref, err, exact))
            if err > tr.TOL_DB or exact is False:
                fails.append((name, rows, n, got, ref, exact))
    _rec(kt, "metrics[%s]" % family, worst_err_db=worst, err_db=shapes, tol_db=tr.TOL_DB)
    assert not fails, fails


def test_metric_refusals_write_nothing(kt):
    """rows = 65536 (rows is the grid's y dimension), n = 0, rows = 0: ATHD_EINVAL, `out` and the scratch untouched.
    The scratch is large enough for 65536 rows, so nothing could be written out of bounds either way."""
    lib = _lib()
    be, bt = kt.Buf(np.ones(65536, dtype=np.float32), "f32", 4096), kt.Buf(np.ones(65536, dtype=np.float32), "f32", 4096)
    for name, fn in (("sdr", lib.athd_sdr), ("sisdr", lib.athd_sisdr)):
        for rows, n in ((65536, 1), (8, 0), (0, 8)):
            bs = kt.Buf(np.full(5 * 65536, kt.F32_SENTINEL), "f64", 64, output=True)
            bo = _out(kt, 1, guard=64)
            rc = fn(be.ptr, bt.ptr, rows, n, bs.ptr, bo.ptr, _stream())
            kt.sync()
            assert rc == EINVAL, (name, rows, n, rc)
            raw, bands = bs.host()
            assert bands and (raw == kt.F32_SENTINEL).all(), (name, rows, n, "scratch written")
            assert _untouched(kt, bo), (name, rows, n, "out written")
    _rec(kt, "metric refusals", cases=6)
