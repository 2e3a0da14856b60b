"""CPU self-test of tests/track_refs.py: the case list, the float64 references and bounds against torch's own float32
loops (the oracle restatement of test_inference.py:92-141 and benchmark.py:155-204 in oracle/athtdemucs_ref.py), the
float32 restatements against the same bounds and against torch.linspace, and the conditioning of the metric references.

Measured here (worst err / bound over all cases, torch's loops and the restatements alike): mode 0 0.14, mode 1 acc 0.38,
ws 0.33, normalised 0.24; the metric references move by at most 7e-15 dB between pairwise and exactly rounded sums."""
import numpy as np
import pytest
import torch

import track_refs as tr
from oracle.athtdemucs_ref import benchmark_chunked_inference, chunk_plan, linear_fade

CASES = tr.cases()
CASES0 = [c for c in CASES if tr.in_domain0(c[2], c[0], c[1])]
BY_PAIR = {p: [c for c in CASES if c[:2] == p] for p in tr.PAIRS}
S = 2


def _ratio(got, ref, bound):
    r = np.abs(np.asarray(got, dtype=np.float64) - ref) / np.maximum(bound, 1e-300)
    r[(bound == 0) & (np.asarray(got, dtype=np.float64) == ref)] = 0.0
    return float(r.max())


def test_case_counts():
    assert len(CASES) == 130 and len(set(CASES)) == 130
    assert len(CASES0) >= 70, len(CASES0)
    # what the list is there for: the n == 1 ramps and the two-point ramp, odd and 1-sample tails of fade_len = len // 2,
    # hop < overlap with tens of windows on one sample, several blocks of 256 output samples
    assert {o for _, o, _ in CASES} >= {0, 1, 2}
    tails = {(min(o, (e - s) // 2), (e - s) % 2) for c, o, L in CASES for s, e in tr.plan(L, c, o)[-1:] if e - s < 2 * o}
    assert any(fl == 0 for fl, _ in tails) and any(fl == 1 for fl, _ in tails) and any(odd for _, odd in tails)
    assert max(tr.ola1_ref(tr.ola_windows(257, 255, 1288, 1), 1288, 257, 255).m) >= 128
    assert max(L for _, _, L in CASES) > 4 * 256


def test_plan_matches_oracle_plan():
    for c, o, L in CASES:
        p = chunk_plan(L, 1, c, o)
        assert [(s, e) for s, e, _, _ in p] == tr.plan(L, c, o)
        assert [(fi, fo) for _, _, fi, fo in p] == tr.fades0(L, c, o)


def test_reference_domain_is_the_oracles():
    """linear_fade (torchaudio's Fade restated) fails exactly outside in_domain0"""
    for c, o, L in CASES:
        ok = True
        try:
            for s, e, fi, fo in chunk_plan(L, 1, c, o):
                linear_fade(torch.zeros(1, e - s), fi, fo)
        except RuntimeError:
            ok = False
        assert ok == tr.in_domain0(L, c, o), (c, o, L)


def _torch_mode0(win, L, c, o):
    final = torch.zeros((win.shape[1], 2, L), dtype=torch.float32)
    for k, (s, e, fi, fo) in enumerate(chunk_plan(L, 1, c, o)):
        final[:, :, s:e] += linear_fade(torch.from_numpy(win[k, :, :, :e - s]), fi, fo)
    return final.numpy()


def _torch_mode1(win, L, c, o):
    """benchmark_chunked_inference with the window outputs as the 'model', and the chunk_weight loop restated for the
    weight sum (the oracle returns only output / weight)"""
    it = iter(range(win.shape[0]))
    q = benchmark_chunked_inference(lambda chunk: torch.from_numpy(win[next(it)].reshape(1, -1, c)),
                                    torch.zeros(2 * win.shape[1], L), 1, c, o)
    output, weight = torch.zeros(2 * win.shape[1], L), torch.zeros(L)
    for k, (s, e) in enumerate(tr.plan(L, c, o)):
        n = e - s
        fl = min(o, n // 2)
        cw = torch.ones(n)
        if s > 0 and fl > 0:
            cw[:fl] = torch.linspace(0, 1, fl)
        if e < L and fl > 0:
            cw[-fl:] = torch.linspace(1, 0, fl)
        output[:, s:e] += torch.from_numpy(win[k].reshape(-1, c)[:, :n]) * cw
        weight[s:e] += cw
    assert torch.equal(output / weight.clamp(min=1e-8), q)
    shape = (win.shape[1], 2, L)
    return output.numpy().reshape(shape), weight.numpy(), q.numpy().reshape(shape)


@pytest.mark.parametrize("pair", tr.PAIRS, ids=lambda p: "%d-%d" % p)
def test_bounds_hold_for_torch_and_restatement(pair):
    worst = {}

    def upd(k, v):
        worst[k] = max(worst.get(k, 0.0), v)

    for c, o, L in BY_PAIR[pair]:
        win = tr.ola_windows(c, o, L, S)
        r1 = tr.ola1_ref(win, L, c, o)
        assert r1.m.min() >= 1 and (r1.ws > 0).all()
        for name, (acc, ws, q) in (("torch", _torch_mode1(win, L, c, o)), ("f32", tr.ola1_f32(win, L, c, o))):
            upd(name + "1_acc", _ratio(acc, r1.acc, r1.b_acc))
            upd(name + "1_ws", _ratio(ws, r1.ws, r1.b_ws))
            upd(name + "1_q", _ratio(q, r1.q, r1.b_q))
        if tr.in_domain0(L, c, o):
            r0 = tr.ola0_ref(win, L, c, o)
            upd("torch0", _ratio(_torch_mode0(win, L, c, o), r0.out, r0.bound))
            upd("f320", _ratio(tr.ola0_f32(win, L, c, o), r0.out, r0.bound))
        else:
            with pytest.raises(AssertionError):
                tr.ola0_ref(win, L, c, o)
    print(pair, {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


def test_window_ranges_sum_to_the_one_range_reference():
    """float64: the spans of [0, a) and [a, n) add up to the one-range sums, m and A included; float32: bit-equal on
    rank_mask, which is everything when overlap <= hop (every plan the product runs)"""
    for c, o, L in CASES:
        n = len(tr.plan(L, c, o))
        if not 2 <= n <= 12:
            continue
        win = tr.ola_windows(c, o, L, 1)
        full, (facc, fws, _) = tr.ola1_ref(win, L, c, o), tr.ola1_f32(win, L, c, o)
        for a in range(1, n):
            t1 = tr.span_of(L, c, o, a, n)[0]
            lo, hi = tr.ola1_ref(win, L, c, o, 0, a), tr.ola1_ref(win, L, c, o, a, n)
            acc, m = np.zeros_like(full.acc), np.zeros_like(full.m)
            acc[..., :lo.acc.shape[-1]] += lo.acc
            acc[..., t1:] += hi.acc
            m[:lo.m.size] += lo.m
            m[t1:] += hi.m
            assert np.allclose(acc, full.acc, rtol=1e-13, atol=1e-13) and (m == full.m).all()
            a32, w32 = np.zeros_like(facc), np.zeros_like(fws)
            l32, h32 = tr.ola1_f32(win, L, c, o, 0, a), tr.ola1_f32(win, L, c, o, a, n)
            a32[..., :l32[0].shape[-1]] += l32[0]
            a32[..., t1:] += h32[0]
            w32[:l32[1].size] += l32[1]
            w32[t1:] += h32[1]
            mask = tr.rank_mask(L, c, o, a)
            assert mask.all() or o > c - o
            assert (a32.view(np.uint32)[..., mask] == facc.view(np.uint32)[..., mask]).all()
            assert (w32.view(np.uint32)[mask] == fws.view(np.uint32)[mask]).all()


def test_checks_would_notice_a_shifted_ramp_and_an_fma():
    """on the (300, 37) plan: a fade-in ramp that starts one sample late is far outside the per-sample bound, and
    acc = fma(w, x, acc) (the product not rounded; exact in float64, since two float32 factors have 48 significant
    bits) stays inside the bound and inside a global 1e-6 max|x| but changes bit patterns, which the GPU test compares"""
    c, o, L = 300, 37, 2 * 263 + 37 + 1
    win = tr.ola_windows(c, o, L, 1)
    r1, (acc32, _, _) = tr.ola1_ref(win, L, c, o), tr.ola1_f32(win, L, c, o)
    p = tr.plan(L, c, o)
    shifted = np.zeros_like(r1.acc)
    fma = np.zeros(r1.acc.shape, dtype=np.float32)
    for k, (s, e) in enumerate(p):
        w = tr.weight1_f32(e - s, o, s == 0, e == L)
        fma[:, :, s:e] = (w.astype(np.float64) * win[k, :, :, :e - s] + fma[:, :, s:e]).astype(np.float32)
        if s > 0:
            w = np.concatenate([w[:1], w[:-1]])
        shifted[:, :, s:e] += w.astype(np.float64) * win[k, :, :, :e - s]
    assert _ratio(shifted, r1.acc, r1.b_acc) > 1000.0
    assert _ratio(fma, r1.acc, r1.b_acc) <= 1.0 and np.abs(fma - acc32).max() <= 1e-6 * np.abs(win).max()
    assert (fma.view(np.uint32) != acc32.view(np.uint32)).sum() > 10


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_ramps_match_torch_linspace_to_one_ulp():
    exact = True
    for n in list(range(1, 700)) + [4410, 66150]:
        up, dn = torch.linspace(0, 1, n).numpy(), torch.linspace(1, 0, n).numpy()
        a, b = tr.lin01_f32(n), tr.lin10_f32(n)
        assert _ulps(a, up).max() <= 1 and _ulps(b, dn).max() <= 1, n
        exact = exact and (a == up).all() and (b == dn).all()
        assert np.abs(a - tr.up64(n)).max() <= 3 * tr.U and np.abs(b - tr.down64(n)).max() <= 3 * tr.U, n
    assert tr.lin01_f32(1)[0] == 0.0 and tr.lin10_f32(1)[0] == 1.0
    assert (tr.lin01_f32(2) == [0.0, 1.0]).all() and (tr.lin10_f32(2) == [1.0, 0.0]).all()
    print("restated ramps bit-equal to torch.linspace at every n:", exact)


@pytest.mark.parametrize("family", tr.FAMILIES + ["mixed"])
def test_metric_references_are_well_conditioned(family):
    """numpy's pairwise sums against exactly rounded sums: 1e-9 dB, far inside the GPU tolerance"""
    worst = 0.0
    for rows, n in tr.metric_shapes(family):
        est, tgt = tr.metric_case(family, rows, n)
        assert est.shape == tgt.shape == (rows, n) and est.dtype == np.float32
        for f64, fsum in ((tr.sdr_rows64, tr.sdr_rows_fsum), (tr.sisdr_rows64, tr.sisdr_rows_fsum)):
            a, b = f64(est, tgt), fsum(est, tgt)
            worst = max(worst, float(np.abs(a - b).max()), abs(float(a.mean()) - tr.mean_fsum(b)))
    print(family, "worst |pairwise - fsum| dB:", worst)
    assert worst <= 1e-9


def test_metric_families_do_what_they_are_named_for():
    n = 1000
    one = {f: tr.metric_case(f, 1, n) for f in tr.FAMILIES}
    sdr = {f: float(tr.sdr_rows64(*one[f])[0]) for f in tr.FAMILIES}
    si = {f: float(tr.sisdr_rows64(*one[f])[0]) for f in tr.FAMILIES}
    assert sdr["clamp_hi"] == 30.0 and si["clamp_hi"] == 30.0
    assert sdr["clamp_lo40"] == -30.0 and sdr["tgt_zero"] == -30.0 and si["tgt_zero"] == -30.0
    assert abs(sdr["clamp_lo"] - 10 * np.log10(1 / 961)) < 1e-6 and si["clamp_lo"] == 30.0
    assert abs(sdr["edge"] - 29.9) < 1e-3 and abs(sdr["edge_lo"] + 29.9) < 1e-3
    assert sdr["silence"] == 0.0 and si["silence"] == 0.0
    assert sdr["gain"] == 0.0 and si["gain"] == 30.0
    assert sdr["dc"] == 30.0 and 5.0 < si["dc"] < 15.0            # the offset dominates SDR; SI-SDR removes it
    # tiny: the sums are comparable to 1e-8, so dropping the 1e-8 terms moves the value by far more than TOL_DB
    e64, t64 = (v[0].astype(np.float64) for v in one["tiny"])
    num, den = float(np.sum(t64 ** 2)), float(np.sum((t64 - e64) ** 2))
    assert 1e-9 < num < 1e-6 and abs(10 * np.log10(num / den) - sdr["tiny"]) > 1000 * tr.TOL_DB
    assert 5.0 < sdr["gauss"] < 15.0
    est, tgt = tr.metric_case("mixed", len(tr.FAMILIES), n)
    rows = tr.sdr_rows64(est, tgt)
    assert (np.abs(rows) == 30.0).any() and (np.abs(rows) < 30.0).any()
