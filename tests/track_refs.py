"""float64 references, derived bounds and float32 restatements for the track-level kernels of csrc/track.hip
(tests/test_gpu_track_kernels.py reaches them through the product ABI: athd_overlap_add, athd_overlap_add_weighted,
athd_ola_normalize, athd_sdr, athd_sisdr).  numpy only, no GPU; tests/test_track_refs.py checks this file on the CPU.

Window plan (both protocols): start_k = k hop, hop = chunk - overlap, while start < L; end_k = min(start_k + chunk, L).

Ramps are exact here: up(n)[i] = i / (n - 1) (0 for n == 1), down(n)[i] = (n - 1 - i) / (n - 1) (1 for n == 1), the
values torch.linspace(0, 1, n) / torch.linspace(1, 0, n) approximate.

Mode 0 (test_inference.py:92-141): window k is multiplied by fi fo, fi = up(fade_in_k) over its first fade_in_k samples
(fade_in_k = overlap for k > 0), fo = 1 - up(fade_out_k) over its last fade_out_k samples (fade_out_k = overlap while
end_k < L), 1 elsewhere, and the windows are summed in ascending k.  The reference (torchaudio's Fade) exists only where
every window is at least as long as each of its fades (`in_domain0`); ola0_ref refuses any other plan.

Mode 1 (benchmark.py:155-204): fade_len_k = min(overlap, len_k // 2); w_k = 1 with up(fade_len_k) over the first
fade_len_k samples if start_k > 0 and down(fade_len_k) over the last if end_k < L; acc = sum w x, ws = sum w,
q = acc / max(ws, 1e-8).  Defined for every plan.

Each reference also returns, per output sample, m = the number of windows of [k0, k1) that cover it and
A = sum |x_k| over those windows.

Bounds, u = 2^-24 (one float32 rounding, relative; every quantity rounded below is at most |x| or a partial sum of
magnitudes, so each rounding costs at most u |x| resp. u A):
* A ramp value takes 3 roundings: step = 1 / (n - 1), step i, and (second half) 1 - step i'.  Values are at most 1, so
  the ramp is known to 3u absolutely.
* Mode 0: fo = 1 - ramp takes one more (4u), fi fo one (3 + 4 + 1 = 8u), (fi fo) x one (9u |x|), and the sum of m terms
  m - 1 additions of partial sums no larger than A:          |out - out64| <= (9 + m) u A.
* Mode 1, acc: w to 3u, x w one more (4u |x|), m - 1 additions:  |acc - acc64| <= (m + 3) u A.
* Mode 1, ws: m weights to 3u each, m - 1 additions of partial sums no larger than ws64 (w >= 0):
                                                             |ws - ws64| <= (3 m + (m - 1) ws64) u.
  (The second term matters: chunk 257 with overlap 255 stacks 129 windows on one sample.)
* Mode 1, q = fl(acc / max(ws, 1e-8)): with d_acc, d_ws the two bounds above,
      |q - q64| <= (d_acc + |q64| d_ws) / max(ws64 - d_ws, 1e-8) + u |q64|.
Any order of the m - 1 additions meets the same bounds, so a track recombined from the spans of window ranges does too.

float32 restatements (ola0_f32, ola1_f32): the arithmetic csrc/track.hip documents, with np.float32 arrays.  numpy rounds
every operation to float32 and never contracts a product into an fma, so the result is the bit pattern the kernels
promise: linspace01 / linspace10 with their two halves (ATen's range formula), the [0, 1] clamps, w = fi fo,
acc = acc + w x in ascending k from 0.0f, acc / max(ws, 1e-8f).  For mode 0 outside the reference's domain the
restatement follows the kernel's own indexing (window sample j reads fade-in index j and fade-out index
j - (len - fade_out)), so the bit comparison covers every plan while the float64 bound covers the domain.

SDR / SI-SDR (src/loss.py:9-68, sign flipped): float64, literally as the reference reads, per row, clamp to +-30 dB,
mean over rows.  `*_fsum` recompute the same with math.fsum (exactly rounded sums) instead of numpy's pairwise sums.
"""
import math
import zlib
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
F1 = np.float32(1.0)
EPS32 = np.float32(1e-8)

# ---------------------------------------------------------------------------------------------------- overlap-add cases
PAIRS = [(8, 0), (8, 1), (8, 2), (8, 3), (9, 4), (10, 5), (10, 7), (10, 9), (300, 37), (257, 255), (1000, 513)]


def lengths(chunk, ov):
    hop = chunk - ov
    ls = [1, 2, 3, chunk - 1, chunk, chunk + 1, hop + ov, 2 * hop + ov, 2 * hop + ov + 1, 3 * hop + chunk - 1,
          3 * hop + chunk, 7 * hop + max(ov, 1), 5 * chunk + 3]
    return sorted(set(ls))


def cases():
    """[(chunk, overlap, L)]: 130 cases"""
    return [(c, o, L) for c, o in PAIRS for L in lengths(c, o)]


def plan(L, chunk, overlap):
    out, start = [], 0
    while start < L:
        out.append((start, min(start + chunk, L)))
        start += chunk - overlap
    return out


def fades0(L, chunk, overlap):
    """[(fade_in, fade_out)] per window of mode 0"""
    return [(0 if s == 0 else overlap, overlap if e < L else 0) for s, e in plan(L, chunk, overlap)]


def in_domain0(L, chunk, overlap):
    return all(e - s >= max(f) for (s, e), f in zip(plan(L, chunk, overlap), fades0(L, chunk, overlap)))


def span_of(L, chunk, overlap, k0, k1):
    """(t0, span) of windows [k0, k1)"""
    p = plan(L, chunk, overlap)
    return p[k0][0], p[k1 - 1][1] - p[k0][0]


def ola_windows(chunk, overlap, L, S, poison=False):
    """window outputs [n][S][2][chunk] float32: independent N(0, 1) per (window, stem, channel), the rows of stem s and
    channel c scaled by 2^(2 s + c); poison: NaN at j >= len_k"""
    p = plan(L, chunk, overlap)
    rng = np.random.default_rng(zlib.crc32(repr(("ola", chunk, overlap, L, S)).encode()))
    win = rng.standard_normal((len(p), S, 2, chunk)).astype(np.float32)
    win *= (2.0 ** (2 * np.arange(S)[:, None] + np.arange(2)[None, :])).astype(np.float32)[None, :, :, None]
    if poison:
        for k, (s, e) in enumerate(p):
            win[k, :, :, e - s:] = np.nan
    return win


# ------------------------------------------------------------------------------------------------- float64 references
def up64(n):
    return np.zeros(n) if n <= 1 else np.arange(n, dtype=np.float64) / (n - 1)


def down64(n):
    return np.ones(n) if n <= 1 else np.arange(n - 1, -1, -1, dtype=np.float64) / (n - 1)


def weight0_64(ln, fin, fout):
    assert ln >= fin and ln >= fout, "outside the reference's domain (Fade needs len >= fade)"
    fi, fo = np.ones(ln), np.ones(ln)
    fi[:fin] = up64(fin)
    fo[ln - fout:] = 1.0 - up64(fout)
    return fi * fo


def weight1_64(ln, ov, first, last):
    fl = min(ov, ln // 2)
    w = np.ones(ln)
    if not first and fl > 0:
        w[:fl] = up64(fl)
    if not last and fl > 0:
        w[ln - fl:] = down64(fl)
    return w


def _gather64(win, L, chunk, overlap, k0, k1, weight):
    p = plan(L, chunk, overlap)
    k1 = len(p) if k1 is None else k1
    t0, span = span_of(L, chunk, overlap, k0, k1)
    S = win.shape[1]
    acc, A = np.zeros((S, 2, span)), np.zeros((S, 2, span))
    ws, m = np.zeros(span), np.zeros(span, dtype=np.int64)
    for k in range(k0, k1):
        s, e = p[k]
        w = weight(k, s, e)
        x = win[k, :, :, :e - s].astype(np.float64)
        acc[:, :, s - t0:e - t0] += w * x
        A[:, :, s - t0:e - t0] += np.abs(x)
        ws[s - t0:e - t0] += w
        m[s - t0:e - t0] += 1
    return acc, ws, m, A


def ola0_ref(win, L, chunk, overlap, k0=0, k1=None):
    """win: all n windows [n][S][2][chunk]; -> out [S][2][span] float64, m [span], A, bound"""
    fd = fades0(L, chunk, overlap)
    out, _, m, A = _gather64(win, L, chunk, overlap, k0, k1, lambda k, s, e: weight0_64(e - s, *fd[k]))
    return SimpleNamespace(out=out, m=m, A=A, bound=(9 + m) * U * A)


def ola1_ref(win, L, chunk, overlap, k0=0, k1=None):
    acc, ws, m, A = _gather64(win, L, chunk, overlap, k0, k1,
                              lambda k, s, e: weight1_64(e - s, overlap, s == 0, e == L))
    q = acc / np.maximum(ws, 1e-8)
    b_acc = (m + 3) * U * A
    b_ws = (3 * m + (m - 1) * ws) * U
    b_q = (b_acc + np.abs(q) * b_ws) / np.maximum(ws - b_ws, 1e-8) + U * np.abs(q)
    return SimpleNamespace(acc=acc, ws=ws, q=q, m=m, A=A, b_acc=b_acc, b_ws=b_ws, b_q=b_q)


# ------------------------------------------------------------------------------------------------ float32 restatements
def lin01_f32(n):
    """track.hip linspace01(i, n), i = 0 .. n-1"""
    if n <= 1:
        return np.zeros(n, dtype=np.float32)
    i = np.arange(n)
    step = F1 / np.float32(n - 1)
    lo = step * i.astype(np.float32)
    hi = F1 - step * (n - i - 1).astype(np.float32)
    return np.where(i < n // 2, lo, hi).astype(np.float32)


def lin10_f32(n):
    """track.hip linspace10(i, n)"""
    if n <= 1:
        return np.ones(n, dtype=np.float32)
    i = np.arange(n)
    step = -(F1 / np.float32(n - 1))
    lo = F1 + step * i.astype(np.float32)
    hi = -step * (n - i - 1).astype(np.float32)
    return np.where(i < n // 2, lo, hi).astype(np.float32)


def weight0_f32(ln, fin, fout):
    j = np.arange(ln)
    fi = np.ones(ln, dtype=np.float32)
    if fin > 0:
        fi = np.where(j < fin, lin01_f32(fin)[np.minimum(j, fin - 1)], F1)
    fo = np.ones(ln, dtype=np.float32)
    if fout > 0:
        idx = j - (ln - fout)
        fo = np.where(idx >= 0, F1 - lin01_f32(fout)[np.maximum(idx, 0)], F1)
    fi = np.minimum(np.maximum(fi.astype(np.float32), np.float32(0)), F1)
    fo = np.minimum(np.maximum(fo.astype(np.float32), np.float32(0)), F1)
    return fi * fo


def weight1_f32(ln, ov, first, last):
    fl = min(ov, ln // 2)
    w = np.ones(ln, dtype=np.float32)
    if not first and fl > 0:
        w[:fl] = lin01_f32(fl)
    if not last and fl > 0:
        w[ln - fl:] = lin10_f32(fl)
    return w


def _gather32(win, L, chunk, overlap, k0, k1, weight):
    p = plan(L, chunk, overlap)
    k1 = len(p) if k1 is None else k1
    t0, span = span_of(L, chunk, overlap, k0, k1)
    acc = np.zeros((win.shape[1], 2, span), dtype=np.float32)
    ws = np.zeros(span, dtype=np.float32)
    for k in range(k0, k1):
        s, e = p[k]
        w = weight(k, s, e)
        assert w.dtype == np.float32
        x = win[k, :, :, :e - s]
        acc[:, :, s - t0:e - t0] = acc[:, :, s - t0:e - t0] + w * x
        ws[s - t0:e - t0] = ws[s - t0:e - t0] + w
    return acc, ws


def ola0_f32(win, L, chunk, overlap, k0=0, k1=None):
    fd = fades0(L, chunk, overlap)
    return _gather32(win, L, chunk, overlap, k0, k1, lambda k, s, e: weight0_f32(e - s, *fd[k]))[0]


def ola1_f32(win, L, chunk, overlap, k0=0, k1=None):
    """-> (acc, ws, q) float32"""
    acc, ws = _gather32(win, L, chunk, overlap, k0, k1, lambda k, s, e: weight1_f32(e - s, overlap, s == 0, e == L))
    return acc, ws, acc / np.maximum(ws, EPS32)


def rank_mask(L, chunk, overlap, a):
    """samples at which the sum of the spans of windows [0, a) and [a, n) in rank order performs the one-range
    additions: no window of the first range covers the sample (0.0f + x = x) or at most one of the second does
    (then the last addition is the one-range one).  Elsewhere the second range's terms are added among themselves
    first and float addition does not re-associate."""
    p = plan(L, chunk, overlap)
    m0, m1 = np.zeros(L, dtype=np.int64), np.zeros(L, dtype=np.int64)
    for k, (s, e) in enumerate(p):
        (m0 if k < a else m1)[s:e] += 1
    return (m0 == 0) | (m1 <= 1)


# ------------------------------------------------------------------------------------------------------ SDR / SI-SDR
FAMILIES = ["gauss", "clamp_hi", "clamp_lo", "clamp_lo40", "edge", "edge_lo", "tiny", "silence", "tgt_zero", "dc", "gain"]
METRIC_N = [1, 63, 64, 65, 255, 256, 257, 1000, 262144 + 257]
METRIC_SHAPES = [(r, n) for r in (1, 3) for n in METRIC_N] + [(65535, 2)]
TOL_DB = 4e-6          # 2 x (2^-24 x 32): the float32 rounding of a mean of magnitude <= 30, doubled


def metric_shapes(family):
    """'mixed' holds one row of each family, so its row count is fixed; it also runs as the many-rows case"""
    if family == "mixed":
        return [(len(FAMILIES), n) for n in METRIC_N] + [(65535, 2)]
    return METRIC_SHAPES


def _edge_sigma(t, nz, db):
    """sigma with 10 log10((|t|^2 + 1e-8) / (sigma^2 |nz|^2 + 1e-8)) = db"""
    den = (float(np.sum(t * t)) + 1e-8) / 10.0 ** (db / 10.0) - 1e-8
    return math.sqrt(max(den, 0.0) / max(float(np.sum(nz * nz)), 1e-300))


def metric_row(family, n, rng):
    """one (est, tgt) row pair, float32"""
    g = rng.standard_normal(n).astype(np.float32).astype(np.float64)
    nz = rng.standard_normal(n)
    if family == "gauss":
        est, tgt = g + 0.3 * nz, g
    elif family == "clamp_hi":
        est, tgt = g, g
    elif family == "clamp_lo":          # SDR 10 log10(1 / 961) = -29.83 dB (inside the clamp); SI-SDR +30
        est, tgt = -30.0 * g, g
    elif family == "clamp_lo40":        # SDR 10 log10(1 / 1681) = -32.3 dB: clamped at -30
        est, tgt = -40.0 * g, g
    elif family == "edge":
        est, tgt = g + _edge_sigma(g, nz, 29.9) * nz, g
    elif family == "edge_lo":
        est, tgt = g + _edge_sigma(g, nz, -29.9) * nz, g
    elif family == "tiny":
        est, tgt = 1e-5 * g + 1e-5 * nz, 1e-5 * g
    elif family == "silence":
        est, tgt = np.zeros(n), np.zeros(n)
    elif family == "tgt_zero":
        est, tgt = g, np.zeros(n)
    elif family == "dc":
        est, tgt = 100.0 + 0.01 * (g + 0.3 * nz), 100.0 + 0.01 * g
    elif family == "gain":
        est, tgt = 2.0 * g, g
    else:
        raise KeyError(family)
    return est.astype(np.float32), tgt.astype(np.float32)


def metric_case(family, rows, n):
    """(est, tgt) float32 [rows][n]; 'mixed': row r is of family FAMILIES[r % len(FAMILIES)]"""
    rng = np.random.default_rng(zlib.crc32(repr(("metric", family, rows, n)).encode()))
    fam = [FAMILIES[r % len(FAMILIES)] if family == "mixed" else family for r in range(rows)]
    if rows > 1000:                      # many short rows: draw each family's rows in one call
        est, tgt = np.zeros((rows, n), dtype=np.float32), np.zeros((rows, n), dtype=np.float32)
        for f in sorted(set(fam)):
            idx = [r for r in range(rows) if fam[r] == f]
            pairs = [metric_row(f, n, rng) for _ in idx]
            est[idx], tgt[idx] = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        return est, tgt
    pairs = [metric_row(f, n, rng) for f in fam]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def _db(num, den):
    return np.clip(10.0 * np.log10((num + 1e-8) / (den + 1e-8)), -30.0, 30.0)


def sdr_rows64(est, tgt):
    """src/loss.py:9-30 per row (sign flipped), float64"""
    e, t = est.astype(np.float64), tgt.astype(np.float64)
    return _db(np.sum(t ** 2, axis=-1), np.sum((t - e) ** 2, axis=-1))


def sisdr_rows64(est, tgt):
    """src/loss.py:33-68 per row (sign flipped), float64"""
    e, t = est.astype(np.float64), tgt.astype(np.float64)
    e = e - e.mean(axis=-1, keepdims=True)
    t = t - t.mean(axis=-1, keepdims=True)
    dot = np.sum(e * t, axis=-1, keepdims=True)
    tt = np.sum(t ** 2, axis=-1, keepdims=True)
    s_target = (dot / (tt + 1e-8)) * t
    e_noise = e - s_target
    return _db(np.sum(s_target ** 2, axis=-1), np.sum(e_noise ** 2, axis=-1))


def _fs(a):
    return math.fsum(a.tolist())


def sdr_rows_fsum(est, tgt):
    e, t = est.astype(np.float64), tgt.astype(np.float64)
    return np.array([_db(_fs(t[r] ** 2), _fs((t[r] - e[r]) ** 2)) for r in range(e.shape[0])])


def sisdr_rows_fsum(est, tgt):
    e, t = est.astype(np.float64), tgt.astype(np.float64)
    out = []
    for r in range(e.shape[0]):
        n = e.shape[1]
        ec, tc = e[r] - _fs(e[r]) / n, t[r] - _fs(t[r]) / n
        a = _fs(ec * tc) / (_fs(tc ** 2) + 1e-8)
        st = a * tc
        out.append(_db(_fs(st ** 2), _fs((ec - st) ** 2)))
    return np.array(out)


def mean_fsum(v):
    return math.fsum(v.tolist()) / len(v)
