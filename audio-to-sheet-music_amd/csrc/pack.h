// Private: the host side of the weight contract, pure functions from the reference's fp32 tensors to the row-major
// matrices the kernels read.  ctx.h uploads what they return, pack.cpp calls them per stage, ktest.cpp exports them.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

namespace athd {

inline uint16_t host_f2bf(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// Moments of a 1x1 conv W [N][H] (row-major), b [N] for GroupNorm statistics from its input alone:
// [G = W^T W (H x H) | v = W^T b (H) | ws = W^T 1 (H) | sum b | sum b^2], accumulated in fp64; round_bf16: from the
// bf16-rounded weights the MFMA kernels multiply with
inline std::vector<float> conv1x1_moments(const std::vector<float>& w, const std::vector<float>& b, int N, int H,
                                          bool round_bf16) {
    std::vector<double> g((size_t)H * H + 2 * H + 2, 0.0);
    auto wv = [&](int n, int j) -> double {
        const float x = w[(size_t)n * H + j];
        if (!round_bf16) return x;
        const uint32_t u = (uint32_t)host_f2bf(x) << 16;
        float r;
        std::memcpy(&r, &u, 4);
        return r;
    };
    for (int n = 0; n < N; ++n) {
        const double bn = b[n];
        for (int j = 0; j < H; ++j) {
            const double wj = wv(n, j);
            for (int k = 0; k < H; ++k) g[(size_t)j * H + k] += wj * wv(n, k);
            g[(size_t)H * H + j] += bn * wj;
            g[(size_t)H * H + H + j] += wj;
        }
        g[(size_t)H * H + 2 * H] += bn;
        g[(size_t)H * H + 2 * H + 1] += bn * bn;
    }
    return std::vector<float>(g.begin(), g.end());
}
// K order of the rewrite weights that the fused DConv apply multiplies (dconv.hip dconv_apply_kernel<C, NW, true>,
// C = 48, 96): K slot 32 ks + 8 g + i holds channel 32 ks + 4 g + i (i < 4) or 32 ks + 16 + 4 g + (i - 4), the order in
// which a lane holds its row's updated channels.  Slots whose channel is >= C are zero.
inline int dconv_rewrite_perm(int k) {
    const int ks = k / 32, g = (k % 32) / 8, i = k % 8;
    return 32 * ks + (i < 4 ? 4 * g + i : 16 + 4 * g + (i - 4));
}
// The last decoder level folded with its 1x1 output projection (dec_last.hip's header), in double.  w: ConvT weight
// [48][4][8], b: its bias [4], P: freq_out / time_out weight [2][4], pb: its bias [2]; br 0 = freq, 1 = time.
//   freq: [Am | A0 | Ap] (3 x [2][48]: P W7 / 2, P (W3 + W4) / 2, P W0 / 2), P b + pb (2), 0.1 P (8)
//   time: Q_k = P W_k (8 x [2][48]), P b (2), pb (2), 0.1 P (8)
inline std::vector<float> dec_last_fold(const std::vector<float>& w, const std::vector<float>& b,
                                        const std::vector<float>& P, const std::vector<float>& pb, int br) {
    const int cin = 48, co = 4;
    auto pw = [&](int j, int ci, int k) {     // (P W_k)[j][ci]
        double a = 0.0;
        for (int cc = 0; cc < co; ++cc) a += (double)P[j * co + cc] * w[((size_t)ci * co + cc) * 8 + k];
        return a;
    };
    double pbias[2];
    for (int j = 0; j < 2; ++j) {
        pbias[j] = 0.0;
        for (int cc = 0; cc < co; ++cc) pbias[j] += (double)P[j * co + cc] * b[cc];
    }
    std::vector<float> f;
    if (br == 0) {
        for (int m = 0; m < 3; ++m)
            for (int j = 0; j < 2; ++j)
                for (int ci = 0; ci < cin; ++ci)
                    f.push_back((float)(0.5 * (m == 0 ? pw(j, ci, 7) : m == 1 ? pw(j, ci, 3) + pw(j, ci, 4) : pw(j, ci, 0))));
        for (int j = 0; j < 2; ++j) f.push_back((float)(pbias[j] + pb[j]));
    } else {
        for (int k = 0; k < 8; ++k)
            for (int j = 0; j < 2; ++j)
                for (int ci = 0; ci < cin; ++ci) f.push_back((float)pw(j, ci, k));
        for (int j = 0; j < 2; ++j) f.push_back((float)pbias[j]);
        for (int j = 0; j < 2; ++j) f.push_back(pb[j]);
    }
    for (int j = 0; j < 2; ++j)
        for (int cc = 0; cc < co; ++cc) f.push_back((float)(0.1 * P[j * co + cc]));
    return f;
}

// GLU pair order of a [n = 2C] layer: per 32 packed rows [a(16q..16q+15) | gate(C+16q..)]; packed row pr is natural
// row glu_src(pr, n)
inline int glu_src(int pr, int n) {
    const int C = n / 2, qq = pr / 32, s = pr % 32;
    return s < 16 ? 16 * qq + s : C + 16 * qq + (s - 16);
}
// the rows of v ([n][K] row-major; K = 1: a bias or an affine) in GLU pair order
inline std::vector<float> glu_order(const std::vector<float>& v, int K = 1) {
    std::vector<float> o(v.size());
    const int n = (int)(v.size() / K);
    for (int pr = 0; pr < n; ++pr) std::memcpy(&o[(size_t)pr * K], &v[(size_t)glu_src(pr, n) * K], (size_t)K * 4);
    return o;
}

// conv weight [Cout][Cin][taps] -> [Cout][tap * Cin + ci]
inline std::vector<float> conv_tap_major(const std::vector<float>& w, int cout, int cin, int taps) {
    std::vector<float> p((size_t)cout * taps * cin);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < taps; ++t) p[((size_t)co * taps + t) * cin + ci] = w[((size_t)co * cin + ci) * taps + t];
    return p;
}

// a packed matrix with its bias, rows and bias in the same order
struct PackedRows {
    std::vector<float> w, bias;
};

// rows [row0, row0 + rows) of a linear layer w [N][K], b [N]; the first `scaled_rows` (weights and bias) times `scale`
inline PackedRows lin_rows(const std::vector<float>& w, const std::vector<float>& b, int K, int row0, int rows,
                           int scaled_rows, float scale) {
    PackedRows p{{w.begin() + (size_t)row0 * K, w.begin() + (size_t)(row0 + rows) * K},
                 {b.begin() + row0, b.begin() + row0 + rows}};
    for (int n = 0; n < scaled_rows && n < rows; ++n) {
        for (int k = 0; k < K; ++k) p.w[(size_t)n * K + k] *= scale;
        p.bias[n] *= scale;
    }
    return p;
}

// M' = L . M, m' = L . m + l for L [D][D] (fp32), M [D][TD], in double
inline void affine_compose(const float* L, const float* l, const std::vector<double>& M, const std::vector<double>& m,
                           int D, int TD, std::vector<double>& Mo, std::vector<double>& mo) {
    Mo.assign((size_t)D * TD, 0.0);
    mo.assign(D, 0.0);
    for (int r = 0; r < D; ++r) {
        double* row = &Mo[(size_t)r * TD];
        double acc = l[r];
        for (int q = 0; q < D; ++q) {
            const double lv = L[(size_t)r * D + q];
            const double* mr = &M[(size_t)q * TD];
            for (int k = 0; k < TD; ++k) row[k] += lv * mr[k];
            acc += lv * m[q];
        }
        mo[r] = acc;
    }
}

// ConvTranspose (k8 s4 p2) residue classes: output row 4u+rho = taps in rows u+in_off, u+in_off+1 with kernel
// indices {k0, k1}
constexpr int RES_OFF[4] = {-1, -1, 0, 0};
constexpr int RES_K0[4] = {6, 7, 4, 5};
constexpr int RES_K1[4] = {2, 3, 0, 1};

// ConvTranspose weight w [cin][cout][8], bias b [cout] as GEMM rows over a window of input rows u + row_lo + j,
// j < nrows: row [i * cout + co] of residue res[i] holds at K = j * cin + ci the tap with which that residue reads
// input row u + row_lo + j, and zero where it does not read the row; the bias once per residue
inline PackedRows convt_rows(const std::vector<float>& w, const std::vector<float>& b, int cin, int cout,
                             const std::vector<int>& res, int row_lo, int nrows) {
    const size_t K = (size_t)nrows * cin;
    PackedRows p{std::vector<float>(res.size() * cout * K, 0.f), std::vector<float>(res.size() * cout)};
    for (size_t i = 0; i < res.size(); ++i) {
        const int r = res[i], j0 = RES_OFF[r] - row_lo;      // the window's slot of the residue's first row
        for (int co = 0; co < cout; ++co) {
            float* row = &p.w[(i * cout + co) * K];
            for (int ci = 0; ci < cin; ++ci) {
                const float* taps = &w[((size_t)ci * cout + co) * 8];
                if (j0 >= 0 && j0 < nrows) row[(size_t)j0 * cin + ci] = taps[RES_K0[r]];
                if (j0 + 1 >= 0 && j0 + 1 < nrows) row[(size_t)(j0 + 1) * cin + ci] = taps[RES_K1[r]];
            }
            p.bias[i * cout + co] = b[co];
        }
    }
    return p;
}
// residue pair pi: rows [residue 2pi | residue 2pi+1], K = the pair's two input rows
inline PackedRows convt_pair(const std::vector<float>& w, const std::vector<float>& b, int cin, int cout, int pi) {
    return convt_rows(w, b, cin, cout, {2 * pi, 2 * pi + 1}, RES_OFF[2 * pi], 2);
}
// all four residues over rows u-1 | u | u+1 (a zero block where a residue does not read that row)
inline PackedRows convt_quad(const std::vector<float>& w, const std::vector<float>& b, int cin, int cout) {
    return convt_rows(w, b, cin, cout, {0, 1, 2, 3}, -1, 3);
}
// convt4.hip: all four residues, each over its own two input rows only (K = 2 cin), in bf16
inline std::vector<uint16_t> convt4_rows(const std::vector<float>& w, const std::vector<float>& b, int cin, int cout) {
    std::vector<uint16_t> q;
    for (int r = 0; r < 4; ++r)
        for (float v : convt_rows(w, b, cin, cout, {r}, RES_OFF[r], 2).w) q.push_back(host_f2bf(v));
    return q;
}

}  // namespace athd
