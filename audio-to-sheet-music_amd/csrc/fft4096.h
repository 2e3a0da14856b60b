// The 4096-point register FFT and the overlap-add envelope shared by the spectral kernels (spectral.hip: STFT and fused
// iSTFT; head_grad.hip: the adjoint of the fused mask + iSTFT).  Device code only.
#pragma once
#include "common.h"

namespace athd {

constexpr int NFFT = 4096;
constexpr int HOP = 1024;

template <typename R>
struct cx { R x, y; };
using cpx = cx<float>;
template <typename R> ATHD_DEV cx<R> cadd(cx<R> a, cx<R> b) { return {a.x + b.x, a.y + b.y}; }
template <typename R> ATHD_DEV cx<R> csub(cx<R> a, cx<R> b) { return {a.x - b.x, a.y - b.y}; }
template <typename R> ATHD_DEV cx<R> cmul(cx<R> a, cx<R> b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }

// 4096-point forward FFT (e^{-2 pi i}) with 256 threads as three radix-16 Stockham passes (4096 = 16^3).  Each
// thread keeps 16 points in registers; a pass is twiddle -> 16-point DFT in registers, and only the two
// exchanges between passes go through LDS (vs six LDS round trips for radix-4).  Pass Ns (1, 16, 256): thread j
// holds a[j + 256 r], multiplies by tw[(j mod Ns) r 4096/(16 Ns)] and writes its DFT output q to
// (j / Ns) 16 Ns + (j mod Ns) + q Ns.  After the last pass thread j holds X[j + 256 q] with no store needed.
// LDS slots are padded (one per 16) so that the stride-16 stores of the first exchange are conflict-free.
//
// R = float in throughput (bf16) mode.  R = double in the f32 parity mode: Z_k is then the correctly rounded fp32
// value, and a stored component (Z_k +- Z_-k) / 128 carries those two roundings and that of the sum: within
// 2^-24 (|Z_k| + |Z_-k|) / 128 + 2^-24 |X| of the exact spectrum (tests/spectral_refs.py), up to three roundings, not
// the one of a correctly rounded X.  That matters because the reference's phase term z / (Re z_L + 1e-8)
// (ATHTDemucs_v2.py:308) is singular: at a bin with Re z_L within a few 1e-8 of -1e-8 the output depends on the
// last bits of the FFT, and an fp32 FFT whose rounding differs from torch's (another summation order) can move
// the whole-output SDR by tens of dB on the reference fixtures.  A spectrum this close to the exact one stays within
// ~90 dB of the reference output on all of them.
constexpr int FPAD = NFFT + NFFT / 16;
ATHD_DEV int pidx(int i) { return i + (i >> 4); }

// in-place forward radix-4: (x0, x1, x2, x3) <- DFT4
template <typename R>
ATHD_DEV void r4(cx<R>& x0, cx<R>& x1, cx<R>& x2, cx<R>& x3) {
    const cx<R> s02 = cadd(x0, x2), d02 = csub(x0, x2), s13 = cadd(x1, x3), d13 = csub(x1, x3);
    const cx<R> md13 = {d13.y, -d13.x};                  // -i * d13
    x0 = cadd(s02, s13);
    x1 = cadd(d02, md13);
    x2 = csub(s02, s13);
    x3 = csub(d02, md13);
}

// 16-point DFT as 4 x 4: v[r] (r = 4 r1 + r0) in; output bin q = k0 + 4 k1 is left in v[4 k0 + k1] (see vq)
template <typename R>
ATHD_DEV void dft16(cx<R> (&v)[16]) {
    constexpr R C1 = (R)0.92387953251128675613, S1 = (R)0.38268343236508977173, C2 = (R)0.70710678118654752440;
#pragma unroll
    for (int r0 = 0; r0 < 4; ++r0) r4(v[r0], v[4 + r0], v[8 + r0], v[12 + r0]);
    // a[r0][k0] sits in v[r0 + 4 k0]; multiply by W16^(r0 k0)
    v[1 + 4] = cmul(v[5], {C1, -S1});      // W^1
    v[1 + 8] = cmul(v[9], {C2, -C2});      // W^2
    v[1 + 12] = cmul(v[13], {S1, -C1});    // W^3
    v[2 + 4] = cmul(v[6], {C2, -C2});      // W^2
    v[2 + 8] = {v[10].y, -v[10].x};        // W^4 = -i
    v[2 + 12] = cmul(v[14], {-C2, -C2});   // W^6
    v[3 + 4] = cmul(v[7], {S1, -C1});      // W^3
    v[3 + 8] = cmul(v[11], {-C2, -C2});    // W^6
    v[3 + 12] = cmul(v[15], {-C1, S1});    // W^9
#pragma unroll
    for (int k0 = 0; k0 < 4; ++k0) r4(v[4 * k0], v[4 * k0 + 1], v[4 * k0 + 2], v[4 * k0 + 3]);
}
// register holding DFT16 output bin q
ATHD_DEV constexpr int vq(int q) { return 4 * (q & 3) + (q >> 2); }

// One LDS exchange: DFT output q of this thread goes to slot dst(q), then v[r] = slot j + 256 r.  `lds` holds
// FPAD 8-byte words: complex floats, or the real and then the imaginary parts of complex doubles.  Ends synced.
template <typename R, typename Dst>
ATHD_DEV void exchange(cx<R> (&v)[16], void* lds, Dst dst, int j) {
    if constexpr (sizeof(R) == 4) {
        cpx* b = reinterpret_cast<cpx*>(lds);
#pragma unroll
        for (int q = 0; q < 16; ++q) b[pidx(dst(q))] = v[vq(q)];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = b[pidx(j + 256 * r)];
        __syncthreads();
    } else {
        R* b = reinterpret_cast<R*>(lds);
        R t[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) b[pidx(dst(q))] = v[vq(q)].x;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) t[r] = b[pidx(j + 256 * r)];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 16; ++q) b[pidx(dst(q))] = v[vq(q)].y;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = {t[r], b[pidx(j + 256 * r)]};
        __syncthreads();
    }
}

// v[r] = x[threadIdx.x + 256 r] on entry; X[threadIdx.x + 256 q] = v[vq(q)] on exit.  tw[m] = e^{-2 pi i m/4096}.
// j = threadIdx.x (a parameter so that a caller looping over frames can make it opaque per iteration)
// Twiddles of the Ns = 16 and Ns = 256 passes: w^r for r = 1..15 with w = tw[16 (j & 15)] and w = tw[j].  R = double
// (the f32 parity mode) reads every power from the table; R = float takes them as running products of the two base
// twiddles the caller loaded once (tw16, tw256): no table loads per frame (30 dependent L2 round trips per frame were
// most of the iSTFT's wait time, SQ).  w^r then carries r times the base's rounding and r - 1 complex-product roundings:
// at most (r + (r - 1) sqrt 5) 2^-24 = 46 x 2^-24 on w^15 in the worst case, 11 x 2^-24 at most over the 2 x 256 chains
// this table produces (tests/test_spectral_refs.py), which keeps the per-frame error of the transform within the L2
// criterion of tests/spectral_refs.py.
// (no defaults for tw16 / tw256: a float caller that forgot them would run on zero twiddles)
template <typename R, typename TW>
ATHD_DEV void fft4096(cx<R> (&v)[16], void* lds, const TW* __restrict__ tw, int j, cpx tw16, cpx tw256) {
    constexpr bool REC = sizeof(R) == 4;
    dft16(v);                                                       // Ns = 1: no twiddles
    exchange(v, lds, [j](int q) { return 16 * j + q; }, j);
    {                                                               // Ns = 16
        const int k = j & 15;
        cx<R> w = {(R)tw16.x, (R)tw16.y};
#pragma unroll
        for (int r = 1; r < 16; ++r) {
            if constexpr (REC) {
                v[r] = cmul(v[r], w);
                // (pinned: the product chain interleaved with its uses, not all 15 powers held at once)
                asm volatile("" : "+v"(w.x), "+v"(w.y), "+v"(v[r].x), "+v"(v[r].y));
                if (r < 15) w = cmul(w, {(R)tw16.x, (R)tw16.y});
            } else {
                const TW t = tw[k * r * 16];
                v[r] = cmul(v[r], {t.x, t.y});
            }
        }
        dft16(v);
        const int base = (j >> 4) * 256 + k;
        exchange(v, lds, [base](int q) { return base + 16 * q; }, j);
    }
    cx<R> w = {(R)tw256.x, (R)tw256.y};
#pragma unroll
    for (int r = 1; r < 16; ++r) {                                  // Ns = 256
        if constexpr (REC) {
            v[r] = cmul(v[r], w);
            // (pinned: the product chain interleaved with its uses, not all 15 powers held at once)
            asm volatile("" : "+v"(w.x), "+v"(w.y), "+v"(v[r].x), "+v"(v[r].y));
            if (r < 15) w = cmul(w, {(R)tw256.x, (R)tw256.y});
        } else {
            const TW t = tw[j * r];
            v[r] = cmul(v[r], {t.x, t.y});
        }
    }
    dft16(v);
}
// the two base twiddles of fft4096's running products for thread j (R = float only)
template <typename TW>
ATHD_DEV void fft4096_base(const TW* __restrict__ tw, int j, cpx& tw16, cpx& tw256) {
    const TW a = tw[16 * (j & 15)], c = tw[j];
    tw16 = {(float)a.x, (float)a.y};
    tw256 = {(float)c.x, (float)c.y};
}

// interior overlap-add envelope (the sum of win^2 over the four frames B-3 .. B that cover a hop block, in ascending
// order) at offsets j + 256 o of the block; win2 = win * win
ATHD_DEV void ola_env_in(int j, const float* __restrict__ win2, float (&e)[4]) {
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int q = 3 * HOP + j + 256 * o;
        e[o] = ((win2[q] + win2[q - HOP]) + win2[q - 2 * HOP]) + win2[q - 3 * HOP];
    }
}

}  // namespace athd
