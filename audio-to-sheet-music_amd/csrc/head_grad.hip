// Head training's output stage (gfx950): the adjoint of the fused mask + iSTFT of spectral.hip, and the packing of the
// exported spectrogram into the frame-major layout both directions read.
//
// Forward (istft_ola_kernel, ATHTDemucs_v2.py:303-324), per item and channel c with N = 4096, HOP = 1024:
//   mask_c = sigmoid(resize(xd_c)), X_c = mask_c w_c with w_c = m_c z_c / (m_c + 1e-8), (m_0, m_1) = (Re z_0, Im z_0),
//   out = istft(X) + (xt std + mean), the DC bin's imaginary part and the Nyquist bin zero.
// Adjoint, given g = dL/dout (B, 2, T):
//   u[q] = g[q - 3584] / env[q mod 1024] (zero outside the samples; every such q lies in an interior hop block)
//   G_c[kb, t] = (c_kb / 64) sum_m u_c[1024 (t + 2) + m] win[m] e^{-2 pi i kb m / 4096},  c_0 = 1, c_kb = 2, Im G_c[0] = 0
//   dmask_c = Re G_c Re w_c + Im G_c Im w_c,  dup_c = dmask_c mask_c (1 - mask_c)
//   dxd_c[r, t] = sum_kb (l0(kb) [i0(kb) = r] + l1(kb) [i1(kb) = r]) dup_c[kb, t]      (the resize table, transposed)
// i.e. an STFT of the gradient: both channels go through ONE complex FFT (u_0 + i u_1) and are split through the
// Hermitian pair (k, 4096 - k), as stft_kernel does with the waveform.
//
// One workgroup per (item, frame).  Every element of grad_logits is written exactly once by exactly one workgroup, the
// transposed resize is summed by one thread per row in ascending bin order, and there are no atomics: the result is the
// same bits on every run and does not depend on what the caller left in the output.  Plain f32 arithmetic with IEEE
// expf and divisions, one variant for both context dtypes: this is not the inference throughput path.
#include <stdint.h>

#include "common.h"
#include "fft4096.h"
#include "kernels.h"
#include "prof.h"

namespace athd {

// LDS: buf 34816 B + ltab 16384 B + dup 16384 B = 67584 B, two workgroups per CU
__global__ __launch_bounds__(256) void head_grad_kernel(const float* __restrict__ g, const float* __restrict__ fo,
                                                        const float* __restrict__ specT, int Tspec, int T,
                                                        const float2* __restrict__ tw, const float* __restrict__ win,
                                                        const float* __restrict__ win2, float* __restrict__ gfo) {
    __shared__ cpx buf[FPAD];
    __shared__ uint2 ltab[2048];       // the forward's resize table: {i0 | i1 << 16, l1}
    __shared__ float2 dup[2048];       // dL/d(resized logits) of this frame, both channels
    // the four frames that share a hop of g run on one XCD (stft_kernel's order)
    const int id = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int t = id % Tspec;
    const int64_t b = id / Tspec;
    const int j = threadIdx.x;
    for (int kb = j; kb < 2048; kb += 256) {
        const LinIdx li = lin_index(kb, Tspec, 2048);
        ltab[kb] = make_uint2((uint32_t)li.i0 | ((uint32_t)li.i1 << 16), __float_as_uint(li.l1));
    }
    float env[4];
    ola_env_in(j, win2, env);
    // ---- u win / 64 of frame t: positions q = 1024 (t + 2) + m, samples n = q - 3584 ----
    const float* g0 = g + b * 2 * T;
    const float* g1 = g0 + T;          // (not 16-byte aligned for odd T: scalar loads, coalesced along j)
    const int n0 = t * HOP - 1536;
    cpx v[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = j + 256 * r, n = n0 + m;
        const bool in = n >= 0 && n < T;
        const float a0 = in ? g0[n] : 0.f, a1 = in ? g1[n] : 0.f;
        const float wq = win[m] * (1.f / 64.f);
        v[r] = {(a0 / env[r & 3]) * wq, (a1 / env[r & 3]) * wq};
    }
    cpx tw16, tw256;
    fft4096_base(tw, j, tw16, tw256);
    fft4096(v, buf, tw, j, tw16, tw256);                   // (its last exchange ends synced: buf is free)
#pragma unroll
    for (int q = 0; q < 16; ++q) buf[pidx(j + 256 * q)] = v[vq(q)];
    __syncthreads();                                       // buf and ltab
    // ---- G, the mask recomputed from the logits, dup ----
    const float* F0 = fo + (b * Tspec + t) * (int64_t)Tspec * 2;
    const float* S = specT + (b * Tspec + t) * 2048LL * 4;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int kb = j + 256 * i;
        const cpx zk = buf[pidx(kb)], zn = buf[pidx((NFFT - kb) & (NFFT - 1))];
        // G_0 = c_kb (zk + conj zn) / 2, G_1 = c_kb (zk - conj zn) / (2i); at kb = 0 (zn = zk) both are real
        const float s = kb == 0 ? 0.5f : 1.0f;
        const cpx G0 = {(zk.x + zn.x) * s, (zk.y - zn.y) * s};
        const cpx G1 = {(zk.y + zn.y) * s, -(zk.x - zn.x) * s};
        const uint2 e = ltab[kb];
        const float l1 = __uint_as_float(e.y), l0 = 1.f - l1;
        const float2 ra = *reinterpret_cast<const float2*>(F0 + 2 * (int)(e.x & 0xFFFFu));
        const float2 rb = *reinterpret_cast<const float2*>(F0 + 2 * (int)(e.x >> 16));
        const float m0 = sigmoidf_(l0 * ra.x + l1 * rb.x), m1 = sigmoidf_(l0 * ra.y + l1 * rb.y);
        const float4 z = *reinterpret_cast<const float4*>(S + (int64_t)kb * 4);
        const float d0 = z.x + 1e-8f, d1 = z.y + 1e-8f;
        const float dm0 = z.x * (G0.x * (z.x / d0) + G0.y * (z.y / d0));
        const float dm1 = z.y * (G1.x * (z.z / d1) + G1.y * (z.w / d1));
        dup[kb] = make_float2(dm0 * (m0 * (1.f - m0)), dm1 * (m1 * (1.f - m1)));
    }
    __syncthreads();
    // ---- the transposed resize: row r takes the bins with i0 = r or i1 = r, one contiguous range (i0 and i1 do not
    // decrease with kb and i1 <= i0 + 1 while Tspec <= 2048), summed in ascending kb by one thread ----
    float* O = gfo + (b * Tspec + t) * (int64_t)Tspec * 2;
    for (int r = j; r < Tspec; r += 256) {
        int lo = 0, hi = 2048;                             // first kb with i1(kb) >= r
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int)(ltab[mid].x >> 16) >= r) hi = mid;
            else lo = mid + 1;
        }
        float s0 = 0.f, s1 = 0.f;
        for (int kb = lo; kb < 2048; ++kb) {
            const uint2 e = ltab[kb];
            const int i0 = (int)(e.x & 0xFFFFu), i1 = (int)(e.x >> 16);
            if (i0 > r) break;
            const float l1 = __uint_as_float(e.y);
            const float w = (i0 == r ? 1.f - l1 : 0.f) + (i1 == r ? l1 : 0.f);
            const float2 d = dup[kb];
            s0 += w * d.x;
            s1 += w * d.y;
        }
        *reinterpret_cast<float2*>(O + 2 * r) = make_float2(s0, s1);
    }
}

int head_grad_launch(const float* g, const float* fo, const float* specT, int64_t B, int Tspec, int64_t T,
                     const float2* tw, const float* win, const float* win2, float* gfo, hipStream_t s) {
    if (!g || !fo || !specT || !tw || !win || !win2 || !gfo || B <= 0 || T <= 0) return -1;
    if (Tspec != (T + HOP - 1) / HOP || Tspec > 2048 || B * Tspec > 0x7fffffffLL) return -1;
    KScope ks(s);
    if (ks.on())
        ks.begin("head_grad_kernel", 0.0,
                 (double)B * 2 * T * 4 + (double)B * 2048 * Tspec * 4 * 4 + 2.0 * B * Tspec * Tspec * 2 * 4);
    hipLaunchKernelGGL(head_grad_kernel, dim3((unsigned)(B * Tspec)), dim3(256), 0, s, g, fo, specT, Tspec, (int)T, tw,
                       win, win2, gfo);
    return (int)hipGetLastError();
}

// --------------------------------------------------------------------------------------------- spectrogram, packed
// z[b][ch][f][t] = {Re, Im} (athd_encode's export) -> specT[b][t][f] = {Re L, Im L, Re R, Im R}: the exact inverse of
// export_spec_kernel (export.hip), the same tile of PT frames x PT bins per audio channel.  Reads: 8 B per lane along
// t; writes: 16 B per lane along f.
constexpr int PT = 32;

__global__ __launch_bounds__(256) void pack_spec_kernel(const float* __restrict__ z, int Tspec,
                                                        float* __restrict__ specT) {
    __shared__ float2 tile[2][PT][PT + 1];
    const int64_t b = blockIdx.z;
    const int f0 = blockIdx.x * PT, t0 = blockIdx.y * PT;
    const int th = min(PT, Tspec - t0);
    for (int i = threadIdx.x; i < 2 * PT * PT; i += 256) {
        const int t = i & (PT - 1), f = (i >> 5) & (PT - 1), ch = i >> 10;
        if (t < th)
            tile[ch][f][t] = *reinterpret_cast<const float2*>(z + (((b * 2 + ch) * 2048LL + f0 + f) * Tspec + t0 + t) * 2);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < th * PT; i += 256) {
        const int t = i >> 5, f = i & (PT - 1);
        const float2 l = tile[0][f][t], r = tile[1][f][t];
        *reinterpret_cast<float4*>(specT + ((b * Tspec + t0 + t) * 2048LL + f0 + f) * 4) = make_float4(l.x, l.y, r.x, r.y);
    }
}

int pack_spec_launch(const float* z, int64_t B, int64_t Tspec, float* specT, hipStream_t s) {
    if (!z || !specT || B <= 0 || B > 65535 || Tspec <= 0 || Tspec > 65535LL * PT) return -1;
    const dim3 grid(2048 / PT, (unsigned)((Tspec + PT - 1) / PT), (unsigned)B);
    KScope ks(s);
    if (ks.on()) ks.begin("pack_spec_kernel", 0.0, (double)B * Tspec * 2048 * 4 * 8);
    hipLaunchKernelGGL(pack_spec_kernel, grid, dim3(256), 0, s, z, (int)Tspec, specT);
    return (int)hipGetLastError();
}

}  // namespace athd
