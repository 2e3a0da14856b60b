// DConv (demucs residual dilated-conv branch), bf16 mode: the three passes of one layer with
// their weights resident in LDS (apply, conv3, gn_gelu_mom between them; C = 48, 96, 192, 384), and dconv_plan, which
// decides a level's launches from the launchers' shape predicates.  (The narrow levels' VALU layer: dconv_small.hip.)
#include <algorithm>

#include "common.h"
#include "prof.h"
#include "kernels.h"

namespace athd {

// Wide levels (C = 192, 384; bf16 mode): the DConv 1x1 apply  x += LayerScale(GLU(GN(W1 hb + b1)))  as a weights-
// resident MFMA pass (the pattern of convt4.hip) instead of a tiled GEMM: K = H = C/8 (24, 48) is one or two 32-wide
// K-steps, so the tiled GEMM (gemm3 / gemm5, one K-tile per 256-row tile) was all prologue and epilogue at ~7 GB/s
// per CU.  Here the packed 1x1 weights ([2C][64] bf16, GLU-interleaved columns, 48 / 96 KB) are loaded into LDS once
// per workgroup (XOR-swizzled 16-B chunks, conflict-free fragment reads as gemm3), and every wave walks 16-row units
// with no workgroup barrier: per unit the lane's activation fragment (row m, 8 hidden channels per K-step) comes from
// global memory, all of the row's residual channels are loaded up front, and the 2C columns are processed one
// GLU pair (32 packed columns -> 16 output channels) at a time: 2 x KS MFMAs, GroupNorm -> GLU -> LayerScale ->
// residual on the lane's 4 channels of row m, one 8-B store.
struct DcApply {
    const uint16_t* hb;        // [M][H] bf16 GELU(GN(h))
    const uint16_t* w;         // [2C][kp] packed GLU-interleaved 1x1 weights (kp == 64)
    const float* bias;         // [2C] packed
    const double* st;          // per group {sum, sumsq} of the 1x1 output
    const float* gn_w;         // [2C] packed
    const float* gn_b;
    const float* scale;        // [C] LayerScale
    uint16_t* x;               // [M][C] bf16 residual stream, updated in place
    int64_t M, L, gn_count;
    int kp;
    // fused rewrite (RW, C = 48 / 96, the layer's second DConv layer): out = GLU(Wr x + br) of the updated rows
    // instead of storing x; rw [2C][rkp] GLU-interleaved rows with the K order of ctx.h dconv_rewrite_perm
    const uint16_t* rw = nullptr;
    const float* rbias = nullptr;  // [2C] packed
    uint16_t* out = nullptr;       // [M][C] bf16
    uint16_t* c4 = nullptr;        // optional [M][4]: channels 0..3 of out again (the decoder's compact skip)
    int rkp = 0;
};

template <int C, int NW, bool RW = false>
__global__ __launch_bounds__(NW * 64) void dconv_apply_kernel(const DcApply d) {
    constexpr int H = C / 8, KS = (H + 31) / 32, NP = C / 16;      // K-steps, GLU pairs (16 output channels each)
    constexpr int HS = H % 8 == 0 ? H : (H + 15) / 16 * 16;       // hidden row stride (H = 6, 12: padded to 16)
    constexpr int RK = (C + 31) / 32;                              // rewrite K-steps
    constexpr int RPB = RW ? (RK * 4 + 7) / 8 * 128 : 0;           // rewrite LDS row bytes (chunks padded to 8 k)
    __shared__ __attribute__((aligned(16))) char wl[2 * C * 128 + 2 * C * RPB];
    // per packed column: bias, GroupNorm weight, bias; per output channel: LayerScale; (RW) per packed rewrite column:
    // bias
    __shared__ __attribute__((aligned(16))) float cst[3 * 2 * C + C + (RW ? 2 * C : 0)];
    for (int i = threadIdx.x; i < 2 * C * 8; i += NW * 64) {
        const int row = i >> 3, ch = i & 7;
        const uint4 v = *reinterpret_cast<const uint4*>(d.w + (int64_t)row * d.kp + ch * 8);
        *reinterpret_cast<uint4*>(wl + row * 128 + ((ch ^ (row & 7)) * 16)) = v;
    }
    for (int i = threadIdx.x; i < 2 * C; i += NW * 64) {
        cst[i] = d.bias[i];
        cst[2 * C + i] = d.gn_w[i];
        cst[4 * C + i] = d.gn_b[i];
    }
    for (int i = threadIdx.x; i < C; i += NW * 64) cst[6 * C + i] = d.scale[i];
    char* const wr = wl + 2 * C * 128;
    if constexpr (RW) {
        for (int i = threadIdx.x; i < 2 * C * (RPB / 16); i += NW * 64) {
            const int row = i / (RPB / 16), ch = i % (RPB / 16);
            const uint4 v = ch < RK * 4 ? *reinterpret_cast<const uint4*>(d.rw + (int64_t)row * d.rkp + ch * 8)
                                        : make_uint4(0u, 0u, 0u, 0u);
            *reinterpret_cast<uint4*>(wr + row * RPB + ((ch ^ (row & 7)) * 16)) = v;
        }
        for (int i = threadIdx.x; i < 2 * C; i += NW * 64) cst[7 * C + i] = d.rbias[i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, fr = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nunits = (d.M + 15) / 16;
    const int64_t stride = (int64_t)gridDim.x * NW;
    typedef __attribute__((ext_vector_type(8))) __bf16 bf16v8;
    auto wfrag = [&](int t, int ks) -> bf16v8 {
        return *reinterpret_cast<const bf16v8*>(wl + (16 * t + fr) * 128 + (((4 * ks + g) ^ (fr & 7)) * 16));
    };
    for (int64_t u = (int64_t)blockIdx.x * NW + wave; u < nunits; u += stride) {
        const int64_t m = u * 16 + fr;
        const bool ok = m < d.M;
        const int64_t mm = ok ? m : d.M - 1;
        // activation fragments: hidden channels 32 ks + 8 g .. + 7 of row mm (zero past H)
        bf16v8 af[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int k0 = 32 * ks + 8 * g;
            af[ks] = k0 < H ? *reinterpret_cast<const bf16v8*>(d.hb + mm * HS + k0) : bf16v8{};
        }
        // the row's residual channels 16 p + 4 g .. + 3, PG pairs per group; the next group's loads are issued
        // before the current group's MFMAs (the first group's before the GroupNorm parameters)
        constexpr int PG = NP % 6 == 0 ? 6 : NP, NG = NP / PG;
        static_assert(NP % PG == 0, "pair groups");
        static_assert(!RW || NG == 1, "the fused rewrite keeps all of the row's pairs in registers");
        uint2 xk[RW ? NP : 1];            // (RW) the updated bf16 x channels 16 p + 4 g .. + 3 of row m
        const uint16_t* xr = d.x + mm * C + 4 * g;
        uint2 rr[PG];
#pragma unroll
        for (int p = 0; p < PG; ++p) rr[p] = *reinterpret_cast<const uint2*>(xr + 16 * p);
        float gm, gr;
        gn_params(d.st, mm / d.L, d.gn_count, gm, gr);
        uint2* const xo = reinterpret_cast<uint2*>(d.x + mm * C + 4 * g);
#pragma unroll 1
        for (int gi = 0; gi < NG; ++gi) {
            uint2 rn[PG];
            if (gi + 1 < NG) {
#pragma unroll
                for (int p = 0; p < PG; ++p) rn[p] = *reinterpret_cast<const uint2*>(xr + 16 * (PG * (gi + 1) + p));
            }
            // (an opaque per-group LDS base: the column constants are read here, not hoisted out of the loops)
            int cb = 0;
            asm volatile("v_mov_b32 %0, 0" : "=v"(cb));
            const float* cs = cst + cb;
#pragma unroll
            for (int pp = 0; pp < PG; ++pp) {
                const int p = PG * gi + pp;
                f32x4_t aa = {0.f, 0.f, 0.f, 0.f}, ag = aa;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    aa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfrag(2 * p, ks), af[ks], aa, 0, 0, 0);
                    ag = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfrag(2 * p + 1, ks), af[ks], ag, 0, 0, 0);
                }
                const int na = 32 * p + 4 * g, oc = 16 * p + 4 * g;
                const float4 ba = *reinterpret_cast<const float4*>(cs + na), bg = *reinterpret_cast<const float4*>(cs + na + 16);
                const float4 wa = *reinterpret_cast<const float4*>(cs + 2 * C + na), wg = *reinterpret_cast<const float4*>(cs + 2 * C + na + 16);
                const float4 ca = *reinterpret_cast<const float4*>(cs + 4 * C + na), cg = *reinterpret_cast<const float4*>(cs + 4 * C + na + 16);
                const float4 sc = *reinterpret_cast<const float4*>(cs + 6 * C + oc);
                const float bav[4] = {ba.x, ba.y, ba.z, ba.w}, bgv[4] = {bg.x, bg.y, bg.z, bg.w};
                const float wav[4] = {wa.x, wa.y, wa.z, wa.w}, wgv[4] = {wg.x, wg.y, wg.z, wg.w};
                const float cav[4] = {ca.x, ca.y, ca.z, ca.w}, cgv[4] = {cg.x, cg.y, cg.z, cg.w};
                const float scv[4] = {sc.x, sc.y, sc.z, sc.w};
                const uint2 q = rr[pp];
                const float r4[4] = {__uint_as_float(q.x << 16), __uint_as_float(q.x & 0xFFFF0000u),
                                     __uint_as_float(q.y << 16), __uint_as_float(q.y & 0xFFFF0000u)};
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float a = (aa[e] + bav[e] - gm) * gr * wav[e] + cav[e];
                    const float gt = (ag[e] + bgv[e] - gm) * gr * wgv[e] + cgv[e];
                    o[e] = r4[e] + scv[e] * (a * sigmoid_fast(gt));
                }
                if constexpr (RW) xk[pp] = make_uint2(pack2bf(o[0], o[1]), pack2bf(o[2], o[3]));
                else if (ok) xo[4 * p] = make_uint2(pack2bf(o[0], o[1]), pack2bf(o[2], o[3]));
            }
            if (gi + 1 < NG) {
#pragma unroll
                for (int p = 0; p < PG; ++p) rr[p] = rn[p];
            }
        }
        if constexpr (RW) {
            // rewrite: the lane's x values of K-step ks are channels 32 ks + 4 g + {0..3} (pair 2 ks) and
            // 32 ks + 16 + 4 g + {0..3} (pair 2 ks + 1), which is the K order the packed rewrite weights carry, so the
            // B fragments are the registers as they are
            bf16v8 bx[RK];
#pragma unroll
            for (int ks = 0; ks < RK; ++ks) {
                const uint2 lo = xk[2 * ks], hi = 2 * ks + 1 < NP ? xk[2 * ks + 1 < NP ? 2 * ks + 1 : 0] : make_uint2(0u, 0u);
                const uint32_t w4[4] = {lo.x, lo.y, hi.x, hi.y};
                bx[ks] = __builtin_bit_cast(bf16v8, w4);
            }
            uint16_t* const orow = d.out + mm * C + 4 * g;
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                f32x4_t aa = {0.f, 0.f, 0.f, 0.f}, ag = aa;
#pragma unroll
                for (int ks = 0; ks < RK; ++ks) {
                    const bf16v8 fa = *reinterpret_cast<const bf16v8*>(wr + (32 * q + fr) * RPB + (((4 * ks + g) ^ (fr & 7)) * 16));
                    const bf16v8 fg = *reinterpret_cast<const bf16v8*>(wr + (32 * q + 16 + fr) * RPB + (((4 * ks + g) ^ (fr & 7)) * 16));
                    aa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, bx[ks], aa, 0, 0, 0);
                    ag = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fg, bx[ks], ag, 0, 0, 0);
                }
                const int na = 32 * q + 4 * g;
                const float4 ba = *reinterpret_cast<const float4*>(cst + 7 * C + na);
                const float4 bg = *reinterpret_cast<const float4*>(cst + 7 * C + na + 16);
                const float bav[4] = {ba.x, ba.y, ba.z, ba.w}, bgv[4] = {bg.x, bg.y, bg.z, bg.w};
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = (aa[e] + bav[e]) * sigmoid_fast(ag[e] + bgv[e]);
                const uint2 v = make_uint2(pack2bf(o[0], o[1]), pack2bf(o[2], o[3]));
                if (ok) {
                    *reinterpret_cast<uint2*>(orow + 16 * q) = v;
                    if (q == 0 && g == 0 && d.c4) *reinterpret_cast<uint2*>(d.c4 + mm * 4) = v;
                }
            }
        }
    }
}

// Wide levels: the DConv conv3 (C -> H = C/8, 3 taps at dilation dil, zero padding at the GroupNorm row's ends)
// + the GroupNorm statistics of h, as a weights-resident pass (the pattern above; the tiled 256 x 32 GEMM streamed
// the taps' 64-wide K-tiles through LDS at ~2 TB/s).  The packed conv3 weights (H rows padded to 16 NT, K = 3C) sit in
// LDS with XOR-swizzled 16-B chunks; each wave walks a contiguous range of 16-row units (the tap rows +-dil stay in its
// L2 neighbourhood), loads its B fragments x[m + (tap - 1) dil][32 ks + 8 g ..] straight from global memory, and keeps
// the GroupNorm sums in fp64 per lane until the group changes (one wave reduction + atomic pair per change).
struct DcConv3 {
    const uint16_t* x;         // [M][C] bf16
    const uint16_t* w;         // [>= 16 NT][kp] packed conv3 weights, K = tap * C + ci
    const float* bias;         // [H]
    float* h;                  // [M][HF] f32 (HF = H, or 8 for H = 6)
    double* st;                // per group {sum, sumsq}
    int64_t M, L;
    int kp, dil;
};

template <int C, int NW>
__global__ __launch_bounds__(NW * 64) void dconv_conv3_kernel(const DcConv3 d) {
    constexpr int H = C / 8, NT = (H + 15) / 16, KS = (C + 31) / 32, K = 3 * C;
    constexpr int HF = H % 4 == 0 ? H : (H + 7) / 8 * 8;   // f32 hidden row stride (16-B stores)
    constexpr int RB = (K / 8 + 7) / 8 * 128;               // LDS row bytes (chunks padded to a multiple of 8: the
                                                            // XOR swizzle stays inside the row, e.g. C = 96: 36 -> 40)
    __shared__ __attribute__((aligned(16))) char wl[16 * NT * RB];
    for (int i = threadIdx.x; i < 16 * NT * (RB / 16); i += NW * 64) {    // (padding chunks zeroed: the masked
        const int row = i / (RB / 16), q = i % (RB / 16);                      // K-steps of C = 48 multiply them by 0)
        const uint4 v = q < K / 8 ? *reinterpret_cast<const uint4*>(d.w + (int64_t)row * d.kp + q * 8)
                                  : make_uint4(0u, 0u, 0u, 0u);
        *reinterpret_cast<uint4*>(wl + row * RB + ((q ^ (row & 7)) * 16)) = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, fr = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    typedef __attribute__((ext_vector_type(8))) __bf16 bf16v8;
    const int64_t nunits = (d.M + 15) / 16;
    const int64_t nw = (int64_t)gridDim.x * NW, wid = (int64_t)blockIdx.x * NW + wave;
    const int64_t u0 = nunits * wid / nw, u1 = nunits * (wid + 1) / nw;
    float bj[NT][4];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) bj[j][e] = 16 * j + 4 * g + e < H ? d.bias[16 * j + 4 * g + e] : 0.f;
    int64_t cur_b = -1;
    double r1 = 0.0, r2 = 0.0;
    auto flush = [&]() {
        if (cur_b >= 0) {
            const double t1 = wave_sum_d(r1), t2 = wave_sum_d(r2);
            if (lane == 0) {
                atomicAdd(&d.st[2 * cur_b], t1);
                atomicAdd(&d.st[2 * cur_b + 1], t2);
            }
        }
        r1 = r2 = 0.0;
    };
    // unit epilogue: h store + GroupNorm sums (the unit's rows belong to group gb0 of its first row or, past a
    // boundary, gb0 + 1: L >= 16)
    auto finish = [&](int64_t u, const f32x4_t* acc) {
        const int64_t m = u * 16 + fr;
        const bool ok = m < d.M;
        const int64_t mm = ok ? m : d.M - 1;
        const int64_t gb = mm / d.L;
        const int64_t gb0 = (u * 16) / d.L;
        float s1a = 0.f, s2a = 0.f, s1b = 0.f, s2b = 0.f;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[j][e] + bj[j][e];
            const int c0 = 16 * j + 4 * g;
            if (ok && c0 < H) {        // (H = 6: channels 6, 7 of the second chunk are 0 - zero weight rows and bias)
                *reinterpret_cast<float4*>(d.h + mm * HF + c0) = make_float4(v[0], v[1], v[2], v[3]);
                const float p1 = (v[0] + v[1]) + (v[2] + v[3]);
                const float p2 = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
                if (gb == gb0) { s1a += p1; s2a += p2; } else { s1b += p1; s2b += p2; }
            }
        }
        if (gb0 != cur_b) {
            flush();
            cur_b = gb0;
        }
        r1 += (double)s1a;
        r2 += (double)s2a;
        const bool split = __any(gb != gb0);
        if (split) {
            flush();
            cur_b = gb0 + 1;
            r1 = (double)s1b;
            r2 = (double)s2b;
        }
    };
    // C = 96, 192: steps (unit, tap) in ping-pong buffers (below); C = 48, 384 measured slower that way (one box: 0.34
    // -> 0.37 and 0.17 -> 0.18 ms) and keep one tap at a time with the zeroing at the load
    constexpr bool PP = C == 96 || C == 192;
    // lane row of unit u (clamped) and its position in the group row (32-bit: M < 2^31, launcher)
    auto unit_row = [&](int64_t u, int64_t& mm, int& t) {
        const int64_t m = u * 16 + fr;
        mm = m < d.M ? m : d.M - 1;
        t = (int)((uint32_t)mm % (uint32_t)d.L);
    };
    // B fragments of one tap: x[mm + (tap - 1) dil][32 ks + 8 g ..]; returns whether the tap row lies inside the group
    // row.  PP: the loads are unconditional (rows outside the group read the lane's own row, K-steps past C its first
    // chunk) and the fragments are zeroed where they are used, so a prefetched step is not waited for at the load.
    auto load_tap = [&](int64_t mm, int t, int tap, bf16v8* bf) -> bool {
        const int tt = t + (tap - 1) * d.dil;
        const bool in = tt >= 0 && tt < (int)d.L;
        const uint16_t* xr = d.x + (mm + (in ? (int64_t)(tap - 1) * d.dil : 0)) * C + 8 * g;
        if constexpr (PP) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
                bf[ks] = *reinterpret_cast<const bf16v8*>(xr + (32 * ks + 8 * g < C ? 32 * ks : 0));
        } else {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
                bf[ks] = in && 32 * ks + 8 * g < C ? *reinterpret_cast<const bf16v8*>(xr + 32 * ks) : bf16v8{};
        }
        return in;
    };
    auto mfma_tap = [&](int tap, bool in, const bf16v8* bf, f32x4_t* acc) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int q = (tap * C + 32 * ks) / 8 + g;
            const bf16v8 b = !PP || (in && 32 * ks + 8 * g < C) ? bf[ks] : bf16v8{};
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const bf16v8 af = *reinterpret_cast<const bf16v8*>(wl + (16 * j + fr) * RB + ((q ^ (fr & 7)) * 16));
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, b, acc[j], 0, 0, 0);
            }
        }
    };
    f32x4_t acc[NT];
    if constexpr (PP) {
        // the load side runs one step ahead of the compute side: the next step's fragments are in flight during
        // this step's MFMAs and the unit epilogue (registers: 2 x 4 KS)
        int64_t lu = u0, lmm = 0, cu = u0;
        int ltap = 0, lt = 0, ctap = 0;
        if (u0 < u1) unit_row(u0, lmm, lt);
        auto advance = [&]() {
            if (++ltap == 3) {
                ltap = 0;
                if (++lu < u1) unit_row(lu, lmm, lt);
            }
        };
        auto compute = [&](bool in, const bf16v8* bf) {
            if (ctap == 0) {
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            }
            mfma_tap(ctap, in, bf, acc);
            if (ctap == 2) {
                finish(cu, acc);
                ctap = 0;
                ++cu;
            } else {
                ++ctap;
            }
        };
        bf16v8 ba[KS], bb[KS];
        bool ia = false, ib = false;
        if (lu < u1) { ia = load_tap(lmm, lt, ltap, ba); advance(); }
#pragma unroll 1
        while (cu < u1) {
            if (lu < u1) { ib = load_tap(lmm, lt, ltap, bb); advance(); }
            compute(ia, ba);
            if (cu >= u1) break;
            if (lu < u1) { ia = load_tap(lmm, lt, ltap, ba); advance(); }
            compute(ib, bb);
        }
    } else {
        for (int64_t u = u0; u < u1; ++u) {
            int64_t mm;
            int t;
            unit_row(u, mm, t);
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
            for (int tap = 0; tap < 3; ++tap) {
                bf16v8 bf[KS];
                const bool in = load_tap(mm, t, tap, bf);
                mfma_tap(tap, in, bf, acc);
            }
            finish(u, acc);
        }
    }
    flush();
}

// Wide DConv levels (H = C/8 = 24, 48; bf16 mode): gn_gelu_bf16_kernel's output plus the GroupNorm statistics of the
// following 1x1 conv's 2C outputs from its moments (ctx.h conv1x1_moments on the bf16-rounded weights: G = W^T W,
// v = W^T b, u = W^T 1, sum b, sum b^2), so no separate statistics GEMM pass over the 1x1 (forward.cpp dconv):
//   sum_n y_n = sum b + u.x,   sum_n y_n^2 = sum b^2 + 2 v.x + x^T G x,   x = the bf16 GELU(GN(h)) row the GEMM reads.
// One lane per position (row of H channels); groups of L >= 64 positions, so a wave spans at most two groups (its
// sums go to the first active lane's group and, for lanes past a boundary, to the last lane's group).
constexpr int GN_MOM_RMAX = 4;

template <int H, bool MULTI>
__global__ __launch_bounds__(256) void gn_gelu_mom_kernel(const float* __restrict__ h, bf16_t* __restrict__ out,
                                                          int64_t npos, int64_t L, int R_,
                                                          const double* __restrict__ st,
                                                          const float* __restrict__ w, const float* __restrict__ bb,
                                                          const float* __restrict__ gram, double* __restrict__ st_y) {
    __shared__ float wb[2 * H];
    // per (pass, wave) the segmented sums of its <= 2 groups; merged in position order into one atomic pair per
    // group and workgroup (one pair per wave put up to ~260 waves on each group's line: atomic-bound at large L)
    __shared__ double rs[GN_MOM_RMAX * 4 * 2][2];
    __shared__ int64_t rgid[GN_MOM_RMAX * 4 * 2];
    for (int i = threadIdx.x; i < 2 * H; i += 256) wb[i] = i < H ? w[i] : bb[i - H];
    __syncthreads();
    const int wv = threadIdx.x >> 6;
    const int R = MULTI ? R_ : 1;     // (MULTI = false: one pass, no loop - the H = 24, 48 loop bodies spill SGPRs)
#pragma unroll 1
    for (int it = 0; it < R; ++it) {
        const int64_t p0 = ((int64_t)blockIdx.x * R + it) * 256;
        const int64_t p = p0 + threadIdx.x;
        const bool act = p < npos;
        const int64_t pp = act ? p : npos - 1;
        const int64_t g = pp / L;
        float mean, rstd;
        gn_params(st, g, L * H, mean, rstd);
        constexpr int HF = H % 4 == 0 ? H : (H + 7) / 8 * 8;       // f32 input row stride (H = 6: 8, dconv_conv3)
        float x[HF];
        const float4* hr = reinterpret_cast<const float4*>(h + pp * HF);
#pragma unroll
        for (int q = 0; q < HF / 4; ++q) {
            const float4 v = hr[q];
            x[4 * q] = v.x; x[4 * q + 1] = v.y; x[4 * q + 2] = v.z; x[4 * q + 3] = v.w;
        }
        constexpr int OS = H % 8 == 0 ? H : (H + 15) / 16 * 16;     // output row stride (H = 12: rows padded to 16)
        uint32_t pk[OS / 2];
#pragma unroll
        for (int j = 0; j < H; j += 2) {
            pk[j / 2] = pack2bf(gelu_fast((x[j] - mean) * rstd * wb[j] + wb[H + j]),
                                gelu_fast((x[j + 1] - mean) * rstd * wb[j + 1] + wb[H + j + 1]));
            x[j] = __uint_as_float(pk[j / 2] << 16);                 // the bf16 values the 1x1 GEMM multiplies
            x[j + 1] = __uint_as_float(pk[j / 2] & 0xFFFF0000u);
        }
#pragma unroll
        for (int j = H / 2; j < OS / 2; ++j) pk[j] = 0u;
        if (act) {
            uint4* o = reinterpret_cast<uint4*>(out + pp * OS);
#pragma unroll
            for (int q = 0; q < OS / 8; ++q) o[q] = make_uint4(pk[4 * q], pk[4 * q + 1], pk[4 * q + 2], pk[4 * q + 3]);
        }
        // the moments are wave-uniform: scalar loads, one G row per step (the pointer is made opaque per row, so the
        // compiler cannot hoist all H*H loads to the front, which needed ~2300 registers and spilled)
        typedef __attribute__((address_space(4))) const float cfloat;    // constant address space: scalar loads
        float qf = 0.f, lv = 0.f, lw = 0.f;
#pragma unroll
        for (int j = 0; j < H; ++j) {
            cfloat* gr = (cfloat*)(gram + j * H);
            asm volatile("" : "+s"(gr), "+v"(qf));              // row j's loads after row j-1's products
            float t4[4] = {0.f, 0.f, 0.f, 0.f};                 // 4 independent chains (the FMA latency, not issue)
#pragma unroll
            for (int k0 = 0; k0 < H; k0 += 24) {               // (at most 24 row values in SGPRs at a time)
                cfloat* gk = gr + k0;
                if (k0 > 0) asm volatile("" : "+s"(gk), "+v"(t4[0]));
#pragma unroll
                for (int k = 0; k < (H - k0 < 24 ? H - k0 : 24); ++k) t4[k & 3] = fmaf(gk[k], x[k0 + k], t4[k & 3]);
            }
            qf = fmaf(x[j], (t4[0] + t4[1]) + (t4[2] + t4[3]), qf);
            lv = fmaf(gr[H * (H - j) + j], x[j], lv);            // gram[H*H + j]      = (W^T b)_j
            lw = fmaf(gr[H * (H - j) + H + j], x[j], lw);        // gram[H*H + H + j]  = (W^T 1)_j
        }
        cfloat* gt = (cfloat*)(gram + H * H + 2 * H);
        const float sb = gt[0], sb2 = gt[1];
        const double s1 = act ? (double)(sb + lw) : 0.0;
        const double s2 = act ? (double)(sb2 + (2.f * lv + qf)) : 0.0;
        // segmented wave sums: group gA of the first lane, gB of the last active lane (gA <= g <= gB, gB <= gA + 1)
        const int64_t gA = __builtin_amdgcn_readfirstlane((int)g);
        const int64_t last = p0 + wv * 64 + 63;
        const int64_t gB = (last < npos ? last : npos - 1) / L;
        const bool inA = g == gA;
        const double a1 = wave_sum_d(inA ? s1 : 0.0), a2 = wave_sum_d(inA ? s2 : 0.0);
        double b1 = 0.0, b2 = 0.0;
        if (gB != gA) {
            b1 = wave_sum_d(inA ? 0.0 : s1);
            b2 = wave_sum_d(inA ? 0.0 : s2);
        }
        if ((threadIdx.x & 63) == 0) {
            const int e = (it * 4 + wv) * 2;
            rgid[e] = gA; rs[e][0] = a1; rs[e][1] = a2;
            rgid[e + 1] = gB != gA ? gB : -1; rs[e + 1][0] = b1; rs[e + 1][1] = b2;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {          // entries in position order: groups non-decreasing
        int64_t cg = -1;
        double c1 = 0.0, c2 = 0.0;
        for (int e = 0; e < R * 8; ++e) {
            const int64_t ge = rgid[e];
            if (ge < 0) continue;
            if (ge != cg) {
                if (cg >= 0) {
                    atomicAdd(&st_y[2 * cg], c1);
                    atomicAdd(&st_y[2 * cg + 1], c2);
                }
                cg = ge;
                c1 = c2 = 0.0;
            }
            c1 += rs[e][0];
            c2 += rs[e][1];
        }
        if (cg >= 0) {
            atomicAdd(&st_y[2 * cg], c1);
            atomicAdd(&st_y[2 * cg + 1], c2);
        }
    }
}

// H = 48 with the quadratic form split over the workgroup's 4 waves: a workgroup takes 64 positions, wave w
// writes GELU(GN(h)) of channels [w H/4, (w + 1) H/4) of all 64 (one lane per position) and its bf16-rounded values
// into an LDS row per position, then takes G rows [w H/4, (w + 1) H/4) (scalar loads, as above) against the whole row;
// wave 0 adds the 4 partial forms.  4x the waves of gn_gelu_mom_kernel and a quarter of its serial G-row chain per
// wave: level 3 has only 66 k / 132 k positions, so the one-wave-per-64-positions form left the CUs idle (fenc3
// 0.104 -> 0.075 ms, tenc3 0.103 -> 0.051 for two launches; at H = 24 the split measured slower and is not used).
template <int H>
__global__ __launch_bounds__(256) void gn_gelu_mom_split_kernel(const float* __restrict__ h, bf16_t* __restrict__ out,
                                                                int64_t npos, int64_t L,
                                                                const double* __restrict__ st,
                                                                const float* __restrict__ w,
                                                                const float* __restrict__ bb,
                                                                const float* __restrict__ gram,
                                                                double* __restrict__ st_y) {
    constexpr int QJ = H / 4;
    static_assert(QJ % 2 == 0, "channel pairs");
    __shared__ float wb[2 * H];
    __shared__ float xs[64][H + 1];          // (odd pitch: the row reads of 64 lanes hit distinct banks)
    __shared__ float red[4][64][3];
    for (int i = threadIdx.x; i < 2 * H; i += 256) wb[i] = i < H ? w[i] : bb[i - H];
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t p = (int64_t)blockIdx.x * 64 + lane;
    const bool act = p < npos;
    const int64_t pp = act ? p : npos - 1;
    const int64_t g = pp / L;
    float mean, rstd;
    gn_params(st, g, L * H, mean, rstd);
    {
        const int c0 = QJ * wv;
        const float2* hr = reinterpret_cast<const float2*>(h + pp * H + c0);
        uint32_t* o = reinterpret_cast<uint32_t*>(out + pp * H + c0);
#pragma unroll
        for (int q = 0; q < QJ / 2; ++q) {
            const float2 v = hr[q];
            const int c = c0 + 2 * q;
            const uint32_t pk = pack2bf(gelu_fast((v.x - mean) * rstd * wb[c] + wb[H + c]),
                                        gelu_fast((v.y - mean) * rstd * wb[c + 1] + wb[H + c + 1]));
            if (act) o[q] = pk;
            xs[lane][c] = __uint_as_float(pk << 16);
            xs[lane][c + 1] = __uint_as_float(pk & 0xFFFF0000u);
        }
    }
    __syncthreads();
    float x[H];
#pragma unroll
    for (int k = 0; k < H; ++k) x[k] = xs[lane][k];
    typedef __attribute__((address_space(4))) const float cfloat;    // constant address space: scalar loads
    float qf = 0.f, lv = 0.f, lw = 0.f;
    const int j0 = __builtin_amdgcn_readfirstlane(QJ * wv);
#pragma unroll
    for (int jj = 0; jj < QJ; ++jj) {
        const int j = j0 + jj;
        cfloat* gr = (cfloat*)(gram + j * H);
        asm volatile("" : "+s"(gr), "+v"(qf));              // row j's loads after row j-1's products
        float t4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k0 = 0; k0 < H; k0 += 24) {
            cfloat* gk = gr + k0;
            if (k0 > 0) asm volatile("" : "+s"(gk), "+v"(t4[0]));
#pragma unroll
            for (int k = 0; k < (H - k0 < 24 ? H - k0 : 24); ++k) t4[k & 3] = fmaf(gk[k], x[k0 + k], t4[k & 3]);
        }
        const float xj = xs[lane][j];
        qf = fmaf(xj, (t4[0] + t4[1]) + (t4[2] + t4[3]), qf);
        lv = fmaf(gr[H * (H - j) + j], xj, lv);             // gram[H*H + j]      = (W^T b)_j
        lw = fmaf(gr[H * (H - j) + H + j], xj, lw);         // gram[H*H + H + j]  = (W^T 1)_j
    }
    red[wv][lane][0] = qf;
    red[wv][lane][1] = lv;
    red[wv][lane][2] = lw;
    __syncthreads();
    if (wv != 0) return;
    qf = (red[0][lane][0] + red[1][lane][0]) + (red[2][lane][0] + red[3][lane][0]);
    lv = (red[0][lane][1] + red[1][lane][1]) + (red[2][lane][1] + red[3][lane][1]);
    lw = (red[0][lane][2] + red[1][lane][2]) + (red[2][lane][2] + red[3][lane][2]);
    cfloat* gt = (cfloat*)(gram + H * H + 2 * H);
    const float sb = gt[0], sb2 = gt[1];
    const double s1 = act ? (double)(sb + lw) : 0.0;
    const double s2 = act ? (double)(sb2 + (2.f * lv + qf)) : 0.0;
    const int64_t gA = __builtin_amdgcn_readfirstlane((int)g);
    const int64_t last = (int64_t)blockIdx.x * 64 + 63;
    const int64_t gB = (last < npos ? last : npos - 1) / L;
    const bool inA = g == gA;
    const double a1 = wave_sum_d(inA ? s1 : 0.0), a2 = wave_sum_d(inA ? s2 : 0.0);
    if (lane == 0) {
        atomicAdd(&st_y[2 * gA], a1);
        atomicAdd(&st_y[2 * gA + 1], a2);
    }
    if (gB != gA) {
        const double b1 = wave_sum_d(inA ? 0.0 : s1), b2 = wave_sum_d(inA ? 0.0 : s2);
        if (lane == 0) {
            atomicAdd(&st_y[2 * gB], b1);
            atomicAdd(&st_y[2 * gB + 1], b2);
        }
    }
}

// ---- launchers.  Each refuses with -1, before any launch, exactly where its predicate does not hold.
static bool dconv_rows_ok(int64_t M) { return M > 0 && M < (1LL << 31); }     // (32-bit row arithmetic in the kernels)

bool gn_gelu_mom_supported(int H, int64_t L) { return L >= 64 && (H == 6 || H == 12 || H == 24 || H == 48); }

int gn_gelu_mom_launch(const DconvDesc& d, hipStream_t s) {
    const int H = d.C / 8;
    if (!gn_gelu_mom_supported(H, d.L) || d.C != 8 * H) return -1;
    const int64_t npos = d.M, L = d.L;
    // 256-position passes per workgroup: as many as keep >= 2048 workgroups (8 per CU), at most GN_MOM_RMAX
    const int64_t passes = (npos + 255) / 256;
    const int R = H <= 12 ? (int)std::max<int64_t>(1, std::min<int64_t>(GN_MOM_RMAX, passes / 2048)) : 1;
    const dim3 grid((unsigned)((passes + R - 1) / R));
    KScope ks(s);
    if (ks.on())
        ks.begin(klabel(H <= 24 ? "gn_gelu_mom_kernel<%d>" : "gn_gelu_mom_split_kernel<%d>", H), 2.0 * npos * (H * H + 2 * H),
                 (double)npos * H * (4 + 2));
    if (H == 6) hipLaunchKernelGGL((gn_gelu_mom_kernel<6, true>), grid, dim3(256), 0, s, d.h, d.hb, npos, L, R, d.st_h, d.g1w, d.g1b, d.gram, d.st_y);
    else if (H == 12) hipLaunchKernelGGL((gn_gelu_mom_kernel<12, true>), grid, dim3(256), 0, s, d.h, d.hb, npos, L, R, d.st_h, d.g1w, d.g1b, d.gram, d.st_y);
    else if (H == 24) hipLaunchKernelGGL((gn_gelu_mom_kernel<24, false>), grid, dim3(256), 0, s, d.h, d.hb, npos, L, R, d.st_h, d.g1w, d.g1b, d.gram, d.st_y);
    else hipLaunchKernelGGL((gn_gelu_mom_split_kernel<48>), dim3((unsigned)((npos + 63) / 64)), dim3(256), 0, s, d.h, d.hb, npos, L, d.st_h, d.g1w, d.g1b, d.gram, d.st_y);
    return (int)hipGetLastError();
}

// Grid of a weights-resident pass: 16-row units dealt to `waves`-wave workgroups, at most per_cu per CU (LDS)
template <typename Args>
struct DcGrid { int C, per_cu, waves; void (*kernel)(const Args); };
template <typename Args, size_t N>
static int dc_launch(const DcGrid<Args> (&table)[N], int C, const Args& a, hipStream_t s) {
    for (const DcGrid<Args>& g : table) {
        if (g.C != C) continue;
        const int64_t units = (a.M + 15) / 16;
        const int64_t blocks = std::min<int64_t>((int64_t)g.per_cu * device_cus(), (units + g.waves - 1) / g.waves);
        hipLaunchKernelGGL(g.kernel, dim3((unsigned)blocks), dim3(64 * g.waves), 0, s, a);
        return (int)hipGetLastError();
    }
    return -1;
}
// conv3 weights in LDS: 6, 10, 36 KB; 110 KB (one 16-wave workgroup per CU)
static const DcGrid<DcConv3> kConv3Grid[] = {{48, 3, 8, dconv_conv3_kernel<48, 8>}, {96, 3, 8, dconv_conv3_kernel<96, 8>},
                                             {192, 2, 8, dconv_conv3_kernel<192, 8>}, {384, 1, 16, dconv_conv3_kernel<384, 16>}};
// 1x1 weights in LDS: 12, 27 (hidden rows padded to 16 channels by gn_gelu_mom), 48, 96 KB; with the rewrite 25, 77 KB
static const DcGrid<DcApply> kApplyGrid[] = {{48, 3, 8, dconv_apply_kernel<48, 8>}, {96, 3, 8, dconv_apply_kernel<96, 8>},
                                             {192, 2, 8, dconv_apply_kernel<192, 8>}, {384, 1, 16, dconv_apply_kernel<384, 16>}};
static const DcGrid<DcApply> kApplyRewriteGrid[] = {{48, 3, 8, dconv_apply_kernel<48, 8, true>},
                                                    {96, 2, 8, dconv_apply_kernel<96, 8, true>}};

bool dconv_conv3_supported(int C, int H, int kp, int64_t L) {
    return (C == 48 || C == 96 || C == 192 || C == 384) && H == C / 8 && kp >= 3 * C && L >= 16;
}

int dconv_conv3_launch(const DconvDesc& d, hipStream_t s) {
    const int C = d.C;
    if (!dconv_conv3_supported(C, C / 8, d.w3_kp, d.L) || !dconv_rows_ok(d.M)) return -1;
    const DcConv3 a = {(const uint16_t*)d.x, d.w3, d.b3, d.h, d.st_h, d.M, d.L, d.w3_kp, d.dil};
    KScope ks(s);
    if (ks.on()) {
        const double H = C / 8;
        ks.begin(klabel("dconv_conv3_kernel<%d>", C), 2.0 * a.M * H * 3 * C, (double)a.M * (C * 2 + H * 4));
    }
    return dc_launch(kConv3Grid, C, a, s);
}

bool dconv_apply_supported(int C, int H, int kp, int64_t M) {
    return (C == 48 || C == 96 || C == 192 || C == 384) && H == C / 8 && kp == 64 && M > 0;
}

int dconv_apply_launch(const DconvDesc& d, hipStream_t s, const DcRewrite* rwd) {
    const int C = d.C;
    const int64_t M = d.M;
    if (!dconv_apply_supported(C, C / 8, d.w1_kp, M)) return -1;
    if (rwd && (!dconv_narrow(C) || rwd->kp < (C + 31) / 32 * 32)) return -1;
    DcApply a;
    a.hb = d.hb; a.w = d.w1; a.bias = d.b1; a.st = d.st_y; a.gn_w = d.g2w; a.gn_b = d.g2b; a.scale = d.scale;
    a.x = (uint16_t*)d.x; a.M = M; a.L = d.L; a.gn_count = d.L * 2 * C; a.kp = d.w1_kp;
    if (rwd) { a.rw = rwd->w; a.rkp = rwd->kp; a.rbias = rwd->bias; a.out = rwd->out; a.c4 = rwd->c4; }
    KScope ks(s);
    if (ks.on()) {
        const double H = C / 8;
        if (rwd)
            ks.begin(klabel("dconv_apply_kernel<%d,rewrite>", C), 2.0 * M * 2 * C * (H + C),
                     (double)M * (H * 2 + 2.0 * C * 2 + (rwd->c4 ? 8 : 0)));
        else
            ks.begin(klabel("dconv_apply_kernel<%d>", C), 2.0 * M * 2 * C * H, (double)M * (H * 2 + 2.0 * C * 2));
    }
    return rwd ? dc_launch(kApplyRewriteGrid, C, a, s) : dc_launch(kApplyGrid, C, a, s);
}

// the plan (kernels.h), by the predicates above at the packed row lengths gemm_kp (ctx.h up_gemm)
DconvPlan dconv_plan(int mode, int C, int64_t nb, int64_t L, bool rewrite_fusable) {
    DconvPlan p = {};
    const int H = C / 8;
    if ((mode != 0 && mode != 1) || !dconv_rows_ok(nb) || !dconv_rows_ok(L)) return p;
    const int64_t M = nb * L;       // (no overflow: both factors below 2^31)
    // (the same channel counts and packed 1x1 in every form of the layer: the apply pass's rule)
    if (!dconv_rows_ok(M) || !dconv_apply_supported(C, H, gemm_kp(H), M)) return p;
    p.ok = true;
    const bool bf = dconv_bf16(mode);
    const bool conv3 = bf && dconv_conv3_supported(C, H, gemm_kp(3 * C), L), mom = bf && gn_gelu_mom_supported(H, L);
    p.valu = dconv_narrow(C) && !(conv3 && mom);
    if (p.valu) return p;
    p.conv3_mfma = conv3;
    p.norm = mom ? DconvPlan::MOM : bf ? DconvPlan::BF16 : DconvPlan::F32;
    p.apply_mfma = bf;
    p.rewrite = rewrite_fusable && bf && dconv_narrow(C);
    return p;
}

}  // namespace athd
