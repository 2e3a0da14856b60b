// Audio front end of the reference's user path (app.py:74-126): "a file of any rate, mono or stereo" -> the 44.1 kHz
// stereo tensor the separator takes, and the dB spectrogram of app.py:74-94.  Stream-only like track.hip: no context,
// no host synchronisation, no device allocation, status-code returns.
//
// Resampler = torchaudio.transforms.Resample(orig, new) with its defaults (sinc_interp_hann, lowpass_filter_width 6,
// rolloff 0.99); the algorithm is stated in include/athd.h.  Of the 2w + o taps of a phase only those inside the Hann
// window's support are non-zero once the table is rounded to fp32 (the others underflow), so the kernel works on the
// band form: per phase i a first tap first[i] and NT coefficients.  The host builds that table in double, rounds it
// once, caches it per (orig, new) pair (in page-locked memory from the pair's first launch on) and copies it into
// the caller's scratch on the stream.
//
// Spectrogram = torch.stft(mean of the channels, n_fft = 2048, hop_length = 512) with torch's defaults (rectangular
// window, center = True, reflect pad 1024, one-sided), 20 log10(|X| + 1e-8), frequency-major (1025, 1 + T / 512).
//
// Evaluation spectrogram = utils.compute_spectrogram (utils.py:30-95) of benchmark.py --plot-spectrograms and
// generate_spectrogram.py: the same framing with a periodic Hann window, |X|^power, 10 log10(max(., 1e-10)) and a floor
// at the array's maximum - top_db, for several signals per call.
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <utility>
#include <vector>

#include "common.h"
#include "prof.h"
#include "kernels.h"

namespace athd {

// ------------------------------------------------------------------------------------------------- resampler
// LDS budget of resample_kernel: the band table (n first taps + n x NTP coefficients) and the input stage.
constexpr size_t RS_TABLE_MAX = 40960;        // bytes; include/athd.h states this bound
constexpr int RS_XS_CAP = 6144;               // floats of staged input per chunk: o J + 2 w <= RS_XS_CAP
constexpr int RS_CHUNK_OUT = 4096;            // outputs per channel a chunk aims at

struct ResPlan {
    int o, n, w, taps;
    int NT, NTP;                              // live taps per phase; row pitch (odd: conflict-free LDS rows)
    int G, J;                                 // groups per work item, groups per chunk (a multiple of G)
    bool ok;                                  // false: the pair is over the stated bound
    std::vector<uint32_t> blob;               // [n] int first | [n][NTP] float coef
    void* pinned = nullptr;                   // blob in page-locked memory (made by the first launch of the pair), so
                                              // that the per-call copy is asynchronous and can be captured in a graph
    size_t bytes() const { return blob.size() * 4; }
};

static std::mutex g_res_mu;

// K[i][k] of include/athd.h in double (torchaudio's operation order), rounded once to fp32
static float res_coef(int i, int k, int o, int n, int w, double base) {
    double t = (-(double)i / (double)n + (double)(k - w) / (double)o) * base;
    t = t < -6.0 ? -6.0 : (t > 6.0 ? 6.0 : t);
    const double c = cos(t * M_PI / 6.0 / 2.0);
    const double window = c * c;
    const double tp = t * M_PI;
    const double s = tp == 0.0 ? 1.0 : sin(tp) / tp;
    return (float)(s * (window * (base / (double)o)));
}

static ResPlan* res_plan(int orig, int nw) {
    static std::map<std::pair<int, int>, std::unique_ptr<ResPlan>> cache;
    std::lock_guard<std::mutex> lock(g_res_mu);
    auto& slot = cache[{orig, nw}];
    if (slot) return slot.get();
    slot.reset(new ResPlan());
    ResPlan& p = *slot;
    const int g = std::gcd(orig, nw);
    p.o = orig / g;
    p.n = nw / g;
    const double base = (double)std::min(p.o, p.n) * 0.99;
    p.w = (int)ceil(6.0 * (double)p.o / base);
    p.taps = 2 * p.w + p.o;
    p.ok = false;
    p.NT = p.NTP = p.G = p.J = 0;
    // |t| < 6 spans 12 o / base taps: reject a hopeless pair before any table work
    const double width = 12.0 * (double)p.o / base + 3.0;
    if ((double)p.n * (width + 1.0) * 4.0 > 2.0 * (double)RS_TABLE_MAX || p.o + 2 * p.w > RS_XS_CAP) return &p;
    std::vector<int> first(p.n);
    std::vector<std::vector<float>> rows(p.n);
    int NT = 1;
    for (int i = 0; i < p.n; ++i) {
        const double centre = (double)p.w + (double)p.o * (double)i / (double)p.n;
        const int lo = std::max(0, (int)floor(centre - 6.0 * (double)p.o / base) - 2);
        const int hi = std::min(p.taps - 1, (int)ceil(centre + 6.0 * (double)p.o / base) + 2);
        int f = -1, l = -1;
        std::vector<float>& r = rows[i];
        r.assign(hi - lo + 1, 0.f);
        for (int k = lo; k <= hi; ++k) {
            r[k - lo] = res_coef(i, k, p.o, p.n, p.w, base);
            if (r[k - lo] != 0.f) { if (f < 0) f = k; l = k; }
        }
        if (f < 0) f = l = lo;
        first[i] = f;
        NT = std::max(NT, l - f + 1);
        r.erase(r.begin(), r.begin() + (f - lo));      // r[0] = K[i][first]
        r.resize(l - f + 1);
    }
    p.NT = NT;
    p.NTP = NT | 1;
    if ((size_t)p.n * (size_t)(p.NTP + 1) * 4 > RS_TABLE_MAX) return &p;
    p.blob.assign((size_t)p.n * (p.NTP + 1), 0u);
    for (int i = 0; i < p.n; ++i) {
        // first + NT <= taps, so that every staged read of a chunk stays inside its o J + 2 w samples
        const int f = std::min(first[i], p.taps - NT);
        const int32_t fi = f;
        std::memcpy(&p.blob[i], &fi, 4);
        for (int t = 0; t < NT; ++t) {
            const int k = f + t - first[i];             // index into rows[i]
            const float c = (k >= 0 && k < (int)rows[i].size()) ? rows[i][k] : 0.f;
            std::memcpy(&p.blob[(size_t)p.n + (size_t)i * p.NTP + t], &c, 4);
        }
    }
    p.G = p.n >= 64 ? 4 : 1;
    int jmax = (RS_XS_CAP - 2 * p.w) / p.o;
    if (jmax < p.G) p.G = 1;
    jmax = jmax / p.G * p.G;
    int j = (RS_CHUNK_OUT + p.n - 1) / p.n;
    j = (j + p.G - 1) / p.G * p.G;
    p.J = std::min(j, jmax);
    p.ok = p.J >= 1;
    return &p;
}

struct ResDesc {
    const float* in;
    float* out;
    const int* first;
    const float* coef;
    int64_t L, out_len, fs, cs, groups;       // groups = ceil(out_len / n)
    int o, n, w, NT, NTP, J, R, in_ch, out_ch;
};

// One workgroup owns R consecutive chunks of J whole groups of one input channel.  Per chunk it stages the
// o J + 2 w input samples xpad[j0 o ..] (zero outside the signal: both edges go through the index guard, there is
// no separate edge path) next to the band table in LDS.  A work item is (G consecutive groups, phase i): lanes run
// over consecutive phases, so the stores of one group are consecutive outputs, and a coefficient read serves G
// outputs.  fp32 FMAs in ascending tap order from 0.0f: the result does not depend on the launch geometry.
template <int G>
__global__ __launch_bounds__(256) void resample_kernel(const ResDesc d) {
    extern __shared__ float4 rs_smem[];
    float* tb = (float*)rs_smem;                          // [n][NTP]
    int* fi = (int*)(tb + (size_t)d.n * d.NTP);           // [n]
    float* xs = (float*)(fi + d.n);                       // [o J + 2 w]
    const int tid = threadIdx.x;
    const int c = blockIdx.y;
    for (int e = tid; e < d.n * d.NTP; e += 256) tb[e] = d.coef[e];
    for (int e = tid; e < d.n; e += 256) fi[e] = d.first[e];
    const int S = d.o * d.J + 2 * d.w;
    const int items = (d.J / G) * d.n;
    const float* in = d.in + (int64_t)c * d.cs;
    for (int r = 0; r < d.R; ++r) {
        const int64_t j0 = ((int64_t)blockIdx.x * d.R + r) * d.J;
        if (j0 >= d.groups) break;
        __syncthreads();
        const int64_t base = j0 * d.o - d.w;
        for (int m = tid; m < S; m += 256) {
            const int64_t idx = base + m;
            xs[m] = (idx >= 0 && idx < d.L) ? in[idx * d.fs] : 0.f;
        }
        __syncthreads();
        for (int e = tid; e < items; e += 256) {
            const int jq = e / d.n, i = e - jq * d.n;
            const float* cp = tb + i * d.NTP;
            const float* xp = xs + jq * G * d.o + fi[i];
            float acc[G];
#pragma unroll
            for (int g = 0; g < G; ++g) acc[g] = 0.f;
            for (int t = 0; t < d.NT; ++t) {
                const float cf = cp[t];
#pragma unroll
                for (int g = 0; g < G; ++g) acc[g] = fmaf(xp[g * d.o + t], cf, acc[g]);
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int64_t p = (j0 + jq * G + g) * d.n + i;
                if (p < d.out_len) {
                    if (d.in_ch == d.out_ch) {
                        d.out[(int64_t)c * d.out_len + p] = acc[g];
                    } else {                              // mono in: the same value into every output channel
                        for (int oc = 0; oc < d.out_ch; ++oc) d.out[(int64_t)oc * d.out_len + p] = acc[g];
                    }
                }
            }
        }
    }
}

// orig == new: de-interleave / duplicate only
__global__ __launch_bounds__(256) void deinterleave_kernel(const float* __restrict__ in, int64_t L, int64_t fs,
                                                           int64_t cs, int in_ch, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= L) return;
    const int oc = blockIdx.y;
    out[(int64_t)oc * L + t] = in[t * fs + (in_ch == 1 ? 0 : oc) * cs];
}

int64_t resample_length(int64_t length, int orig, int nw) {
    if (length <= 0 || orig <= 0 || nw <= 0) return 0;
    const int g = std::gcd(orig, nw);
    const int64_t o = orig / g, n = nw / g;
    if (length > INT64_MAX / n - 1) return 0;
    return (n * length + o - 1) / o;
}

size_t resample_scratch_bytes(int orig, int nw) {
    if (orig <= 0 || nw <= 0) return 0;
    if (orig == nw) return 16;                             // unused by the identity pass; non-zero = supported
    const ResPlan* p = res_plan(orig, nw);
    return p->ok ? p->bytes() : 0;
}

// -1: bad argument or unsupported pair, -5: scratch too small, > 0: HIP error
int resample_launch(const float* in, int64_t L, int in_ch, int64_t fs, int64_t cs, int orig, int nw, float* out,
                    int out_ch, void* scratch, size_t scratch_bytes, hipStream_t s) {
    if (!in || !out || L <= 0 || orig <= 0 || nw <= 0 || in_ch <= 0 || out_ch <= 0 || out_ch > 65535) return -1;
    if (out_ch != in_ch && in_ch != 1) return -1;
    if (fs <= 0 || cs < 0 || (in_ch > 1 && cs == 0)) return -1;
    const int64_t out_len = resample_length(L, orig, nw);
    if (out_len <= 0) return -1;
    KScope ks(s);
    if (orig == nw) {
        if (ks.on()) ks.begin("deinterleave_kernel", 0.0, (double)L * 4 * (in_ch + out_ch));
        hipLaunchKernelGGL(deinterleave_kernel, dim3((unsigned)((L + 255) / 256), (unsigned)out_ch), dim3(256), 0, s,
                           in, L, fs, cs, in_ch, out);
        return (int)hipGetLastError();
    }
    ResPlan* p = res_plan(orig, nw);
    if (!p->ok) return -1;
    if (!scratch || scratch_bytes < p->bytes()) return -5;
    {
        std::lock_guard<std::mutex> lock(g_res_mu);
        if (!p->pinned) {
            void* h = nullptr;
            HIP_CHECK_RET(hipHostMalloc(&h, p->bytes(), hipHostMallocDefault));
            std::memcpy(h, p->blob.data(), p->bytes());
            p->pinned = h;
        }
    }
    HIP_CHECK_RET(hipMemcpyAsync(scratch, p->pinned, p->bytes(), hipMemcpyHostToDevice, s));
    ResDesc d;
    d.in = in;
    d.out = out;
    d.first = (const int*)scratch;
    d.coef = (const float*)scratch + p->n;
    d.L = L;
    d.out_len = out_len;
    d.fs = fs;
    d.cs = cs;
    d.groups = (out_len + p->n - 1) / p->n;
    d.o = p->o;
    d.n = p->n;
    d.w = p->w;
    d.NT = p->NT;
    d.NTP = p->NTP;
    d.J = p->J;
    d.in_ch = in_ch;
    d.out_ch = out_ch;
    const int64_t chunks = (d.groups + d.J - 1) / d.J;
    d.R = (int)std::min<int64_t>(8, std::max<int64_t>(1, chunks / 1024));
    const int64_t gx = (chunks + d.R - 1) / d.R;
    if (gx > 0x7fffffff) return -1;
    const size_t lds = p->bytes() + (size_t)(d.o * d.J + 2 * d.w) * 4;
    // HBM-bound: every input sample read and every output sample written once (the table stays in L2)
    if (ks.on()) ks.begin("resample_kernel", 2.0 * d.NT * out_len * in_ch, ((double)L * in_ch + (double)out_len * out_ch) * 4);
    const dim3 grid((unsigned)gx, (unsigned)in_ch);
    if (p->G == 4)
        hipLaunchKernelGGL(resample_kernel<4>, grid, dim3(256), lds, s, d);
    else
        hipLaunchKernelGGL(resample_kernel<1>, grid, dim3(256), lds, s, d);
    return (int)hipGetLastError();
}

// ----------------------------------------------------------------------------------------------- spectrogram
constexpr int SP_NFFT = 2048, SP_HOP = 512, SP_M = 1024, SP_BINS = 1025;
constexpr int SP_FB = 8;                      // consecutive frames per workgroup: 32-byte runs of the (bin, frame) store
constexpr int SP_ROW = SP_FB + 1;             // odd pitch of the staged (bin, frame) tile

ATHD_DEV int sp_slot(int i) { return i + (i >> 3); }       // padded LDS slot of complex point i
ATHD_DEV float2 sp_cmul(float2 a, float2 b) {
    return make_float2(fmaf(a.x, b.x, -a.y * b.y), fmaf(a.x, b.y, a.y * b.x));
}
// e^{-2 pi i m / 2048} for m < 2048 from the half table
ATHD_DEV float2 sp_tw(const float2* tw, int m) {
    const float2 v = tw[m & 1023];
    return m < 1024 ? v : make_float2(-v.x, -v.y);
}

// One workgroup = SP_FB consecutive frames.  A real 2048-sample frame is packed as z[m] = x[2m] + i x[2m+1] and goes
// through a 1024-point complex FFT: five radix-4 Stockham passes, one butterfly per thread and pass, exchanged
// through one padded LDS buffer.  Pass Ns (1, 4, .., 256): thread j holds a[j + 256 r], multiplies by
// W1024^(r (j mod Ns) 256 / Ns) and writes DFT output q to (j / Ns) 4 Ns + (j mod Ns) + q Ns.  The real spectrum is
// X[k] = (Z[k] + conj Z[1024-k]) / 2 - i W2048^k (Z[k] - conj Z[1024-k]) / 2, k = 0..1024.  Twiddles: a 1024-entry
// table of W2048^m built per workgroup in double (sincospi), rounded to fp32.  The dB values of the workgroup's
// frames are staged in LDS and stored frequency-major as runs of SP_FB frames per bin.
__global__ __launch_bounds__(256) void spectrogram_db_kernel(const float* __restrict__ wav, int C, int64_t T,
                                                             int64_t F, float* __restrict__ out) {
    __shared__ float2 tw[SP_M];
    __shared__ float2 zb[SP_M + SP_M / 8];
    __shared__ float stage[SP_BINS * SP_ROW];
    const int j = threadIdx.x;
    for (int m = j; m < SP_M; m += 256) {
        double sn, cs;
        sincospi(-(double)m / 1024.0, &sn, &cs);
        tw[m] = make_float2((float)cs, (float)sn);
    }
    __syncthreads();
    const int64_t f0 = (int64_t)blockIdx.x * SP_FB;
    const int nfb = (int)(F - f0 < SP_FB ? F - f0 : SP_FB);
    const float inv_c = 1.0f / (float)C;
    for (int fb = 0; fb < nfb; ++fb) {
        float2 v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float e[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                int64_t p = (f0 + fb) * SP_HOP + 2 * (j + 256 * r) + h - SP_NFFT / 2;
                p = p < 0 ? -p : (p >= T ? 2 * (T - 1) - p : p);           // reflect (T > 1024: one fold)
                float a = wav[p];
                if (C > 1) {
                    for (int ch = 1; ch < C; ++ch) a += wav[(int64_t)ch * T + p];
                    a = C == 2 ? a * 0.5f : a * inv_c;
                }
                e[h] = a;
            }
            v[r] = make_float2(e[0], e[1]);
        }
#pragma unroll
        for (int pass = 0; pass < 5; ++pass) {
            const int Ns = 1 << (2 * pass);
            const int k = j & (Ns - 1);
            if (pass > 0) {
#pragma unroll
                for (int r = 1; r < 4; ++r) v[r] = sp_cmul(v[r], sp_tw(tw, r * k * (512 / Ns)));
            }
            const float2 a0 = make_float2(v[0].x + v[2].x, v[0].y + v[2].y);
            const float2 a1 = make_float2(v[0].x - v[2].x, v[0].y - v[2].y);
            const float2 a2 = make_float2(v[1].x + v[3].x, v[1].y + v[3].y);
            const float2 a3 = make_float2(v[1].y - v[3].y, v[3].x - v[1].x);    // -i (v1 - v3)
            const int j0 = (j / Ns) * 4 * Ns + k;
            zb[sp_slot(j0)] = make_float2(a0.x + a2.x, a0.y + a2.y);
            zb[sp_slot(j0 + Ns)] = make_float2(a1.x + a3.x, a1.y + a3.y);
            zb[sp_slot(j0 + 2 * Ns)] = make_float2(a0.x - a2.x, a0.y - a2.y);
            zb[sp_slot(j0 + 3 * Ns)] = make_float2(a1.x - a3.x, a1.y - a3.y);
            __syncthreads();
            if (pass < 4) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = zb[sp_slot(j + 256 * r)];
                __syncthreads();
            }
        }
        for (int k = j; k <= SP_M; k += 256) {
            const float2 a = zb[sp_slot(k & 1023)];
            const float2 bq = zb[sp_slot((SP_M - k) & 1023)];
            const float2 b = make_float2(bq.x, -bq.y);
            const float2 ev = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y + b.y));
            const float2 od = make_float2(0.5f * (a.y - b.y), -0.5f * (a.x - b.x));    // -i (a - b) / 2
            const float2 wo = sp_cmul(sp_tw(tw, k), od);
            // |X|, the log and the scale in double on the fp32 spectrum, rounded once: at a loud bin (|X| ~ 3 ||frame||,
            // 40 dB) one fp32 ulp of log10f alone is 1.4e-6 ||frame|| of magnitude, more than the whole fp32 FFT's error
            const double re = (double)(ev.x + wo.x), im = (double)(ev.y + wo.y);
            stage[k * SP_ROW + fb] = (float)(20.0 * log10(sqrt(re * re + im * im) + 1e-8));
        }
        __syncthreads();
    }
    for (int e = j; e < SP_BINS * SP_FB; e += 256) {
        const int k = e / SP_FB, fb = e % SP_FB;
        if (fb < nfb) out[(int64_t)k * F + f0 + fb] = stage[k * SP_ROW + fb];
    }
}

int64_t spectrogram_frames(int64_t T) { return T > 0 ? 1 + T / SP_HOP : 0; }

int spectrogram_db_launch(const float* wav, int channels, int64_t T, float* out, hipStream_t s) {
    if (!wav || !out || channels <= 0 || T <= SP_NFFT / 2) return -1;     // torch's reflect pad needs T > 1024
    const int64_t F = spectrogram_frames(T);
    const int64_t gx = (F + SP_FB - 1) / SP_FB;
    if (gx > 0x7fffffff) return -1;
    KScope ks(s);
    // HBM-bound: the track read once (frames overlap 4x, through L2) and the dB array written once
    if (ks.on())
        ks.begin("spectrogram_db_kernel", (double)F * 5.0 * SP_M * 10.0, ((double)T * channels + (double)F * SP_BINS) * 4);
    hipLaunchKernelGGL(spectrogram_db_kernel, dim3((unsigned)gx), dim3(256), 0, s, wav, channels, T, F, out);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------- evaluation spectrogram
// utils.compute_spectrogram (utils.py:30-95): periodic Hann window, |X|^power, 10 log10(max(., 1e-10)) and the floor
// max(dB, max over the signal's array - top_db).  Pass 1 writes the unclamped values and reduces each signal's
// maximum and minimum into its scratch slot; pass 2 clamps in place and writes the range.
//
// Scratch slot of a signal = {enc(max), ~enc(min)}, both zeroed per call and raised with atomicMax on unsigned.
// enc is the order-preserving map of a float onto unsigned (sign bit flipped for non-negative values, every bit for
// negative ones), so the result is the exact fp32 extreme whatever the order of arrival.  0 is below enc of every
// value, -inf included.
ATHD_DEV unsigned ev_enc(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
ATHD_DEV float ev_dec(unsigned e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e); }

constexpr int EV_P2 = 1, EV_DB = 2;           // mode bits of eval_spectrogram_kernel

// spectrogram_db_kernel's frame-group FFT (its body is repeated here so that its machine code stays as it is) with
// the Hann factor applied on load: w[n] = 0.5 - 0.5 cos(2 pi n / 2048) and cos(2 pi n / 2048) = Re W2048^n is tw's
// real part.  Grid (frame group, signal).
__global__ __launch_bounds__(256) void eval_spectrogram_kernel(const float* __restrict__ wav_all, int C, int64_t T,
                                                               int64_t F, int64_t sig_stride, int mode,
                                                               float* __restrict__ out_all,
                                                               unsigned* __restrict__ slots) {
    __shared__ float2 tw[SP_M];
    __shared__ float2 zb[SP_M + SP_M / 8];
    __shared__ float stage[SP_BINS * SP_ROW];
    __shared__ float red[8];
    const int j = threadIdx.x;
    const float* wav = wav_all + (int64_t)blockIdx.y * sig_stride;
    float* out = out_all + (int64_t)blockIdx.y * SP_BINS * F;
    for (int m = j; m < SP_M; m += 256) {
        double sn, cs;
        sincospi(-(double)m / 1024.0, &sn, &cs);
        tw[m] = make_float2((float)cs, (float)sn);
    }
    __syncthreads();
    const int64_t f0 = (int64_t)blockIdx.x * SP_FB;
    const int nfb = (int)(F - f0 < SP_FB ? F - f0 : SP_FB);
    const float inv_c = 1.0f / (float)C;
    for (int fb = 0; fb < nfb; ++fb) {
        float2 v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float e[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int n = 2 * (j + 256 * r) + h;
                int64_t p = (f0 + fb) * SP_HOP + n - SP_NFFT / 2;
                p = p < 0 ? -p : (p >= T ? 2 * (T - 1) - p : p);           // reflect (T > 1024: one fold)
                float a = wav[p];
                if (C > 1) {
                    for (int ch = 1; ch < C; ++ch) a += wav[(int64_t)ch * T + p];
                    a = C == 2 ? a * 0.5f : a * inv_c;
                }
                e[h] = a * (0.5f - 0.5f * sp_tw(tw, n).x);
            }
            v[r] = make_float2(e[0], e[1]);
        }
#pragma unroll
        for (int pass = 0; pass < 5; ++pass) {
            const int Ns = 1 << (2 * pass);
            const int k = j & (Ns - 1);
            if (pass > 0) {
#pragma unroll
                for (int r = 1; r < 4; ++r) v[r] = sp_cmul(v[r], sp_tw(tw, r * k * (512 / Ns)));
            }
            const float2 a0 = make_float2(v[0].x + v[2].x, v[0].y + v[2].y);
            const float2 a1 = make_float2(v[0].x - v[2].x, v[0].y - v[2].y);
            const float2 a2 = make_float2(v[1].x + v[3].x, v[1].y + v[3].y);
            const float2 a3 = make_float2(v[1].y - v[3].y, v[3].x - v[1].x);    // -i (v1 - v3)
            const int j0 = (j / Ns) * 4 * Ns + k;
            zb[sp_slot(j0)] = make_float2(a0.x + a2.x, a0.y + a2.y);
            zb[sp_slot(j0 + Ns)] = make_float2(a1.x + a3.x, a1.y + a3.y);
            zb[sp_slot(j0 + 2 * Ns)] = make_float2(a0.x - a2.x, a0.y - a2.y);
            zb[sp_slot(j0 + 3 * Ns)] = make_float2(a1.x - a3.x, a1.y - a3.y);
            __syncthreads();
            if (pass < 4) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = zb[sp_slot(j + 256 * r)];
                __syncthreads();
            }
        }
        for (int k = j; k <= SP_M; k += 256) {
            const float2 a = zb[sp_slot(k & 1023)];
            const float2 bq = zb[sp_slot((SP_M - k) & 1023)];
            const float2 b = make_float2(bq.x, -bq.y);
            const float2 ev = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y + b.y));
            const float2 od = make_float2(0.5f * (a.y - b.y), -0.5f * (a.x - b.x));    // -i (a - b) / 2
            const float2 wo = sp_cmul(sp_tw(tw, k), od);
            // |X|^power, the log and the factor 10 in double on the fp32 spectrum, rounded once
            const double re = (double)(ev.x + wo.x), im = (double)(ev.y + wo.y);
            const double p2 = re * re + im * im;
            const double S = (mode & EV_P2) ? p2 : sqrt(p2);
            stage[k * SP_ROW + fb] = (float)((mode & EV_DB) ? 10.0 * log10(S > 1e-10 ? S : 1e-10) : S);
        }
        __syncthreads();
    }
    float mx = -INFINITY, mn = INFINITY;
    for (int e = j; e < SP_BINS * SP_FB; e += 256) {
        const int k = e / SP_FB, fb = e % SP_FB;
        if (fb < nfb) {
            const float val = stage[k * SP_ROW + fb];
            out[(int64_t)k * F + f0 + fb] = val;
            mx = fmaxf(mx, val);
            mn = fminf(mn, val);
        }
    }
    // workgroup extremes: wave shuffles, then the 4 waves through LDS; one atomic pair per workgroup
    mx = wave_max(mx);
    mn = -wave_max(-mn);
    if ((j & 63) == 0) {
        red[j >> 6] = mx;
        red[4 + (j >> 6)] = mn;
    }
    __syncthreads();
    if (j == 0) {
        mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        mn = fminf(fminf(red[4], red[5]), fminf(red[6], red[7]));
        atomicMax(slots + 2 * blockIdx.y, ev_enc(mx));
        atomicMax(slots + 2 * blockIdx.y + 1, ~ev_enc(mn));
    }
}

// In-place max(value, M - top_db) over a signal's n values, M and the minimum from its scratch slot; range (may be
// null) = {min, max} of the clamped array (the clamp is monotone, so they follow from the slot).  Grid (chunk,
// signal); a signal's slab starts on a 4-byte boundary only (n is odd), so the scalars before the first 16-byte
// boundary and after the last whole float4 go to the first threads of chunk 0.  clamp == 0: range only.
__global__ __launch_bounds__(256) void db_floor_kernel(float* __restrict__ out_all, int64_t n, float top_db, int clamp,
                                                       const unsigned* __restrict__ slots, float* __restrict__ range) {
    const int sig = blockIdx.y;
    const float M = ev_dec(slots[2 * sig]);
    const float lowest = ev_dec(~slots[2 * sig + 1]);
    const float floor_db = M - top_db;
    if (range && blockIdx.x == 0 && threadIdx.x == 0) {
        range[2 * sig] = clamp ? fmaxf(lowest, floor_db) : lowest;
        range[2 * sig + 1] = M;
    }
    if (!clamp) return;
    float* p = out_all + (int64_t)sig * n;
    int64_t head = (int64_t)(((16 - ((uintptr_t)p & 15)) & 15) >> 2);
    if (head > n) head = n;
    const int64_t nv = (n - head) / 4;
    float4* pv = (float4*)(p + head);
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < nv; g += (int64_t)gridDim.x * 256) {
        float4 q = pv[g];
        q.x = fmaxf(q.x, floor_db);
        q.y = fmaxf(q.y, floor_db);
        q.z = fmaxf(q.z, floor_db);
        q.w = fmaxf(q.w, floor_db);
        pv[g] = q;
    }
    if (blockIdx.x == 0 && threadIdx.x < 8) {                  // at most 3 head and 3 tail scalars
        const int t = threadIdx.x;
        const int64_t idx = t < 4 ? (int64_t)t : head + nv * 4 + (t - 4);
        if (t < 4 ? idx < head : idx < n) p[idx] = fmaxf(p[idx], floor_db);
    }
}

size_t eval_spectrogram_scratch_bytes(int n_signals) { return n_signals > 0 ? (size_t)n_signals * 8 : 0; }

// -1: bad argument, -5: scratch too small, > 0: HIP error
int eval_spectrogram_launch(const float* wav, int n_signals, int channels, int64_t T, int64_t signal_stride,
                            float power, int to_db, float top_db, float* out, float* range, void* scratch,
                            size_t scratch_bytes, hipStream_t s) {
    if (!wav || !out || !scratch || n_signals <= 0 || n_signals > 65535 || channels <= 0 || T <= SP_NFFT / 2) return -1;
    if (!(power == 1.0f || power == 2.0f) || !(top_db >= 0.0f)) return -1;                 // NaN fails the comparison
    if (channels > INT64_MAX / T || signal_stride < (int64_t)channels * T) return -1;
    const int64_t F = spectrogram_frames(T);
    const int64_t gx = (F + SP_FB - 1) / SP_FB;
    if (gx > 0x7fffffff) return -1;
    if (scratch_bytes < eval_spectrogram_scratch_bytes(n_signals)) return -5;
    const int64_t n = F * SP_BINS;
    const int clamp = to_db && !std::isinf(top_db);
    HIP_CHECK_RET(hipMemsetAsync(scratch, 0, eval_spectrogram_scratch_bytes(n_signals), s));
    {
        KScope ks(s);
        // HBM-bound like spectrogram_db_kernel: every signal read once, its array written once
        if (ks.on())
            ks.begin("eval_spectrogram_kernel", (double)n_signals * F * 5.0 * SP_M * 10.0,
                     (double)n_signals * ((double)T * channels + (double)n) * 4);
        hipLaunchKernelGGL(eval_spectrogram_kernel, dim3((unsigned)gx, (unsigned)n_signals), dim3(256), 0, s, wav,
                           channels, T, F, signal_stride, (power == 2.0f ? EV_P2 : 0) | (to_db ? EV_DB : 0), out,
                           (unsigned*)scratch);
        HIP_CHECK_RET(hipGetLastError());
    }
    if (!clamp && !range) return 0;
    KScope ks(s);
    if (ks.on()) ks.begin("db_floor_kernel", 0.0, clamp ? (double)n_signals * 2.0 * n * 4 : (double)n_signals * 16);
    const int64_t chunks = clamp ? std::min<int64_t>(4096, (n / 4 + 1023) / 1024) : 1;      // ~4 float4 per thread
    hipLaunchKernelGGL(db_floor_kernel, dim3((unsigned)std::max<int64_t>(1, chunks), (unsigned)n_signals), dim3(256), 0,
                       s, out, n, top_db, clamp, (const unsigned*)scratch, range);
    return (int)hipGetLastError();
}

}  // namespace athd
