// Launchers for the non-GEMM kernels of the hot path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/athd.h"
#include "gemm.h"

namespace athd {

// demucs pad1d(reflect) plan for HTDemucs._spec: padded index p -> original sample (or 0)
struct PadPlan {
    int64_t L;          // original length
    int64_t left;       // reflect pad applied to the zero-extended signal
    int64_t ext_left;   // zero extension on the left (only when L <= max pad)
    int64_t Lx;         // zero-extended length
};
// the plan of HTDemucs._spec for T samples and Tspec = ceil(T / 1024) kept frames: pad1d(x, (1536, 1536 + 1024 Tspec - T),
// reflect), whose zero extension (inputs no longer than the larger pad) goes to the right first, then to the left
inline PadPlan stft_pad_plan(int64_t T, int64_t Tspec) {
    const int64_t pl = 1536, pr = 1536 + Tspec * 1024 - T, maxpad = pl > pr ? pl : pr;
    const int64_t extra = T <= maxpad ? maxpad - T + 1 : 0, epr = pr < extra ? pr : extra, epl = extra - epr;
    PadPlan pp;
    pp.L = T; pp.left = pl - epl; pp.ext_left = epl; pp.Lx = T + epl + epr;
    return pp;
}

// tconv0.hip: time encoder level-0 conv + GELU on the raw waveform, normalisation on load; w = [48][tap*2 + c] f32
void tconv0_launch(const float* wav, int nb, int64_t T, int64_t Lo, const float* w, const float* bias,
                   const float* tnorm, void* out, int out_bf16, hipStream_t s);

// spectral.hip
// specT [b][t][f][4] (frame-major: level-0 encoder and iSTFT) + per-batch {sum, sumsq} of it into stats (zeroed)
// tw64 != nullptr (f32 parity mode): the FFT runs in double (spectral.hip)
void stft_launch(const float* wav, int nb, int64_t T, const PadPlan& pp, int Tspec, const float2* tw,
                 const double2* tw64, const float* win, float* specT, double* stats, hipStream_t s);
// fo: FO^T [item][t][row][2] (fdec_tail_kernel output); specT as above
// fused: mask + inverse FFT + overlap-add + envelope + time branch (round 1's frame tensor is gone); part:
// istft_ola_part_floats(NI, Tspec) floats of boundary partial sums
void istft_ola_launch(const float* fo, int NI, int Tspec, int P, int64_t T, const float* spec, const float2* tw,
                      const double2* tw64, const float* win, const float* win2, const float* xt2, const float* tnorm,
                      float* out, float* part, hipStream_t s);
int istft_ola_nwg(int Tspec);
int istft_ola_frames(int Tspec);     // frames per workgroup (the last workgroup takes the rest)
inline int64_t istft_ola_part_floats(int64_t NI, int Tspec) { return NI * istft_ola_nwg(Tspec) * 2 * 3 * 1024 * 2; }

// norm.hip
// per-batch {sum, sumsq} (double) of x[b][0..n)
void stats_launch(const float* x, int nb, int64_t n, double* stats, hipStream_t s);
// input normalisation: per batch (mean, 1e-5 + unbiased std) as floats {sub, div} (GemmDesc::a_norm) and (mean, std)
void input_norm_params_launch(const double* stats, int nb, int64_t n, float* mean_inv, float* mean_std,
                              hipStream_t s);
// h[nb][L*H] = GELU(GN(h)) in place (GroupNorm(1,H), stats over L*H per nb)
void gn_gelu_launch(float* h, int nb, int64_t per_batch, int H, const double* stats, const float* w,
                    const float* b, hipStream_t s, bool fast);
// out[nb][per_batch] (bf16) = GELU_fast(GN(h)); per_batch % 8 == 0, H % 8 == 0
void gn_gelu_bf16_launch(const float* h, uint16_t* out, int nb, int64_t per_batch, int H, const double* stats,
                         const float* w, const float* b, hipStream_t s);
void gn_gelu_bf16in_launch(const uint16_t* h, uint16_t* out, int nb, int64_t per_batch, int H, const double* stats,
                           const float* w, const float* b, hipStream_t s);
// x[nb][N][C] = GN(x) in place
void gn_apply_launch(float* x, int nb, int64_t N, int C, const double* stats, const float* w, const float* b,
                     hipStream_t s);
// LayerNorm over C (384 or 512) of rows x[nb*N][C]; optional pending GroupNorm applied first (and written back
// to x), optional positional table pos[N][C] added after the norm, output f32 or bf16 (may alias x if f32).
struct LnDesc {
    float* x = nullptr; int nb = 1; int64_t N = 0; int C = 512;
    const float* w = nullptr; const float* b = nullptr;
    const double* gn_stats = nullptr; const float* gn_w = nullptr; const float* gn_b = nullptr;
    int gn_writeback = 1;    // 0: the pending GroupNorm is applied in registers only (x keeps its raw values; the next
                             // reader of x as a residual applies it again: GemmDesc::res_gn_*, bf16 mode)
    const float* pos = nullptr;
    void* out = nullptr; int out_bf16 = 0;
    // optional second affine of the same normalised rows -> out2 (C = 512, bf16, no pos): the cross layers' two
    // norms of one input (forward.cpp), one read of x instead of two
    const float* w2 = nullptr; const float* b2 = nullptr; void* out2 = nullptr;
};
// the LayerNorm pass can apply a pending GroupNorm in registers only (gn_writeback = 0): the C = 512 row kernel, with
// out2 (if any) fused into the same pass (bf16 output, no positional rows)
inline bool ln_lazy_gn_ok(const LnDesc& d) { return d.C == 512 && (!d.out2 || (d.out_bf16 && !d.pos)); }

void layernorm_launch(const LnDesc& d, hipStream_t s);
// y = bf16(x), n % 8 == 0 (round to nearest even)
void to_bf16_launch(const float* x, uint16_t* y, int64_t n, hipStream_t s);
// a[item] = out_proj(in_v(v_proj(text[item])))   (TextCrossAttention closed form, 384 <- 512), and the prompt's
// out_mlp row biases c0[item] = W0 a + b0, c2[item] = a + b2 (c0 == nullptr: a only)
void text_vec_launch(const float* text, int NI, int P, int text_per_item, const float* maT, const float* ma,
                     const float* mcT, const float* mc, const float* b2, float* a, float* c0, float* c2, hipStream_t s);
// decoder merge: out[item][ho][w][c] = resize_H(act(GN(src)))[ho][w][c] + 0.1 * resize_H(skip[item/P][..][c])
struct MergeDesc {
    const void* src = nullptr; int src_bf16 = 0; int H_src = 0;   // logical ConvT output rows
    int kept = 0;                                // src holds only rows 4d+1, 4d+2 as slots 2d, 2d+1
    int C = 0;                                   // channels of src and out
    const double* stats = nullptr; int64_t gn_count = 0; const float* gn_w = nullptr; const float* gn_b = nullptr;
    const void* skip = nullptr; int skip_bf16 = 0; int H_skip = 0; int C_skip = 0; int P = 1;
    void* out = nullptr; int out_bf16 = 0; int H_out = 0; int W = 1; int NI = 1;
    const float* proj_w = nullptr; const float* proj_b = nullptr;   // optional 1x1 C(=4) -> 2 projection
    int fast_gelu = 0;                            // bf16 mode: branch-free erf
};
int dec_merge_launch(const MergeDesc& d, hipStream_t s);   // -1: P > 256 or NI % P != 0
// positional tables of the cross-transformer (computed on device with the fp32 op order of demucs)
void pos2d_launch(float* out, int Fr, int T1, int C, hipStream_t s);   // out[(f*T1+t)][C]
void pos1d_launch(float* out, int T2, int C, hipStream_t s);           // out[t][C]
// fdec_lr.hip: FreqDecoder level 1 from the 32-row level-0 output (re-associated ConvT; see fdec_lr.hip).
// Z [NI][Hs][W][8*Co] = W_k S[j] per tap k; Zs [NI/P][Hk][W][8*Co] = W_k skip3[m]; skip [NI/P][H_skip][W][C_skip].
// per output-row step v of the level-1 low-rank decoder (fdec_lr.hip): the resize lerps of the Z rows (Hs -> Hd), the
// skip-projection rows (Hk -> Hd) and, for row dd = v - 1, the skip rows (H_skip -> Hd); flags: bit 0 / 1 / 2 = the
// z / k / j rows differ from step v - 1 (always set at v = 0)
struct LrStep {
    float lz, lk, lj;
    uint32_t zk;        // i0z | i1z << 8 | i0k << 16 | i1k << 24
    uint32_t jj;        // i0j | i1j << 16
    uint32_t flags;
    uint32_t pad[2];
};
struct LowRankDesc {
    const LrStep* steps = nullptr;                // Hd + 1 entries (fdec_lr_steps_launch)
    const void* Z = nullptr; const void* Zs = nullptr; int z_bf16 = 0;
    int z_taps = 8;                               // Z rows: [w][8 taps][Co], or 4 = taps 0, 3, 4, 7 as [w][Co / 16][4][16]
                                                  // (merge pass only; written by fdec1_gram_kernel)
    int Hs = 32, Hk = 8, Hd = 0, W = 0, Co = 0, P = 1, NI = 0;
    const float* bias = nullptr;                  // ConvT bias [Co]
    double* stats = nullptr;                      // per item {sum, sumsq} over the 4*Hd ConvT rows
    const float* gn_w = nullptr; const float* gn_b = nullptr; int fast_gelu = 0;
    const void* skip = nullptr; int skip_bf16 = 0; int H_skip = 0; int C_skip = 0;
    void* out = nullptr; int out_bf16 = 0;        // [NI][Hd][W][Co]
    // fused passes (fdec1f.hip): the GEMM operands of Z instead of Z itself
    const void* S = nullptr;                      // bf16 [NI][Hs][W][Ci]
    const void* Wt = nullptr; int w_ld = 0;       // bf16 tap weights [8 Co][w_ld] (row k Co + c)
    int Ci = 0;
    void* z4 = nullptr;                           // fdec1_gram_kernel also writes the merge pass's 4-tap Z here (bf16)
};
int fdec_lr_steps_launch(LrStep* steps, int Hd, int Hs, int Hk, int H_skip, hipStream_t s);
int fdec_lr_stats_launch(const LowRankDesc& d, hipStream_t s);
int fdec_lr_merge_launch(const LowRankDesc& d, hipStream_t s);
// fdec1f.hip: the statistics pass as Gram matrices of Z tiles computed in LDS (bf16 mode, Co = 96, Ci = 192, Hs = 32,
// Hk = 8, Hd > 32); gram: fdec1_gram_floats(NI, W) floats, gq: fdec1_gram_q_doubles() doubles of workspace
bool fdec1_gram_supported(const LowRankDesc& d);
int64_t fdec1_gram_floats(int64_t NI, int W);
int64_t fdec1_gram_q_doubles();
int fdec1_gram_launch(const LowRankDesc& d, float* gram, double* gq, hipStream_t s);
// fenc_row.hip: a whole narrow frequency-encoder level (conv + GELU + DConv + rewrite GLU) per (b, f) row, bf16 mode
constexpr int FR_MT_MAX = 17;        // T <= 272 positions (16-position tiles)
struct FencRowDesc {
    const void* in = nullptr;          // level 0: specT f32 [B][T][Fin][4]; level 1: bf16 [B][Fin][T][Cin]
    const float* a_norm = nullptr;     // level 0: per batch {sub, div}
    int B = 0, Fin = 0, Fout = 0, T = 0;
    const uint16_t* wc = nullptr; int wc_ld = 0; const float* bc = nullptr;        // conv [C][8 Cin]
    const uint16_t* w3[2] = {nullptr, nullptr}; int w3_ld = 0;                    // conv3 [16][3C] (rows >= C/8 zero)
    const float* b3[2] = {nullptr, nullptr};
    const float* g1w[2] = {nullptr, nullptr}; const float* g1b[2] = {nullptr, nullptr};
    const uint16_t* w1[2] = {nullptr, nullptr}; int w1_ld = 0;                    // 1x1 [2C][C/8] GLU-interleaved
    const float* b1[2] = {nullptr, nullptr};
    const float* g2w[2] = {nullptr, nullptr}; const float* g2b[2] = {nullptr, nullptr};   // packed order
    const float* gram[2] = {nullptr, nullptr};    // 1x1 moments (pack.h conv1x1_moments, bf16-rounded weights)
    const float* scale[2] = {nullptr, nullptr};
    const uint16_t* wr = nullptr; int wr_ld = 0; const float* br = nullptr;      // rewrite [2C][C] GLU-interleaved
    const float* row_add = nullptr;    // level 0: freq embedding [Fout][C]
    uint16_t* out = nullptr;           // [B][Fout][T][C] bf16
    uint16_t* out4 = nullptr;          // level 0 (optional): channels 0..3 of out, [B][Fout][T][4] (decoder skip copy)
};
bool fenc_row_supported(int cin, int c, int T);
int fenc_row_launch(const FencRowDesc& d, int cin, int c, hipStream_t s);
// dec_last.hip: last decoder level (ConvT 48 -> 4 + resize + 0.1 skip + 1x1 projection to 2, folded) of either branch.
//   freq: in [NI][H][W][48] -> out FO^T [NI][W][H][2] (H = W = Tspec); fold = [Am | A0 | Ap] (3 x [2][48]), P b + pb (2),
//         0.1 P (8); skip [NI/P][H_skip][W][C_skip] (channels 0..3 used)
//   time: in [NI][H][48] (H = Lin) -> out xt2 [NI][T][2] = time_out(...) incl. bias; fold = Q_k (8 x [2][48]), P b (2),
//         tb (2), 0.1 P (8); skip [NI/P][H_skip][C_skip]
struct DecLastDesc {
    const void* in = nullptr; int in_bf16 = 0;
    int NI = 0, P = 1, H = 0, W = 1;
    int64_t T = 0;
    const float* fold = nullptr;
    const void* skip = nullptr; int skip_bf16 = 0; int H_skip = 0; int C_skip = 0;
    float* out = nullptr;
    // dec_tail: the level-2 merge (GroupNorm -> GELU -> resize -> + 0.1 resize(skip2[:, :48])) fused in front, so the
    // 48-channel input x is computed from the level-2 ConvT output g instead of read from `in`:
    //   freq: g = kept slots [NI][2H][W][48] (logical rows 4d+1, 4d+2); time: g = [NI][Hg][48] (Hg = 4 L2 rows)
    const void* g = nullptr; int g_bf16 = 0; int Hg = 0;
    const double* stats = nullptr; int64_t gn_count = 0; const float* gn_w = nullptr; const float* gn_b = nullptr;
    int fast_gelu = 0;
    const void* skip2 = nullptr; int skip2_bf16 = 0; int H_skip2 = 0; int C_skip2 = 0;
};
int fdec_last_launch(const DecLastDesc& d, hipStream_t s);
int tdec_last_launch(const DecLastDesc& d, hipStream_t s);
int fdec_tail_launch(const DecLastDesc& d, hipStream_t s);
bool tdec_tail_supported(const DecLastDesc& d);     // 4 H == T and every block's g rows fit its LDS tile
int tdec_tail_launch(const DecLastDesc& d, hipStream_t s);
// convt4.hip: decoder level-2 ConvTranspose (96 -> 48, k8 s4 p2) over rows (b, u, w) of x [nb][H][W][96] bf16, all
// four residues in one pass (bf16 mode).  w: [4 x 48 rows][192] bf16, row rho*48 + co, K = the residue pair's two
// input rows (u-1 | u for rho 0/1, u | u+1 for rho 2/3) x 96 channels; bias [48].  keep = 1: residues 1, 2 stored as
// rows 2t, 2t+1 of out [nb][2H][W][48]; keep = 0: out [nb][4H][W][48].  stats: per item fp64 {sum, sumsq} over all
// four residues (accumulated).
struct ConvT4Desc {
    const uint16_t* x = nullptr;
    const uint16_t* w = nullptr;
    const float* bias = nullptr;
    uint16_t* out = nullptr;
    double* stats = nullptr;
    int nb = 0, H = 0, W = 1, keep = 0;
    uint32_t M = 0;                       // filled by convt4_launch
    FastDivU fd_w, fd_h, fd_hw;           // filled by convt4_launch
};
bool convt4_supported(int cin, int cout, int64_t nb, int64_t H, int64_t W);
int convt4_launch(const ConvT4Desc& d, hipStream_t s);
// ---- DConv: one residual layer of an encoder level, x += scale * GLU(GN(W1 GELU(GN(conv3(x))) + b1)), x [M][C] in
// GroupNorm groups of L rows (M = nb L in the forward; the MFMA conv3 / apply passes also take a short last group).
// What athd_finalize packs per (mode, C) (mode 0 = f32, 1 = bf16), and so what dconv_plan may route to:
inline bool dconv_narrow(int C) { return C == 48 || C == 96; }    // the VALU layer's natural-order f32 weights + moments
inline bool dconv_bf16(int mode) { return mode == 1; }            // the bf16-rounded 1x1 moments (gn_gelu_mom, fenc_row);
                                                                  // narrow: conv3 rows padded to 16, permuted rewrite
// The launches of a level's two layers, decided by the launchers' own predicates before anything runs
struct DconvPlan {
    bool ok;            // false: no route (C, mode, or M = nb L outside (0, 2^31))
    bool valu;          // the whole layer in dconv_small_launch; the fields below unused
    bool conv3_mfma;    // dconv_conv3_launch, else the tiled GEMM
    enum Norm { MOM, BF16, F32 } norm;   // MOM: gn_gelu_mom (1x1 statistics from its moments), else + a statistics GEMM
    bool apply_mfma;    // dconv_apply_launch, else the GEMM with the GN -> GLU -> residual epilogue
    bool rewrite;       // second layer: the level's rewrite fused into the apply pass
};
DconvPlan dconv_plan(int mode, int C, int64_t nb, int64_t L, bool rewrite_fusable);
// One layer's operands for the launchers its plan names (forward_enc.cpp dconv)
struct DconvDesc {
    void* x = nullptr; int x_bf16 = 0;              // [M][C], updated in place
    float* h = nullptr;                             // conv3 output [M][C/8] f32 (MFMA passes, C = 48: rows of 8)
    uint16_t* hb = nullptr;                         // MFMA passes: GELU(GN(h)) bf16 [M][C/8] (C = 48, 96: rows of 16)
    double *st_h = nullptr, *st_y = nullptr;        // per group {sum, sumsq} of h / of the 1x1's 2C outputs
    int64_t M = 0, L = 0; int C = 0, dil = 1;
    const float *w3f = nullptr, *w1f = nullptr;     // VALU layer: f32 conv3 [C/8][tap * C + ci], 1x1 [2C][C/8]
    bool fast = false;                              // VALU layer: the bf16 mode's branch-free GELU / sigmoid
    const uint16_t *w3 = nullptr, *w1 = nullptr;    // MFMA passes: bf16 conv3 [16 n][w3_kp], 1x1 [2C][w1_kp] GLU-interleaved
    int w3_kp = 0, w1_kp = 0;
    const float *b3 = nullptr, *g1w = nullptr, *g1b = nullptr, *scale = nullptr;
    const float *b1 = nullptr, *g2w = nullptr, *g2b = nullptr;   // in the row order of the 1x1 weights in use
    const float* gram = nullptr;                    // pack.h conv1x1_moments of the 1x1 weights in use
};
// dconv_small.hip: the layer as three VALU kernels (C = 48, 96; M = nb L); -2 if the shape is not covered
int dconv_small_launch(const DconvDesc& d, hipStream_t s);
// dconv.hip: the layer as three weights-resident passes (bf16 mode); -1 before any launch unless the predicate holds.
// conv3 + GroupNorm statistics of h; hb = bf16(GELU(GN(h))) + the 1x1's statistics from d.gram (M = nb L); the 1x1
// apply, with rw (C = 48, 96) followed in registers by the level's rewrite out = GLU(Wr x + br) instead of the store to
// x (rw.w: [2C][kp] GLU-interleaved rows in the K order of pack.h dconv_rewrite_perm)
struct DcRewrite {
    const uint16_t* w;
    int kp;
    const float* bias;
    uint16_t* out;     // [M][C] bf16
    uint16_t* c4;      // optional [M][4]
};
bool dconv_conv3_supported(int C, int H, int kp, int64_t L);
bool gn_gelu_mom_supported(int H, int64_t L);
bool dconv_apply_supported(int C, int H, int kp, int64_t M);
int dconv_conv3_launch(const DconvDesc& d, hipStream_t s);
int gn_gelu_mom_launch(const DconvDesc& d, hipStream_t s);
int dconv_apply_launch(const DconvDesc& d, hipStream_t s, const DcRewrite* rw = nullptr);

// track.hip: window overlap-add of test_inference.py:92-141 (mode 0) and benchmark.py:155-204 (mode 1, weighted;
// wsum != nullptr: unnormalised partial span + weight sums), sdr_loss / sisdr_loss (src/loss.py:9-68)
int ola_launch(const float* win, int64_t L, int64_t chunk, int64_t overlap, int S, int64_t k0, int64_t k1, float* out,
               hipStream_t s, int mode = 0, float* wsum = nullptr);
int ola_normalize_launch(float* out, const float* wsum, int rows, int64_t n, hipStream_t s);
int sdr_launch(const float* est, const float* tgt, int64_t rows, int64_t n, double* sums, float* out, hipStream_t s);
int sisdr_launch(const float* est, const float* tgt, int64_t rows, int64_t n, double* scratch, float* out,
                 hipStream_t s);

// loss.hip: the row metrics of src/loss.py ({sdr, sisdr, new_sdr, l1} per row, fixed-order fp64 sums, no atomics) and
// the dataset segments of src/dataloader.py:104-121; -1 = bad argument, otherwise a HIP error
size_t loss_rows_scratch_bytes(int64_t rows, int64_t n);
int loss_rows_launch(const float* est, const float* tgt, int64_t rows, int64_t n, void* scratch, double* out,
                     hipStream_t s);
int gather_segments_launch(const float* stems, int n_src, int64_t length, const int32_t* src, const int64_t* seg,
                           int64_t rows, int64_t seg_samples, float* out, hipStream_t s);
// loss.hip, training ends: the gradient of the combined losses w.r.t. est (per-row coefficients from the sums of
// loss_rows, then one elementwise pass) and the random / augmented segments of src/dataloader.py:86-134
int loss_grad_coef_launch(const float* est, const float* tgt, int64_t rows, int64_t n, void* scratch, double* table,
                          double* coef, hipStream_t s);
int loss_grad_apply_launch(const float* est, const float* tgt, int64_t rows, int64_t n, const double* coef,
                           double w_sdr, double w_si, double w_l1, const float* upstream, float* grad, hipStream_t s);
int gather_train_segments_launch(const float* stems, int n_src, int64_t length, const int32_t* src,
                                 const int64_t* start, const double* gain, const uint8_t* swap, int64_t rows,
                                 int64_t seg_samples, float* out, hipStream_t s);

// audio_io.hip: torchaudio-default resampler (band-table form) and the dB spectrogram of app.py:74-94.
// resample_launch returns -1 (bad argument / unsupported pair), -5 (scratch too small) or a HIP error
int64_t resample_length(int64_t length, int orig, int nw);
size_t resample_scratch_bytes(int orig, int nw);
int resample_launch(const float* in, int64_t L, int in_ch, int64_t fs, int64_t cs, int orig, int nw, float* out,
                    int out_ch, void* scratch, size_t scratch_bytes, hipStream_t s);
int64_t spectrogram_frames(int64_t T);
int spectrogram_db_launch(const float* wav, int channels, int64_t T, float* out, hipStream_t s);
// evaluation spectrograms of utils.py:30-95 (Hann, |X|^power, dB with the top_db floor), n_signals per call;
// eval_spectrogram_launch returns -1 (bad argument), -5 (scratch too small) or a HIP error
size_t eval_spectrogram_scratch_bytes(int n_signals);
int eval_spectrogram_launch(const float* wav, int n_signals, int channels, int64_t T, int64_t signal_stride,
                            float power, int to_db, float top_db, float* out, float* range, void* scratch,
                            size_t scratch_bytes, hipStream_t s);

// embed_compare.hip: row normalisation, cosine-similarity and Euclidean-distance matrices and the intra / inter
// category statistics of embedding_comparison.py (fp64 accumulation, fixed-order reductions, no atomics);
// embed_compare_launch returns -1 (bad argument), -5 (scratch too small) or a HIP error
size_t embed_compare_scratch_bytes(int n, int d);
int embed_compare_launch(const float* emb, int n, int d, int64_t row_stride, const int32_t* category, float* normed,
                         float* sim, float* dist, double* stats, void* scratch, size_t scratch_bytes, hipStream_t s);

// export.hip: the frozen features of athd_encode in the reference's (channel-first) layout, plain copies.
// export_cf: channels [0, Cs) of a channels-last src [nb][rows][C] (f32, or bf16 widened exactly) -> f32 [nb][Cs][rows]
// export_spec: specT [B][Tspec][2048][4] -> z [B][2][2048][Tspec][2] (re, im of the two audio channels)
// export_norm: tnorm_std [B][2] = {mean, std} -> meant [B], stdt [B]
// each returns -1 for a bad argument (nothing launched) or a HIP error
int export_cf_launch(const void* src, int src_bf16, int64_t nb, int64_t rows, int C, int Cs, float* out, hipStream_t s);
int export_spec_launch(const float* specT, int64_t B, int64_t Tspec, float* z, hipStream_t s);
int export_norm_launch(const float* tnorm_std, int64_t B, float* meant, float* stdt, hipStream_t s);

// head_grad.hip: head training's output stage.
// pack_spec: z [B][2][2048][Tspec][2] -> specT [B][Tspec][2048][4], the inverse of export_spec
// head_grad: the adjoint of istft_ola with P = 1 with respect to its logits: g [B][2][T] = dL/dout, fo [B][Tspec][Tspec][2]
// and specT as the forward read them -> gfo [B][Tspec][Tspec][2], every element written; Tspec = ceil(T / 1024) <= 2048
// each returns -1 for a bad argument (nothing launched) or a HIP error
int pack_spec_launch(const float* z, int64_t B, int64_t Tspec, float* specT, hipStream_t s);
int head_grad_launch(const float* g, const float* fo, const float* specT, int64_t B, int Tspec, int64_t T,
                     const float2* tw, const float* win, const float* win2, float* gfo, hipStream_t s);

// head_cond.hip: head training's text-conditioning stage (include/athd.h), all f32.
// x, y, gy [B][384][N]; a [B][384]; w0, w2 [384][384] row-major [out][in]; ws: head_cond_ws_floats(B, N) floats, 16-byte
// aligned (0 = shape out of range: B in [1, 65535], N in [1, HEAD_COND_MAX_N]).  Every output element is written; fixed
// summation order, no atomics.  Each returns -1 for a bad argument (nothing launched) or a HIP error.
constexpr int HEAD_COND_C = 384, HEAD_COND_TN = 64, HEAD_COND_SLICES = 14;
constexpr int64_t HEAD_COND_MAX_N = 1 << 20;
int64_t head_cond_ws_floats(int64_t B, int64_t N);
int head_cond_fwd_launch(const float* x, const float* a, const float* w0, const float* b0, const float* w2,
                         const float* b2, const float* gamma, const float* beta, int64_t B, int64_t N, float* y,
                         hipStream_t s);
int head_cond_bwd_launch(const float* gy, const float* x, const float* a, const float* w0, const float* b0,
                         const float* w2, const float* b2, const float* gamma, int64_t B, int64_t N, float* gw0,
                         float* gb0, float* gw2, float* gb2, float* ggamma, float* gbeta, float* ga, float* ws,
                         hipStream_t s);

// head_dec.hip: one level of head training's decoders (include/athd.h), all f32.  level 0..3 = (Ci, Co) (384, 192),
// (192, 96), (96, 48), (48, 4); x [B][Ci][M][inner], w [Ci][Co][8], skip [B][Co][S][inner] or nullptr with S = 0,
// y, gy [B][Co][Lt][inner], stats [B][2] = {mu, r} (levels 0..2; gamma, beta, stats and their gradients may be nullptr at
// level 3).  ws: head_dec_ws_floats() floats, 16-byte aligned (0 = shape out of range).  Every output element is written;
// fixed summation order, no atomics.  Each returns -1 for a bad argument (nothing launched) or a HIP error.
constexpr int64_t HEAD_DEC_MAX_M = 1 << 20, HEAD_DEC_MAX_INNER = 4096, HEAD_DEC_MAX_LT = 1 << 22;
constexpr int64_t HEAD_DEC_MAX_TOKENS = 1 << 26;        // M inner; Lt inner and S inner up to four times that
int64_t head_dec_ws_floats(int level, int64_t B, int64_t M, int64_t inner, int64_t Lt);
int head_dec_fwd_launch(int level, const float* x, const float* w, const float* bias, const float* gamma,
                        const float* beta, const float* skip, int64_t B, int64_t M, int64_t inner, int64_t S, int64_t Lt,
                        float* y, float* stats, float* ws, hipStream_t s);
int head_dec_bwd_launch(int level, const float* gy, const float* x, const float* w, const float* bias,
                        const float* gamma, const float* beta, const float* stats, int64_t B, int64_t M, int64_t inner,
                        int64_t Lt, float* gx, float* gw, float* gb, float* ggamma, float* gbeta, float* ws,
                        hipStream_t s);

// head_step.hip: head training's update step (include/athd.h `athd_head_step`: global gradient norm, clip, AdamW), all
// f32 storage, fp64 arithmetic.  A tensor is cut into chunks of HEAD_STEP_CHUNK elements, one workgroup each;
// head_step_chunks() is their number (0 = n_tensors outside 1..64, an n < 1 or more than HEAD_STEP_MAX_CHUNKS) and the
// number of doubles `part` holds.  t and hp are host data, copied into the kernel arguments.  Returns 0, -1 for a bad
// argument (nothing launched), or the positive hipError_t of a failed launch.  Every update workgroup adds all partials
// itself, so the work grows with the square of the chunk count: the limit keeps that sum at a few microseconds.
constexpr int64_t HEAD_STEP_CHUNK = 4096, HEAD_STEP_MAX_CHUNKS = 4096;
int64_t head_step_chunks(const athd_step_tensor* t, int n_tensors);
int head_step_launch(const athd_step_tensor* t, int n_tensors, const athd_step_hparams& hp, const float* grad_scale,
                     const float* found_inf, int32_t* step, float* stats, double* part, hipStream_t s);

// head_proj.hip: head training's output projections (include/athd.h `athd_head_proj*`: freq_out / time_out, a 1x1
// convolution 4 -> 2 channels), all f32.  x, gx [B][4][R][S]; y [B][S][R][2]; gy in y's layout or, channel_first,
// [B][2][R][S]; w [2][4], bias [2]; scale nullptr or [B].  part: head_proj_ws_doubles(B, R, S) doubles (0 = shape out of
// range: B in [1, 65535], R in [1, HEAD_PROJ_MAX_R], S in [1, HEAD_PROJ_MAX_S], R S <= HEAD_PROJ_MAX_RS), ten per
// workgroup of the larger of the backward's two grids.  The big tensors are 16-byte aligned.  Every output element is
// written; fixed summation order, no atomics.  Each returns -1 for a bad argument (nothing launched) or a HIP error.
constexpr int64_t HEAD_PROJ_CHUNK = 4096;
constexpr int64_t HEAD_PROJ_MAX_R = 4096, HEAD_PROJ_MAX_S = 1 << 22, HEAD_PROJ_MAX_RS = 1 << 22;
int64_t head_proj_ws_doubles(int64_t B, int64_t R, int64_t S);
int head_proj_fwd_launch(const float* x, const float* w, const float* bias, int64_t B, int64_t R, int64_t S, float* y,
                         hipStream_t s);
int head_proj_bwd_launch(const float* gy, int channel_first, const float* scale, const float* x, const float* w,
                         int64_t B, int64_t R, int64_t S, float* gx, float* gw, float* gb, double* part, hipStream_t s);

// head_proj.hip: the text cross-attention's vector per item (include/athd.h `athd_head_attn_vec*`), all f32 storage,
// sums in double.  text [B][512]; wv [384][512]; w_in [1152][384] (the value third is read); wo [384][384];
// a [B][384]; keep [B][2][384] = {v_proj(text), in_proj_v(..)}.  The forward takes B in [1, 65535], the backward B in
// [1, HEAD_ATTN_MAX_B]: it keeps its two
// (B, 384) intermediates in the dead two thirds of gw_in until its last launch zeroes them.
constexpr int HEAD_ATTN_D = 384, HEAD_ATTN_TEXT = 512;
constexpr int64_t HEAD_ATTN_MAX_B = 384;
int head_attn_vec_fwd_launch(const float* text, const float* wv, const float* bv, const float* w_in, const float* b_in,
                             const float* wo, const float* bo, int64_t B, float* a, float* keep, hipStream_t s);
int head_attn_vec_bwd_launch(const float* ga, const float* text, const float* keep, const float* w_in, const float* wo,
                             int64_t B, float* gwv, float* gbv, float* gw_in, float* gb_in, float* gwo, float* gbo,
                             hipStream_t s);

}  // namespace athd
