/*
 * athd - C ABI of the MI355X-native AudioTextHTDemucs hot path (libathd.so).
 *
 * Replaces, for the per-segment inference path, the reference's Python surface:
 *   AudioTextHTDemucs(htdemucs, clap, tokenizer)          /root/reference/src/models/stem_separation/ATHTDemucs_v2.py:151-188
 *   model.load_state_dict(ckpt["model_state_dict"], strict=False)   test_inference.py:34-35
 *   model.forward(wav, text) -> (B,2,T)                   ATHTDemucs_v2.py:250-326
 * athd_forward* take prompt embeddings (B x 512 or P x 512 fp32, L2-normalised as ClapModel.get_text_features
 * returns them); the CLAP text tower that computes them from token ids (ATHTDemucs_v2.py:238-248) is the
 * athd_text_* section below, with a context of its own.  Only the tokenizer stays with the caller.
 *
 * Conventions: plain pointers and sizes, no torch types.  All device pointers are HIP device memory owned by
 * the caller (wav, text embeddings, output, workspace); the context owns the packed weights.  Every call
 * returns 0 on success or a negative athd_status; the message is in athd_last_error().  Nothing is thrown
 * across the ABI.  Work is enqueued on the caller's stream (a hipStream_t passed as void*, NULL = default
 * stream); athd_forward* do not synchronise the host and create no memory, streams or events (the time branch's
 * stream and the fork/join events are made by athd_finalize), so they can be captured in a graph.  One context
 * per device; calls on one context must be serialised by the caller, even from different streams (the fork/join
 * events are per context).
 */
#ifndef ATHD_H
#define ATHD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct athd_ctx athd_ctx;

enum athd_status {
    ATHD_OK = 0,
    ATHD_EINVAL = -1,      /* bad argument / shape */
    ATHD_EKEY = -2,        /* unknown, missing or mis-shaped weight */
    ATHD_ESTATE = -3,      /* not finalized / already finalized */
    ATHD_EHIP = -4,        /* HIP runtime error */
    ATHD_EWORKSPACE = -5   /* workspace too small */
};

enum athd_dtype { ATHD_F32 = 0, ATHD_BF16 = 1 };

/* ABI version (major*100 + minor). */
int athd_version(void);

/* Create a context on HIP device `device`.  dtype: ATHD_F32 = exact fp32 MFMA everywhere (parity mode),
 * ATHD_BF16 = bf16 MFMA operands with fp32 accumulation/normalisation (throughput mode). */
int athd_create(athd_ctx** out, int device, int dtype);

/* Stage one weight tensor under its reference state-dict key (e.g. "htdemucs.encoder.0.conv.weight",
 * "text_attn.out_mlp.0.weight", "freq_decoder.layers.1.0.weight").  host points to contiguous fp32
 * (src_dtype 0) with the given shape.  Keys outside the hot path (clap.*, htdemucs.decoder.*, ...) are
 * accepted and ignored, mirroring load_state_dict(strict=False). */
int athd_set_weight(athd_ctx* ctx, const char* key, const void* host, const int64_t* shape, int ndim,
                    int src_dtype);

/* Number / names of the weight keys the hot path requires (reference names). */
int athd_num_required_keys(void);
const char* athd_required_key(int i);

/* Validate that every required key is present with the right shape, pack (transpose, tap-major, GLU pair
 * order, ConvTranspose residue split, bf16 conversion) and upload. */
int athd_finalize(athd_ctx* ctx);

/* (segment, prompt) items the decoder processes per chunk (default 64; 1..4096).  The encoder's buffers scale
 * with B and the decoder's with this setting: at B = 64, T = 264600 (6 s), P = 4 the workspace is about 18 GB
 * at 64 items and about 49 GB at 256 (the whole batch in one decode chunk: fewer, larger launches, the bench setting).
 * Takes effect for the next athd_workspace_bytes / athd_forward* calls; the environment variable
 * ATHD_DECODE_ITEMS overrides it. */
int athd_set_decode_items(athd_ctx* ctx, int64_t items);

/* Workspace bytes needed by athd_forward (P = 1) / athd_forward_prompts (P prompts) for B segments of
 * T samples (see athd_set_decode_items for the sizes at the bench configuration). */
size_t athd_workspace_bytes(athd_ctx* ctx, int64_t B, int64_t T, int P);

/* wav: (B,2,T) f32, text_emb: (B,512) f32 -> out: (B,2,T) f32.  == AudioTextHTDemucs.forward(wav, text). */
int athd_forward(athd_ctx* ctx, const float* wav, int64_t B, int64_t T, const float* text_emb, float* out,
                 void* workspace, size_t workspace_bytes, void* stream);

/* Encode once, decode once per prompt (1 <= P <= 256): wav (B,2,T), text_table (P,512) -> out (B,P,2,T); equal to P calls of
 * athd_forward because the encoder and cross-transformer do not see the prompt (ATHTDemucs_v2.py:278-283). */
int athd_forward_prompts(athd_ctx* ctx, const float* wav, int64_t B, int64_t T, const float* text_table, int P,
                         float* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Frozen features for head training: the no_grad half of the forward (ATHTDemucs_v2.py:190-236, 261-279) ----
 * The reference trains only text_attn / freq_decoder / time_decoder / freq_out / time_out; the HTDemucs encoders and
 * the cross-transformer are frozen.  athd_encode runs exactly the encoder and transformer stages of athd_forward (same
 * kernels, stream plan and runtime switches) and then copies what the trainable half reads into caller-owned tensors:
 * float32, contiguous, in the reference's channel-first layout, whatever the context's dtype (bf16 activations are
 * widened, which is exact).  With Ts = ceil(T / 1024), L[0] = T, L[i+1] = ceil(L[i] / 4), F[1..4] = {512, 128, 32, 8}
 * and Ck = {4, 48, 96, 192}:
 *   x_enc  (B, 384, 8, Ts), xt_enc (B, 384, L[4])    the transformer's outputs after the channel down-projection
 *   skip_f[i] (B, Ck[i], F[i+1], Ts)                 channels [0, Ck[i]) of the reference's saved[i]
 *   skip_t[i] (B, Ck[i], L[i+1])                     channels [0, Ck[i]) of saved_t[i]
 *   z      (B, 2, 2048, Ts, 2)                       torch.view_as_real(z[:, :2]): re, im interleaved
 *   meant, stdt (B)                                  wav.mean / wav.std (unbiased, torch.std) over (C, T)
 * Only the first Ck[i] channels of a skip are exported because the decoders read nothing else: they truncate every skip
 * to their own level's channel count (ATHTDemucs_v2.py:99-100, 134-135).
 * Every member of `out` is a device pointer; a null one is ATHD_EINVAL.  ATHD_ESTATE before athd_finalize,
 * ATHD_EWORKSPACE below athd_encode_workspace_bytes (today equal to athd_workspace_bytes(ctx, B, T, 1)).  Like
 * athd_forward the call does not synchronise the host and creates no HIP objects, so it can be graph-captured from the
 * first call; the time branch runs on the context's second stream and is joined before the copies, which run on the
 * caller's stream: every exported tensor is complete in the order of that stream. */
typedef struct athd_features {
    float* x_enc;
    float* xt_enc;
    float* skip_f[4];
    float* skip_t[4];
    float* z;
    float* meant;
    float* stdt;
} athd_features;
size_t athd_encode_workspace_bytes(athd_ctx* ctx, int64_t B, int64_t T);
int athd_encode(athd_ctx* ctx, const float* wav, int64_t B, int64_t T, const athd_features* out, void* workspace,
                size_t workspace_bytes, void* stream);

/* ---- Head training's output stage: the mask, the inverse STFT and the time branch's denormalisation
 * (ATHTDemucs_v2.py:303-324) in both directions ----
 * What the trainable half ends with, fed by athd_encode's z, meant and stdt and by the head's two 1x1 output
 * convolutions.  With Ts = ceil(T / 1024), per item and audio channel c:
 *   mask_c = sigmoid(resize(logits_c))     the logits' Ts rows stretched linearly to 2048 bins (align_corners = False)
 *   X_c    = (m_c mask_c) z_c / (m_c + 1e-8),  (m_0, m_1) = (Re z_0, Im z_0) as the reference has it
 *   out    = istft(X) + (xt stdt + meant)      demucs' _ispec: Hann 4096 / 1024, normalized, cropped to T
 * The three entries take the context for its FFT and window tables and its dtype; they read no weight.  All enqueue on
 * the caller's stream, do not synchronise the host and create no HIP object, so they can be graph-captured from the
 * first call.  ATHD_ESTATE before athd_finalize; ATHD_EINVAL for a null pointer, B outside [1, 65535], T < 1 or more
 * than 2048 frames (T > 2097152, 47 s: the resize would turn into a downsample whose adjoint is not implemented);
 * ATHD_EWORKSPACE below athd_head_output_workspace_bytes (which is 0 for shapes out of range).  Arguments are checked
 * in that order before anything is read or written.
 *
 * athd_pack_spectrum: z (B, 2, 2048, Ts, 2) as athd_encode exports it -> spec (B, Ts, 2048, 4) = {Re L, Im L, Re R,
 * Im R}, frame-major: the layout the two entries below read, a plain copy (bit-exact).  Once per batch.
 *
 * athd_head_output: logits (B, Ts, Ts, 2) = [frame][row][channel], xt (B, T, 2), tnorm (B, 2) = {meant, stdt} ->
 * out (B, 2, T).  This is the inference path's own fused kernel with one prompt per segment (no frame tensor in
 * memory), bit-identical to athd_forward's last stage on the same buffers: an ATHD_F32 context runs the FFT in double
 * with IEEE exp and divisions, an ATHD_BF16 context the float FFT with v_exp / v_rcp.  ws: device, 16-byte aligned,
 * not initialised by the caller.
 *
 * athd_head_output_backward: grad_out (B, 2, T) = dL/dout, channel-first and contiguous (what athd_loss_grad_apply
 * writes), with the logits and spec of the forward -> grad_logits (B, Ts, Ts, 2) = dL/dlogits.  The adjoint of the
 * inverse STFT is an STFT of grad_out / envelope; the mask is recomputed from the logits (nothing is saved by the
 * forward).  One kernel, f32 arithmetic with IEEE exp and divisions in both dtype modes; every element of grad_logits
 * is written exactly once, sums run in a fixed order and there are no atomics: the same bits on every run and under
 * graph replay.  dL/dxt needs no kernel: it is grad_out * stdt, transposed. */
int athd_pack_spectrum(athd_ctx* ctx, const float* z, int64_t B, int64_t Ts, float* spec, void* stream);
size_t athd_head_output_workspace_bytes(int64_t B, int64_t T);
int athd_head_output(athd_ctx* ctx, const float* logits, const float* spec, const float* xt, const float* tnorm,
                     int64_t B, int64_t T, float* out, void* ws, size_t ws_bytes, void* stream);
int athd_head_output_backward(athd_ctx* ctx, const float* grad_out, const float* logits, const float* spec, int64_t B,
                              int64_t T, float* grad_logits, void* stream);

/* ---- Head training's text-conditioning stage (ATHTDemucs_v2.py:21-58) in both directions, from raw f32 weights ----
 * The cross-attention has ONE key, so its output is one vector per item, a (B, 384) = out_proj(in_proj_v(v_proj(text))),
 * which the caller computes (three tiny matrix-vector products, differentiable where it computes them).  The rest of the
 * stage, per item b on its (384, N) channel-first slab X exactly as athd_encode exports x_enc / xt_enc (the frequency
 * branch's (B, 384, 8, Ts) is the same memory as (B, 384, 8 Ts)), columns = tokens:
 *   U = X + a_b;  V = U + W2 gelu_erf(W0 U + b0) + b2;  Y = gamma (V - mu) r + beta, (mu, r) the mean and
 *   1 / sqrt(var + 1e-5) of each column over the 384 channels (out_mlp.0 / out_mlp.2 / norm_out; weights (384, 384)
 *   row-major [out][in] as torch keeps them).  y (B, 384, N), channel-first like x.
 * All pointers are device f32; the weights are read as they are at the time the kernels run (nothing is packed, nothing
 * is cached across calls: a training step may change them between calls).  The context is taken for its device only: the
 * arithmetic is f32 (v_mfma_f32_16x16x4_f32 and IEEE erf / exp / sqrt / division) in both dtype modes, bit-identical
 * between them.
 *
 * athd_head_cond_backward: grad_y (B, 384, N) = dL/dy with the x, a and weights of the forward -> grad_w0, grad_w2
 * (384, 384), grad_b0, grad_b2, grad_gamma, grad_beta (384) and grad_a (B, 384) = dL/da; x gets no gradient (it comes
 * from the frozen half).  The forward is recomputed from x; nothing is saved between the two calls.  Every output element
 * is written, none is accumulated into and none is read.  Sums over tokens run in a fixed order (per 64-token tile, then
 * tiles in order per item, then items in order; the weight gradients as a split-K GEMM over a fixed 14 slices summed in
 * slice order) and there are no atomics: the same bits on every run and under graph replay.
 *
 * ws: device, 16-byte aligned, not initialised by the caller, athd_head_cond_workspace_bytes(B, N) bytes (about
 * 4 x B x ceil(N / 64) x 64 x 384 floats: the tiles of U, G, dV and dH for the weight-gradient GEMM).  Only the backward
 * uses it; athd_head_cond takes the arguments for symmetry, ignores them and accepts NULL / 0.  w0, w2, grad_w0 and
 * grad_w2 must be 16-byte aligned; x, y and grad_y may have any 4-byte alignment and any N (16-byte loads are used when
 * N is a multiple of 4 and the base is 16-byte aligned, scalar ones otherwise).
 *
 * Both enqueue on the caller's stream, do not synchronise the host and create no HIP object, so they can be
 * graph-captured from the first call.  ATHD_ESTATE before athd_finalize; ATHD_EINVAL for a null pointer, B outside
 * [1, 65535], N < 1 or N > 1048576, a misaligned weight or workspace; ATHD_EWORKSPACE below
 * athd_head_cond_workspace_bytes (which is 0 for shapes out of range).  Checked in that order before anything is read
 * or written. */
size_t athd_head_cond_workspace_bytes(int64_t B, int64_t N);
int athd_head_cond(athd_ctx* ctx, const float* x, const float* a, const float* w0, const float* b0, const float* w2,
                   const float* b2, const float* gamma, const float* beta, int64_t B, int64_t N, float* y, void* ws,
                   size_t ws_bytes, void* stream);
int athd_head_cond_backward(athd_ctx* ctx, const float* grad_y, const float* x, const float* a, const float* w0,
                            const float* b0, const float* w2, const float* b2, const float* gamma, int64_t B, int64_t N,
                            float* grad_w0, float* grad_b0, float* grad_w2, float* grad_b2, float* grad_gamma,
                            float* grad_beta, float* grad_a, void* ws, size_t ws_bytes, void* stream);

/* ---- Head training's decoder levels (ATHTDemucs_v2.py:61-139) in both directions, from raw f32 weights ----
 * Both decoders are four levels of one operation along one axis of a channel-first slab: the frequency decoder on
 * (B, C, F, Ts) with inner = Ts contiguous columns per position, the time decoder on (B, C, L) with inner = 1.  Level l
 * in 0..3 has (Ci, Co) = (384, 192), (192, 96), (96, 48), (48, 4); levels 0..2 have GroupNorm(1) + GELU.  Per item, with
 * x (Ci, M, inner), W (Ci, Co, 8) as torch keeps a ConvTranspose weight ((Ci, Co, 8, 1) is the same memory) and every
 * index along the position axis:
 *   c[co, o] = b[co] + sum_ci W[ci, co, k1] x[ci, m1] + W[ci, co, k1 + 4] x[ci, m1 - 1],  k1 = (o + 2) mod 4,
 *              m1 = (o + 2) div 4, terms with m outside [0, M) dropped; c is (Co, 4 M, inner)
 *   h = gelu_erf(gamma_co (c - mu) r + beta_co), (mu, r) the mean and 1 / sqrt(var + 1e-5) of c over the whole item
 *       (biased variance); level 3: h = c
 *   y = resize(h) + 0.1 resize(skip): the position axis to Lt by torch's linear rule with align_corners = False, in
 *       its f32 arithmetic (src = max(0, (o + 0.5) in / Lt - 0.5), i0 = floor(src), i1 = min(i0 + 1, in - 1), weight
 *       src - i0; the identity when Lt == in), for any ratio: up, down or near 1.  skip (B, Co, S, inner) gets no
 *       gradient (it comes from the frozen half); skip == NULL with S == 0 means no skip.
 * y (B, Co, Lt, inner); stats (B, 2) = {mu, r} per item, what the backward needs beside x.
 *
 * athd_head_dec_level_backward: grad_y (B, Co, Lt, inner) with the x, parameters and stats of the forward -> grad_x
 * (B, Ci, M, inner), grad_w (Ci, Co, 8), grad_bias (Co), grad_gamma, grad_beta (Co).  c is recomputed from x; the
 * adjoint of the resize is a gather per source position (no scatter), then gelu', the GroupNorm backward
 * dc = r (D - mean D - ch mean(D ch)), D = gamma dz, ch = (c - mu) r, and the two GEMMs.  At level 3 gamma, beta, stats,
 * grad_gamma and grad_beta are ignored and may be NULL.
 *
 * All pointers are device f32; the weights are read raw at the time the kernels run (nothing is packed, nothing is
 * cached across calls).  The context is taken for its device only: the three GEMMs of a level run on
 * v_mfma_f32_16x16x4_f32 with IEEE erf / exp / sqrt / division in both dtype modes, bit-identical between them (level 3's
 * data gradient, 32 products per element, is a plain kernel that sums in double and rounds once).  x, y,
 * skip and grad_y may have any 4-byte alignment, inner and Lt any value in range (all operand loads are scalar); w and
 * grad_w must be 16-byte aligned, as torch allocates them.
 *
 * Determinism: no atomics.  Every output element is written exactly once, none is accumulated into or read.  Sums over
 * positions are taken per block of 1024 positions of a channel (8192 elements for the statistics) by a fixed tree,
 * then over the blocks in order, then over the items in order; the mean is taken first and the variance from the centred
 * values; grad_w is a split-K GEMM over the tokens of all items in a fixed number of slices per level (8, 16, 32, 64)
 * summed in slice order.  The same bits on every run and under graph replay.
 *
 * ws: device, 16-byte aligned, not initialised by the caller, athd_head_dec_workspace_bytes() bytes, the same for both
 * directions: with n = Co 4 M inner, q = ceil(4 M inner / 1024) and up4 rounding up to a multiple of 4, in floats
 *   2 up4(B n)  (c and one gradient tensor of its size)  + up4(B ceil(n / 8192)) + 2 up4(2 B)
 *   + up4(2 B Co q) + up4(B Co q) + up4(2 B Co) + up4(slices Ci Co 8);  it does not depend on Lt.
 *
 * Both enqueue on the caller's stream, do not synchronise the host and create no HIP object, so they can be
 * graph-captured from the first call.  ATHD_ESTATE before athd_finalize; ATHD_EINVAL for a null required pointer, level
 * outside 0..3, B outside [1, 65535], M outside [1, 1048576], inner outside [1, 4096], Lt outside [1, 4194304],
 * M inner > 67108864 or Lt inner > 268435456 (2048 frames need M <= 524288 and Lt <= 2097152 in the time decoder and
 * M, inner, Lt <= 2048 in the frequency decoder), a skip without S or S without a skip (S within Lt's limits), a
 * misaligned weight or workspace; ATHD_EWORKSPACE for no workspace or one below athd_head_dec_workspace_bytes (which is
 * 0 for shapes out of range).  Checked in that order before anything is read or written. */
size_t athd_head_dec_workspace_bytes(int level, int64_t B, int64_t M, int64_t inner, int64_t Lt);
int athd_head_dec_level(athd_ctx* ctx, int level, const float* x, const float* w, const float* bias, const float* gamma,
                        const float* beta, const float* skip, int64_t B, int64_t M, int64_t inner, int64_t S, int64_t Lt,
                        float* y, float* stats, void* ws, size_t ws_bytes, void* stream);
int athd_head_dec_level_backward(athd_ctx* ctx, int level, const float* grad_y, const float* x, const float* w,
                                 const float* bias, const float* gamma, const float* beta, const float* stats, int64_t B,
                                 int64_t M, int64_t inner, int64_t Lt, float* grad_x, float* grad_w, float* grad_bias,
                                 float* grad_gamma, float* grad_beta, void* ws, size_t ws_bytes, void* stream);

/* ---- Head training's output projections (freq_out / time_out, ATHTDemucs_v2.py:303-324) in both directions ----
 * A 1x1 convolution from the last decoder level's 4 channels to 2, from the decoders' channel-first layout straight
 * into the layouts athd_head_output reads (no permute, no copy in between):
 *   x (B, 4, R, S) contiguous, w (2, 4) = [out][in] and bias (2) as torch keeps a Conv1d / Conv2d(4, 2, 1) weight,
 *   y (B, S, R, 2):  y[b][s][r][o] = bias[o] + sum_c w[o][c] x[b][c][r][s]   (f32 fused multiply-adds, c ascending).
 * Frequency branch: R = rows, S = frames, y is athd_head_output's logits.  Time branch: R = 1, S = T, y is its xt.
 *
 * athd_head_proj_backward: grad_y = dL/dy in y's layout (grad_channel_first == 0: what athd_head_output_backward writes)
 * or as (B, 2, R, S) channel-first (grad_channel_first != 0: the time branch's dL/dout itself), scale NULL or (B)
 * device floats that multiply item b's gradient first (the time branch's stdt), with the x and w of the forward ->
 *   g = scale[b] grad_y;  grad_x[b][c][r][s] = sum_o w[o][c] g;  grad_w[o][c] = sum_{b,r,s} g x;  grad_b[o] = sum g.
 * One pass reads x and grad_y once.  grad_w and grad_b: every workgroup adds its positions in double in a fixed order
 * and writes ten partial sums to ws; a one-workgroup launch adds the partials in double in index order and rounds once.
 * No atomics; every output element is written exactly once, none is read: the same bits on every run and under graph
 * replay.  The arithmetic is f32 (the sums double) in both dtype modes, bit-identical between them; the context is taken
 * for its device only.
 *
 * x, y, grad_y and grad_x must be 16-byte aligned (16-byte accesses are used when R S is a multiple of 4, or R > 1 with
 * y's layout; 4-byte ones otherwise), the small tensors 4-byte aligned.  ws: device, 16-byte aligned, not initialised by
 * the caller, athd_head_proj_workspace_bytes(B, R, S) bytes = 80 B max(ceil(R S / 4096), ceil(R / 32) ceil(S / 32) if R > 1).
 *
 * Both enqueue on the caller's stream, do not synchronise the host and create no HIP object, so they can be
 * graph-captured from the first call.  ATHD_ESTATE before athd_finalize; ATHD_EINVAL for a null pointer (scale may be
 * NULL), B outside [1, 65535], R outside [1, 4096], S outside [1, 4194304], R S > 4194304 (a 2048 x 2048 grid and 47 s
 * of samples with R = 1 are inside), a misaligned pointer; ATHD_EWORKSPACE for no workspace or one below
 * athd_head_proj_workspace_bytes (which is 0 for shapes out of range), then ATHD_EINVAL for a misaligned one.  Checked
 * in that order before anything is read or written. */
size_t athd_head_proj_workspace_bytes(int64_t B, int64_t R, int64_t S);
int athd_head_proj(athd_ctx* ctx, const float* x, const float* w, const float* bias, int64_t B, int64_t R, int64_t S,
                   float* y, void* stream);
int athd_head_proj_backward(athd_ctx* ctx, const float* grad_y, int grad_channel_first, const float* scale,
                            const float* x, const float* w, int64_t B, int64_t R, int64_t S, float* grad_x,
                            float* grad_w, float* grad_b, void* ws, size_t ws_bytes, void* stream);

/* ---- Head training's attention vector (ATHTDemucs_v2.py:21-58 with one key) in both directions ----
 * a (B, 384) = out_proj(in_proj_v(v_proj(text))), the vector athd_head_cond takes: text (B, 512); wv (384, 512), bv;
 * w_in (1152, 384) and b_in (1152) the WHOLE in_proj_weight / in_proj_bias, of which the value third (rows 768..1151)
 * is read; wo (384, 384), bo.  keep (B, 2, 384) = {v_proj(text), in_proj_v(v_proj(text))} per item, what the backward
 * needs beside text.
 *
 * athd_head_attn_vec_backward: grad_a (B, 384) -> grad_wv, grad_bv, grad_wo, grad_bo and the whole grad_w_in
 * (1152, 384) and grad_b_in (1152), whose query and key thirds are exact zeros.  text gets no gradient.
 *
 * Every output element belongs to one wave (forward) or one thread (backward) that sums in double in ascending order
 * of the inner index, respectively of b, and rounds once; the two gradients that travel between the layers are rounded
 * to f32 like keep.  No atomics: the same bits on every run and under graph replay, and in both dtype modes.  The
 * backward keeps its two (B, 384) intermediates in the dead two thirds of grad_w_in until its last launch writes the
 * zeros, so grad_w_in is scratch while the backward runs and the backward's B is at most 384; the forward takes B up
 * to 65535.
 *
 * Both enqueue on the caller's stream, do not synchronise the host and create no HIP object.  ATHD_ESTATE before
 * athd_finalize; ATHD_EINVAL for a null pointer, B outside [1, 65535] (forward) or [1, 384] (backward), a pointer that is not 4-byte
 * aligned.  Checked in
 * that order before anything is read or written. */
int athd_head_attn_vec(athd_ctx* ctx, const float* text, const float* wv, const float* bv, const float* w_in,
                       const float* b_in, const float* wo, const float* bo, int64_t B, float* a, float* keep,
                       void* stream);
int athd_head_attn_vec_backward(athd_ctx* ctx, const float* grad_a, const float* text, const float* keep,
                                const float* w_in, const float* wo, int64_t B, float* grad_wv, float* grad_bv,
                                float* grad_w_in, float* grad_b_in, float* grad_wo, float* grad_bo, void* stream);

/* ---- Track level: the window loop of test_inference.py:92-141 and sdr_loss (src/loss.py:9-30) ----
 * Windows: start_k = k*hop with hop = chunk_len - overlap, for k = 0 .. athd_num_windows()-1 (while start < length),
 * end_k = min(start_k + chunk_len, length).  Window k is faded by torchaudio Fade(fade_in = k ? overlap : 0,
 * fade_out = end_k < length ? overlap : 0, 'linear') and summed into the track in ascending k.  (The reference
 * fails when a window is shorter than its fade; callers check that with the plan.) */
int64_t athd_num_windows(int64_t length, int64_t chunk_len, int64_t overlap);

/* windows: device (k1-k0, n_stems, 2, chunk_len) f32, row k-k0 = model output of window k in its first
 * end_k - start_k samples.  out: device (n_stems, 2, end_{k1-1} - start_{k0}) f32, the track span of windows
 * [k0, k1) (the whole track for k0 = 0, k1 = athd_num_windows()).  Enqueued on `stream`. */
int athd_overlap_add(const float* windows, int64_t length, int64_t chunk_len, int64_t overlap, int n_stems,
                     int64_t k0, int64_t k1, float* out, void* stream);

/* ---- Track level, benchmark.py protocol (OurModel._chunked_inference, benchmark.py:155-204) ----
 * Same window starts (hop = chunk_len - overlap, while start < length); every window's model input is zero-padded
 * to chunk_len, its first len_k = end_k - start_k outputs are used.  fade_len_k = min(overlap, len_k / 2); the
 * window weight is 1 with linspace(0, 1, fade_len) over its first fade_len samples if start_k > 0 and
 * linspace(1, 0, fade_len) over its last fade_len samples if end_k < length; output += out_k * w and
 * weight += w in ascending k, then output / max(weight, 1e-8).
 * windows: device (k1-k0, n_stems, 2, chunk_len) f32.  weight == NULL: out (n_stems, 2, span) = the normalised
 * track span of windows [k0, k1) (the track itself for the full range).  weight != NULL (device, span floats):
 * out = the unnormalised sum and weight = the weight sum of the span, for sharded runs that add spans of window
 * ranges and then normalise with athd_ola_normalize.  With overlap <= hop (at most one window of a later range on
 * any sample) the sum over ranks in rank order equals the single-range sum bit for bit; with hop < overlap a later
 * range adds its own terms first, so the sums can differ in the last bits (float addition does not re-associate). */
int athd_overlap_add_weighted(const float* windows, int64_t length, int64_t chunk_len, int64_t overlap, int n_stems,
                              int64_t k0, int64_t k1, float* out, float* weight, void* stream);
/* out (rows, n) /= max(weight (n), 1e-8) in place (benchmark.py:201-202). */
int athd_ola_normalize(float* out, const float* weight, int rows, int64_t n, void* stream);

/* SDR of src/loss.py:9-30 with the sign of test_inference.py:153: est/target device (rows, n) f32 ->
 * *out (device f32) = mean over rows of clamp(10 log10((sum t^2 + 1e-8) / (sum (t-e)^2 + 1e-8)), -30, 30).
 * scratch: device, 2*rows doubles.  Sums are accumulated in fp64.  1 <= rows <= 65535 and n >= 1; anything else
 * returns ATHD_EINVAL and writes nothing (neither *out nor scratch). */
int athd_sdr(const float* est, const float* target, int64_t rows, int64_t n, double* scratch, float* out,
             void* stream);

/* SI-SDR of src/loss.py:33-68 with the sign of benchmark.py:586: per row, zero-mean est e and target t,
 * a = <e,t> / (|t|^2 + 1e-8), clamp(10 log10((|a t|^2 + 1e-8) / (|e - a t|^2 + 1e-8)), -30, 30), mean over
 * rows -> *out (device f32).  scratch: device, 5*rows doubles.  fp64 sums.  1 <= rows <= 65535 and n >= 1, as
 * for athd_sdr. */
int athd_sisdr(const float* est, const float* target, int64_t rows, int64_t n, double* scratch, float* out,
               void* stream);

/* ---- Validation level: the metrics of src/loss.py per row and the dataset segments of src/dataloader.py, as
 * validate() of src/train.py:132-202 consumes them ----
 * Stream-only like the track level: no context, no allocation, no host synchronisation, work enqueued on `stream`,
 * capturable in a graph on one stream.
 *
 * Row metrics of src/loss.py in one call.  est/target: device (rows, n) f32, rows contiguous.
 * out: device (rows, 4) f64 = { sdr, sisdr, new_sdr, l1 } per row:
 *   sdr     = clamp(10 log10((sum t^2 + 1e-8) / (sum (t-e)^2 + 1e-8)), -30, 30)          loss.py:9-30, one row
 *   sisdr   = loss.py:33-68 for one row (zero-mean e and t, delta placement as written), clamped to +-30
 *   new_sdr = the same ratio as sdr, not clamped                                       loss.py:71-87
 *   l1      = mean |e - t| over the row                                                loss.py:150, one row
 * All sums in fp64, two sweeps over the data (the second centres on the means of the first).  Every block writes its
 * partial sums to `scratch` and a row's partials are added in a fixed order (no floating-point atomics): the table is
 * the same bits on every run.  Loads are 16 bytes wide from the first 16-byte boundary of each est row when the target
 * row is aligned at the same element (scalar loads otherwise).  scratch: device, 8-byte aligned,
 * athd_loss_rows_scratch_bytes() bytes, not initialised by the caller.  1 <= rows <= 2^20, 1 <= n < 2^31; outside that
 * athd_loss_rows_scratch_bytes returns 0 and athd_loss_rows ATHD_EINVAL. */
size_t athd_loss_rows_scratch_bytes(int64_t rows, int64_t n);
int athd_loss_rows(const float* est, const float* target, int64_t rows, int64_t n, void* scratch, double* out,
                   void* stream);

/* Dataset segments of src/dataloader.py:104-121 (random_segments = False) taken on the device.
 * stems: device (n_src, length, 2) f32, frames interleaved exactly as MusDBTracks.load_stems returns them.
 * Row r of out (rows, 2, seg_samples) = source src[r], samples [seg[r]*seg_samples, (seg[r]+1)*seg_samples),
 * channel-major, zero beyond `length`.  src: device int32 (rows), seg: device int64 (rows).  One launch; a row whose
 * src is outside [0, n_src) or whose seg is negative cannot be reported without a synchronisation: it is all zeros and
 * nothing outside `stems` is read. */
int athd_gather_segments(const float* stems, int n_src, int64_t length, const int32_t* src, const int64_t* seg,
                         int64_t rows, int64_t seg_samples, float* out, void* stream);

/* ---- Training ends: the batches and the loss gradient of train_epoch (src/train.py:23-129) ----
 * Stream-only like the validation level.  The model's own backward is not here.
 *
 * Gradient of total = -(w_sdr mean_r sdr_r + w_sisdr mean_r sisdr_r) + w_l1 mean |e - t| with respect to est, for the
 * two combined losses of src/loss.py:90-162 (combined_loss: w_l1 = 0; combined_L1_sdr_loss: w_sisdr = 0).
 *
 * athd_loss_grad_coef runs the launches of athd_loss_rows (same scratch, same limits; `table` (rows, 4) f64 has the
 * bits athd_loss_rows writes) and one more that writes coef: device (rows, 8) f64, per row
 *   [0] a_sdr = 2k / (D + d)                                   k = 10 / ln 10, d = 1e-8, D = sum (t-e)^2
 *   [1] p     = -2k / (E + d)                                  E = |(e-me) - a (t-mt)|^2, a = dot / (T + d)
 *   [2] q     = k (2aT / ((T+d)(S+d)) + 2a / (E+d) + 2c / ((T+d)(E+d)))   T = |t-mt|^2, S = a^2 T, c = dot d / (T+d)
 *   [3] gate_sdr   1 if -30 <= sdr <= 30 unclamped (read from table[.][2]), else 0
 *   [4] gate_sisdr 1 if table[.][1] lies strictly inside +-30; where it is exactly +-30 the unclamped value, evaluated
 *                  from the same sums by the same expressions, decides (on the boundary: 1, beyond: 0)
 *   [5] me = mean e   [6] mt = mean t   [7] 0
 * so the coefficients carry no weight, no 1/rows and no upstream gradient.  torch.clamp passes the gradient on the
 * closed interval; so do the gates.
 *
 * athd_loss_grad_apply: one elementwise pass, 12 bytes per element, fp64 per element rounded once to f32:
 *   grad_i = g [ w_sdr gate_sdr a_sdr (e_i - t_i) / rows - w_sisdr gate_sisdr (p (e_i - me) + q (t_i - mt)) / rows
 *                + w_l1 sign(e_i - t_i) / (rows n) ],  sign(0) = 0,
 * g = *upstream (a device f32 scalar read by the kernel, no host synchronisation), 1 when upstream is NULL.  16-byte
 * accesses where est, target and grad rows reach a 16-byte boundary at the same element, 4-byte ones otherwise.  A row
 * whose four scalars are all zero (both gates closed and w_l1 = 0, or g = 0) is written as +0.  No atomics: the same
 * bits on every run.  Shapes outside the limits of athd_loss_rows, null or misaligned pointers: ATHD_EINVAL, nothing
 * written. */
size_t athd_loss_grad_scratch_bytes(int64_t rows, int64_t n);
int athd_loss_grad_coef(const float* est, const float* target, int64_t rows, int64_t n, void* scratch, double* table,
                        double* coef, void* stream);
int athd_loss_grad_apply(const float* est, const float* target, int64_t rows, int64_t n, const double* coef,
                         double w_sdr, double w_sisdr, double w_l1, const float* upstream, float* grad, void* stream);

/* Training segments of src/dataloader.py:86-134 (random_segments = True, augment = True) taken on the device.  As
 * athd_gather_segments, but row r starts at any sample start[r] (device int64), every sample is
 * (float)((double)x * gain[r]) (gain: device f64) and the two channels are exchanged where swap[r] (device uint8) is
 * set.  The reference multiplies the float64 array stempeg returns and then calls .float() (dataloader.py:123-134,
 * 152-153): the fp64 product rounded once is bit-equal to it whenever the samples are f32-representable, which holds
 * for every PCM file MusDBTracks reads; gain == 1.0 reproduces the input bits.  Frames past `length` are zero.  A row
 * whose src is outside [0, n_src) or whose start is negative is all zeros and nothing outside `stems` is read. */
int athd_gather_train_segments(const float* stems, int n_src, int64_t length, const int32_t* src, const int64_t* start,
                               const double* gain, const uint8_t* swap, int64_t rows, int64_t seg_samples, float* out,
                               void* stream);

/* ---- Training update step: clip_grad_norm_ + torch.optim.AdamW.step of train_epoch (src/train.py:80-95) in one call,
 * with the AMP scaler's unscale and skip ----
 * Stream-only like the training ends: no context, no allocation, no host synchronisation, capturable in a graph.
 *
 * t: a HOST table of n_tensors (1..ATHD_STEP_MAX_TENSORS) entries; param, grad, exp_avg, exp_avg_sq are device f32
 * arrays of n >= 1 elements each, 4-byte aligned (16-byte accesses are used for a tensor whose four pointers are
 * 16-byte aligned).  The table is copied into the kernel arguments at the call: nothing has to stay alive, and the
 * pointers may differ from call to call.  hp: host.  The hyper-parameters are doubles: a float beta2 = 0.999f would
 * put a relative 1.3e-5 into (1 - beta2), a hundred times the rounding of a float32 step.
 *
 *   total = sum over every element of every tensor of grad^2       fp64, fixed order: one partial per chunk of 4096
 *                                                                  elements into `workspace`, added in index order
 *   inv   = grad_scale ? 1 / *grad_scale : 1                       (torch.amp.GradScaler's optimizer.grad_scale)
 *   norm  = sqrt(total) * inv
 *   coef  = max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1    clip_grad_norm_'s always-applied clamped coefficient
 *   skipped = (found_inf && *found_inf != 0) || !isfinite(norm)
 * If skipped, no parameter and no moment is written and *step stays.  Otherwise t = *step + 1 and per element, evaluated
 * in fp64 and rounded once per stored value, with g = grad * inv * coef, in torch.optim.AdamW's order:
 *   p *= 1 - lr * weight_decay;   m = beta1 m + (1 - beta1) g;   v = beta2 v + (1 - beta2) g^2;
 *   p -= (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps);      *step = t
 * stats: device, 4 floats out = { norm, coef, skipped (0 or 1), the counter after the call }.
 *
 * Two deliberate differences from torch: the gradients are read-only (clip_grad_norm_ rewrites .grad), and a
 * non-finite norm skips the step and reports it in stats[2], where torch without a scaler multiplies every gradient by
 * NaN and poisons every parameter.
 *
 * Three launches: the partial sums, the update (every workgroup adds the partials itself, in the same order, so all
 * hold the same total bit for bit), and a one-workgroup tail whose first thread writes stats and the counter; no workgroup reads a word
 * that another workgroup of the same launch writes, and there are no atomics: the same bits on every run.
 * workspace: device, 8-byte aligned, athd_head_step_workspace_bytes() bytes, not initialised by the caller.  At most
 * 4096 chunks (2^24 elements when every tensor fills its chunks; the head has 763): every workgroup of the update adds
 * all partials, so that sum grows with the square of the chunk count and the limit keeps it at a few microseconds.
 * n_tensors outside 1..64, an n < 1, more chunks than
 * that (athd_head_step_workspace_bytes returns 0 for these), a null or misaligned pointer: ATHD_EINVAL; a short
 * workspace: ATHD_EWORKSPACE; nothing is launched. */
typedef struct { float* param; const float* grad; float* exp_avg; float* exp_avg_sq; int64_t n; } athd_step_tensor;
typedef struct { double lr, beta1, beta2, eps, weight_decay, max_norm; } athd_step_hparams;  /* max_norm <= 0: no clipping */
#define ATHD_STEP_MAX_TENSORS 64
size_t athd_head_step_workspace_bytes(const athd_step_tensor* t /*host*/, int n_tensors);
int athd_head_step(const athd_step_tensor* t /*host*/, int n_tensors, const athd_step_hparams* hp /*host*/,
                   const float* grad_scale /*device, or NULL*/, const float* found_inf /*device, or NULL*/,
                   int32_t* step /*device, in/out*/, float* stats /*device, 4 floats out*/,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- Audio front end: the user path of app.py:74-126 (a file of any rate, mono or stereo) ----
 * Stream-only like the track level: no context, no host synchronisation, no device allocation, work enqueued on
 * `stream`.
 *
 * Resampler = torchaudio.transforms.Resample(orig_freq, new_freq) with its defaults (sinc_interp_hann,
 * lowpass_filter_width = 6, rolloff = 0.99):
 *   g = gcd(orig, new), o = orig / g, n = new / g, base = min(o, n) * 0.99, w = ceil(6 o / base);
 *   the table K[i][k] has n phases i and 2 w + o taps k, computed in double and rounded once to fp32:
 *     t = clamp((-i / n + (k - w) / o) * base, -6, 6),  K = sinc(pi t) * cos^2(pi t / 12) * base / o,  sinc(0) = 1;
 *   y[j n + i] = sum_k xpad[j o + k] K[i][k] with xpad[m] = x[m - w], zero outside the signal;
 *   the output has athd_resample_length() = ceil(n * length / o) samples per channel.
 * The taps outside the Hann window's support are exact zeros in the fp32 table, so the sum runs over the live band of
 * each phase only (at most 14 taps for sources up to 48 kHz -> 44.1 kHz), as fp32 FMAs in ascending tap order from
 * 0.0f: the result is the same bits on every run.
 *
 * Supported pairs: the band table (n first-tap indices + n rows of NT coefficients, NT rounded up to odd) must fit in
 * 40 KiB (it is held in LDS beside the staged input) and o + 2 w <= 6144.  That covers every common rate (8 .. 192
 * kHz <-> 44.1 / 48 kHz); a near co-prime pair such as 44101 -> 44100 is not supported: athd_resample_scratch_bytes
 * returns 0 and athd_resample ATHD_EINVAL.  orig == new is always supported (a de-interleave / duplicate pass that
 * leaves the scratch untouched).
 *
 * in: device f32, sample (frame t, channel c) at in[t * frame_stride + c * channel_stride] (strides in elements:
 * (channels, 1) reads a WAV's interleaved frames, (1, length) a planar tensor).  out: device f32, planar
 * (out_channels, athd_resample_length()).  out_channels == in_channels, or in_channels == 1 and the one channel is
 * duplicated into every output channel (app.py:123-124).  scratch: device, athd_resample_scratch_bytes() bytes
 * (the host builds the table once per pair and copies it there on `stream` in every call; ATHD_EWORKSPACE if too
 * small).  The first call for a rate pair page-locks its copy of the table (one host allocation per pair and
 * process); from then on the call only enqueues a copy and a kernel and can be captured in a graph. */
int64_t athd_resample_length(int64_t length, int orig_freq, int new_freq);
size_t athd_resample_scratch_bytes(int orig_freq, int new_freq);
int athd_resample(const float* in, int64_t length, int in_channels, int64_t frame_stride, int64_t channel_stride,
                  int orig_freq, int new_freq, float* out, int out_channels, void* scratch, size_t scratch_bytes,
                  void* stream);

/* dB spectrogram of app.py:74-94: mono = mean of the channels (one channel is used as is),
 * torch.stft(n_fft = 2048, hop_length = 512) with its defaults (rectangular window, center = True with a reflect pad
 * of 1024, one-sided), 20 log10(|X| + 1e-8).  wav: device planar (channels, T) f32 -> out: device
 * (1025, athd_spectrogram_frames(T) = 1 + T / 512) f32, frequency-major as torch returns it.  The FFT runs in fp32;
 * |X|, the logarithm and the factor 20 are evaluated in double on that spectrum and rounded once to fp32.
 * T <= 1024 returns ATHD_EINVAL (torch's reflect pad fails there too). */
int64_t athd_spectrogram_frames(int64_t T);
int athd_spectrogram_db(const float* wav, int channels, int64_t T, float* out, void* stream);

/* ---- Evaluation spectrograms: utils.compute_spectrogram / amplitude_to_db (utils.py:30-95), as benchmark.py
 * --plot-spectrograms and generate_spectrogram.py compute them, for n_signals signals of equal shape in one call ----
 * Stream-only like the audio front end: no context, no host synchronisation, no allocation; a scratch
 * initialisation and two kernels on `stream`, capturable in a graph from the first call.
 *
 * Per signal i (the planar (channels, T) f32 block at wav + i * signal_stride, signal_stride >= channels * T):
 *   mono = mean of the channels (one channel is used as is);
 *   X = torch.stft(mono, n_fft = 2048, hop_length = 512, window = torch.hann_window(2048), center = True, reflect
 *       pad of 1024, one-sided), window w[n] = 0.5 - 0.5 cos(2 pi n / 2048);
 *   S = |X|^power, power 1.0 or 2.0;
 *   to_db == 0: the result is S.  Otherwise dB = 10 log10(max(S, 1e-10)) and the result is max(dB, M - top_db) with
 *   M the maximum of dB over the signal's whole array; top_db = INFINITY leaves every value unchanged.
 * out: device (n_signals, 1025, athd_spectrogram_frames(T)) f32, frequency-major.  range: device (n_signals, 2) f32 =
 * {min, max} of each signal's result, or NULL.  scratch: device, athd_eval_spectrogram_scratch_bytes(n_signals) bytes.
 *
 * Rounding: the FFT runs in fp32; S, the logarithm and the factor 10 are evaluated in double on that spectrum and
 * rounded once to fp32; M is the maximum of those fp32 values (an integer maximum over an order-preserving encoding,
 * so it does not depend on the order of arrival); M - top_db is one fp32 subtraction and the clamp an fp32 max.  A
 * signal's result depends neither on the other signals of the call nor on the run.
 *
 * ATHD_EINVAL: T <= 1024, channels <= 0, n_signals <= 0 or > 65535, power not 1 or 2, top_db negative or NaN, a null
 * wav / out / scratch, signal_stride < channels * T, more than 2^31 - 1 groups of 8 frames.  ATHD_EWORKSPACE: scratch
 * too small.  Nothing is written in either case. */
size_t athd_eval_spectrogram_scratch_bytes(int n_signals);
int athd_eval_spectrogram(const float* wav, int n_signals, int channels, int64_t T, int64_t signal_stride,
                          float power, int to_db, float top_db, float* out, float* range, void* scratch,
                          size_t scratch_bytes, void* stream);

/* ---- Embedding comparison: embedding_comparison.py:109-111 (row normalisation), :177-184 (scikit-learn's
 * cosine_similarity and euclidean_distances) and :307-333 (analyze_clustering), for a table of n embeddings ----
 * Stream-only like the track and validation levels: no context, no allocation, no host synchronisation, three launches
 * on `stream` (rows, upper-triangular 64 x 64 tiles, one reduction), capturable in a graph on one stream.
 *
 * emb: device f32, n rows of d values, row_stride >= d elements apart.  category: device (n) int32, any values; NULL
 * only if stats is NULL.  Outputs, each NULL = skip it: normed (n, d) f32, sim (n, n) f32, dist (n, n) f32, stats 8
 * doubles.
 *   normed[i] = emb[i] / (||emb[i]|| + 1e-8): the sum of squares in fp64, the norm rounded to f32, the addition and the
 *               division in f32 (numpy's float32 arithmetic); a zero row stays zero.
 *   g_ij      = <normed_i, normed_j>, the f32 rows accumulated in fp64.
 *   sim[i,j]  = g_ij / (sqrt(g_ii) sqrt(g_jj)), a zero norm replaced by 1 (scikit-learn's normalize): a zero row gives
 *               a zero row and column, its diagonal entry included.  Rounded once to f32.
 *   dist[i,j] = sqrt(max(g_ii + g_jj - 2 g_ij, 0)) in fp64, rounded once to f32; the diagonal is exactly 0.
 *   Each pair i <= j is computed once and stored at [i,j] and [j,i]: both matrices are bit-symmetric.  g_ii, g_jj and
 *   g_ij are summed in the same order, so two rows of identical bits have distance exactly 0.
 *   stats     = { intra_mean, intra_std, inter_mean, inter_std, separation, n_intra, n_inter, 0 } over the pairs i < j
 *               of the f32 values written (or that would be written) to sim, split by category[i] == category[j], in
 *               fp64; std is the population standard deviation, centred (exactly 0 for constant data); an empty class
 *               gives NaN for its mean and std and for the separation (np.mean([]) in the reference).
 * Every tile writes its partial counts and sums to `scratch` and the last launch adds them in a fixed order (no
 * floating-point atomics): all outputs are the same bits on every run and under graph replay.  Loads are 16 bytes wide
 * where a row's groups of four start on a 16-byte boundary, scalar otherwise (any 4-byte aligned emb and row_stride).
 *
 * scratch: device, 8-byte aligned, athd_embed_compare_scratch_bytes() bytes, not initialised by the caller.
 * 1 <= n <= 4096, 1 <= d <= 4096, row_stride >= d; outside that athd_embed_compare_scratch_bytes returns 0 and
 * athd_embed_compare ATHD_EINVAL, as for a NULL emb or scratch and a NULL category with stats set.  ATHD_EWORKSPACE:
 * scratch too small.  Nothing is written in any of these cases. */
size_t athd_embed_compare_scratch_bytes(int n, int d);
int athd_embed_compare(const float* emb, int n, int d, int64_t row_stride, const int32_t* category, float* normed,
                       float* sim, float* dist, double* stats, void* scratch, size_t scratch_bytes, void* stream);

/* ---- CLAP text tower: token ids -> prompt embeddings (ATHTDemucs_v2.py:238-248, :282) ----
 * RoBERTa-base (12 post-LN layers, hidden 768, 12 heads of 64, FFN 3072, exact GELU), the tanh pooler on the first
 * token and the 768 -> 512 -> 512 ReLU projection of laion/clap-htsat-unfused, with the weights a reference checkpoint
 * carries under clap.text_model.* / clap.text_projection.*.  A context of its own: athd_create / athd_set_weight /
 * athd_finalize still ignore clap.* and an athd_ctx does not grow.
 *
 * Keys are the Hugging Face names (a leading "clap." is stripped): text_model.embeddings.{word,position,token_type}_
 * embeddings.weight, text_model.embeddings.LayerNorm.*, text_model.encoder.layer.{0..11}.*, text_model.pooler.dense.*,
 * text_projection.linear{1,2}.* - 203 fp32 tensors (athd_text_required_key).  Other keys (the integer buffers
 * position_ids / token_type_ids, the audio tower) are accepted and ignored.  The dimensions are the checkpoint's and
 * fixed: vocab 50265, 514 positions, 768 / 12 / 3072, projection 512, LayerNorm eps 1e-12, pad id 1;
 * athd_text_finalize returns ATHD_EKEY for a missing or mis-shaped key.  dtype: ATHD_F32 = fp32 weights and fp32 MFMA;
 * ATHD_BF16 = bf16 matrix weights and bf16-rounded GEMM inputs with fp32 accumulation (the embedding tables, biases,
 * LayerNorms, attention scores and softmax stay fp32).
 *
 * Semantics, per prompt p of input_ids / attention_mask (P, L) int32:
 *   pos = cumsum(ids != 1) * (ids != 1) + 1           (RoBERTa's rule: it reads the ids, not the mask)
 *   x = LN(word[id] + type[0] + position[pos])
 *   per layer: q, k, v = linear(x); scores = q k^T / 8 per head, softmax over the keys with mask != 0 (a key with mask 0
 *     gets probability exactly 0); x = LN(out(attn) + x); x = LN(W2 gelu_erf(W1 x + b1) + b2 + x)
 *   pooled = tanh(dense(x[:, 0])); emb = linear2(relu(linear1(pooled)))
 *   normalize != 0: out = emb / max(||emb||2, 1e-12)   == ClapModel.get_text_features (:241-244)
 *   normalize == 0: out = emb                          == ClapTextModelWithProjection.forward(...).text_embeds (:245-248)
 *
 * input_ids, attention_mask, out (P, 512) f32 and workspace are device memory (out and workspace 16-byte aligned).
 * athd_text_encode is stream-only: no host synchronisation, no allocation and no launch-configuration query (all of
 * that happens in athd_text_finalize), so it can be captured in a graph from the first call and `out` can be handed to
 * athd_forward_prompts as text_table on the same stream.  ATHD_EINVAL: P outside 1..256, L outside 1..128 (one head's
 * q, k and v sit in LDS in fp32), a null pointer; ATHD_EWORKSPACE: workspace smaller than athd_text_workspace_bytes
 * (which is 0 for P / L out of range); ATHD_ESTATE: before athd_text_finalize.  Nothing is written in those cases.
 * An id outside [0, 50265) cannot be reported without a synchronisation: it is clamped into the table, that prompt's
 * row is unspecified, nothing faults and the other rows are unaffected; the same holds for a prompt whose mask is all
 * zero.  A prompt's row depends neither on the other prompts of the call, nor on how far the batch is padded, nor on
 * the run: masked keys contribute exact zeros, every reduction (split-K included) has a fixed order that depends on
 * the GEMM's (N, K) only, and there are no floating-point atomics. */
typedef struct athd_text_ctx athd_text_ctx;
int athd_text_create(athd_text_ctx** out, int device, int dtype);
int athd_text_set_weight(athd_text_ctx* ctx, const char* key, const void* host, const int64_t* shape, int ndim,
                         int src_dtype);
int athd_text_num_required_keys(void);
const char* athd_text_required_key(int i);
int athd_text_finalize(athd_text_ctx* ctx);
size_t athd_text_workspace_bytes(athd_text_ctx* ctx, int P, int L);
int athd_text_encode(athd_text_ctx* ctx, const int32_t* input_ids, const int32_t* attention_mask, int P, int L,
                     int normalize, float* out, void* workspace, size_t workspace_bytes, void* stream);
const char* athd_text_last_error(athd_text_ctx* ctx);
void athd_text_destroy(athd_text_ctx* ctx);

/* Kernel timing (measurement aid for bench.py; not part of the reference interface).  Between
 * athd_profile_start and athd_profile_stop every launch of kernel `kernel` (its rocprofv3 symbol without
 * "void athd::", the argument list and 'u' suffixes, e.g. "attn_kernel<0>"; NULL or "" = all kernels) made
 * by this context's forwards is bracketed by HIP events on the launch stream.  athd_profile_stop synchronises
 * those events and aggregates per kernel: launches, summed event time, summed ALGORITHMIC flops and bytes.
 * kernel = "@section": every kernel, aggregated per forward section ("encoder", "transformer", "decoder").
 * kernel = "@sites": every kernel per call site, labelled "kernel@stage.site" (e.g.
 * "gemm4_kernel<129>@transformer.linear1"); kernel = "<kernel>@<stage.site>": every launch of that one call site.
 * While a profile is open the time branch runs on the caller's stream, so each event pair times one kernel. */
int athd_profile_start(athd_ctx* ctx, const char* kernel);
int athd_profile_stop(athd_ctx* ctx);
int athd_profile_count(athd_ctx* ctx);
int athd_profile_get(athd_ctx* ctx, int i, const char** kernel, long long* launches, double* ms, double* flops,
                     double* bytes);

/* Last error message of this context ("" if none). */
const char* athd_last_error(athd_ctx* ctx);

void athd_destroy(athd_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* ATHD_H */
