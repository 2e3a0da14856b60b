// athd C ABI (include/athd.h): context lifetime, weight staging and athd_finalize, the track-level, loss, audio and
// embedding entry points over their launchers, the kernel profile.  Status codes out, nothing thrown.  The forward's
// entries are forward.cpp's and forward_export.cpp's, the packing behind athd_finalize is pack.cpp's.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/athd.h"
#include "ctx.h"
#include "kernels.h"

// a launcher's code (0, -1: bad argument, -5: scratch too small, else a HIP error) as the ABI's status
static int api_rc(int rc) {
    return rc == 0 ? ATHD_OK : rc == -1 ? ATHD_EINVAL : rc == -5 ? ATHD_EWORKSPACE : ATHD_EHIP;
}

extern "C" {

int athd_version(void) { return 105; }

int athd_num_required_keys(void) { return (int)required_keys().size(); }

const char* athd_required_key(int i) {
    if (i < 0 || i >= (int)required_keys().size()) return nullptr;
    return required_keys()[i].first.c_str();
}

int athd_create(athd_ctx** out, int device, int dtype) {
    if (!out || (dtype != ATHD_F32 && dtype != ATHD_BF16)) return ATHD_EINVAL;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return ATHD_EHIP;
    athd_ctx* c = new athd_ctx();
    c->device = device;
    c->mode = dtype;
    *out = c;
    return ATHD_OK;
}

int athd_set_weight(athd_ctx* c, const char* key, const void* host, const int64_t* shape, int ndim, int src_dtype) {
    if (!c || !key || !host || (ndim > 0 && !shape)) return ATHD_EINVAL;
    if (c->finalized) return c->fail(ATHD_ESTATE, "athd_set_weight after finalize");
    if (src_dtype != 0) return c->fail(ATHD_EINVAL, std::string("only fp32 host weights are accepted: ") + key);
    bool needed = false;
    for (const auto& k : required_keys())
        if (k.first == key) { needed = true; break; }
    if (!needed) return ATHD_OK;   // strict=False: ignore keys outside the hot path
    HostT t;
    int64_t n = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= shape[i]; }
    t.v.assign((const float*)host, (const float*)host + n);
    c->host[key] = std::move(t);
    return ATHD_OK;
}

int athd_finalize(athd_ctx* c) {
    if (!c) return ATHD_EINVAL;
    if (c->finalized) return c->fail(ATHD_ESTATE, "already finalized");
    for (const auto& k : required_keys()) {
        auto it = c->host.find(k.first);
        if (it == c->host.end()) return c->fail(ATHD_EKEY, "missing weight: " + k.first);
        if (it->second.shape != k.second) return c->fail(ATHD_EKEY, "shape mismatch for " + k.first);
    }
    if (hipSetDevice(c->device) != hipSuccess) return c->fail(ATHD_EHIP, "hipSetDevice failed");
    pack_encoders(*c);
    pack_transformer(*c);
    pack_text_attn(*c);
    pack_decoders(*c);
    pack_tables(*c);
    for (void* p : c->allocs)
        if (!p) return c->fail(ATHD_EHIP, "device allocation failed");
    if (c->upload_failed) return c->fail(ATHD_EHIP, "weight upload failed");
    // the time branch's stream and the fork / join events, made here so that athd_forward* create nothing (they
    // can then be captured in a HIP graph from the first call on)
    if (!c->s_time && hipStreamCreateWithFlags(&c->s_time, hipStreamNonBlocking) != hipSuccess)
        return c->fail(ATHD_EHIP, "stream creation failed");
    if (!c->ev_f && hipEventCreateWithFlags(&c->ev_f, hipEventDisableTiming) != hipSuccess)
        return c->fail(ATHD_EHIP, "event creation failed");
    if (!c->ev_t && hipEventCreateWithFlags(&c->ev_t, hipEventDisableTiming) != hipSuccess)
        return c->fail(ATHD_EHIP, "event creation failed");
    if (hipDeviceSynchronize() != hipSuccess) return c->fail(ATHD_EHIP, "upload failed");
    c->host.clear();
    c->finalized = true;
    return ATHD_OK;
}

int athd_set_decode_items(athd_ctx* c, int64_t items) {
    if (!c) return ATHD_EINVAL;
    if (items < 1 || items > 4096) return c->fail(ATHD_EINVAL, "decode_items must be in [1, 4096]");
    c->decode_items = items;
    return ATHD_OK;
}

int64_t athd_num_windows(int64_t length, int64_t chunk_len, int64_t overlap) {
    if (length <= 0 || chunk_len <= 0 || overlap < 0 || overlap >= chunk_len) return 0;
    const int64_t hop = chunk_len - overlap;
    return (length + hop - 1) / hop;
}

int athd_overlap_add(const float* windows, int64_t length, int64_t chunk_len, int64_t overlap, int n_stems,
                     int64_t k0, int64_t k1, float* out, void* stream) {
    return api_rc(ola_launch(windows, length, chunk_len, overlap, n_stems, k0, k1, out, (hipStream_t)stream));
}

int athd_overlap_add_weighted(const float* windows, int64_t length, int64_t chunk_len, int64_t overlap, int n_stems,
                              int64_t k0, int64_t k1, float* out, float* weight, void* stream) {
    return api_rc(ola_launch(windows, length, chunk_len, overlap, n_stems, k0, k1, out, (hipStream_t)stream, 1, weight));
}

int athd_ola_normalize(float* out, const float* weight, int rows, int64_t n, void* stream) {
    return api_rc(ola_normalize_launch(out, weight, rows, n, (hipStream_t)stream));
}

int athd_sdr(const float* est, const float* target, int64_t rows, int64_t n, double* scratch, float* out,
             void* stream) {
    return api_rc(sdr_launch(est, target, rows, n, scratch, out, (hipStream_t)stream));
}

int athd_sisdr(const float* est, const float* target, int64_t rows, int64_t n, double* scratch, float* out,
               void* stream) {
    return api_rc(sisdr_launch(est, target, rows, n, scratch, out, (hipStream_t)stream));
}

size_t athd_loss_rows_scratch_bytes(int64_t rows, int64_t n) { return loss_rows_scratch_bytes(rows, n); }

int athd_loss_rows(const float* est, const float* target, int64_t rows, int64_t n, void* scratch, double* out,
                   void* stream) {
    return api_rc(loss_rows_launch(est, target, rows, n, scratch, out, (hipStream_t)stream));
}

int athd_gather_segments(const float* stems, int n_src, int64_t length, const int32_t* src, const int64_t* seg,
                         int64_t rows, int64_t seg_samples, float* out, void* stream) {
    return api_rc(gather_segments_launch(stems, n_src, length, src, seg, rows, seg_samples, out, (hipStream_t)stream));
}

size_t athd_loss_grad_scratch_bytes(int64_t rows, int64_t n) { return loss_rows_scratch_bytes(rows, n); }

int athd_loss_grad_coef(const float* est, const float* target, int64_t rows, int64_t n, void* scratch, double* table,
                        double* coef, void* stream) {
    return api_rc(loss_grad_coef_launch(est, target, rows, n, scratch, table, coef, (hipStream_t)stream));
}

int athd_loss_grad_apply(const float* est, const float* target, int64_t rows, int64_t n, const double* coef,
                         double w_sdr, double w_sisdr, double w_l1, const float* upstream, float* grad, void* stream) {
    return api_rc(loss_grad_apply_launch(est, target, rows, n, coef, w_sdr, w_sisdr, w_l1, upstream, grad,
                                         (hipStream_t)stream));
}

int athd_gather_train_segments(const float* stems, int n_src, int64_t length, const int32_t* src, const int64_t* start,
                               const double* gain, const uint8_t* swap, int64_t rows, int64_t seg_samples, float* out,
                               void* stream) {
    return api_rc(gather_train_segments_launch(stems, n_src, length, src, start, gain, swap, rows, seg_samples, out,
                                               (hipStream_t)stream));
}

int64_t athd_resample_length(int64_t length, int orig_freq, int new_freq) {
    return resample_length(length, orig_freq, new_freq);
}

size_t athd_resample_scratch_bytes(int orig_freq, int new_freq) { return resample_scratch_bytes(orig_freq, new_freq); }

int athd_resample(const float* in, int64_t length, int in_channels, int64_t frame_stride, int64_t channel_stride,
                  int orig_freq, int new_freq, float* out, int out_channels, void* scratch, size_t scratch_bytes,
                  void* stream) {
    return api_rc(resample_launch(in, length, in_channels, frame_stride, channel_stride, orig_freq, new_freq, out,
                                  out_channels, scratch, scratch_bytes, (hipStream_t)stream));
}

int64_t athd_spectrogram_frames(int64_t T) { return spectrogram_frames(T); }

int athd_spectrogram_db(const float* wav, int channels, int64_t T, float* out, void* stream) {
    return api_rc(spectrogram_db_launch(wav, channels, T, out, (hipStream_t)stream));
}

size_t athd_eval_spectrogram_scratch_bytes(int n_signals) { return eval_spectrogram_scratch_bytes(n_signals); }

int athd_eval_spectrogram(const float* wav, int n_signals, int channels, int64_t T, int64_t signal_stride, float power,
                          int to_db, float top_db, float* out, float* range, void* scratch, size_t scratch_bytes,
                          void* stream) {
    return api_rc(eval_spectrogram_launch(wav, n_signals, channels, T, signal_stride, power, to_db, top_db, out, range,
                                          scratch, scratch_bytes, (hipStream_t)stream));
}

size_t athd_embed_compare_scratch_bytes(int n, int d) { return embed_compare_scratch_bytes(n, d); }

int athd_embed_compare(const float* emb, int n, int d, int64_t row_stride, const int32_t* category, float* normed,
                       float* sim, float* dist, double* stats, void* scratch, size_t scratch_bytes, void* stream) {
    return api_rc(embed_compare_launch(emb, n, d, row_stride, category, normed, sim, dist, stats, scratch,
                                       scratch_bytes, (hipStream_t)stream));
}

int athd_profile_start(athd_ctx* c, const char* kernel) {
    if (!c) return ATHD_EINVAL;
    delete c->prof;
    c->prof = new KProf();
    c->prof->only = kernel ? kernel : "";
    c->prof_done.agg.clear();
    return ATHD_OK;
}

int athd_profile_stop(athd_ctx* c) {
    if (!c || !c->prof) return c ? c->fail(ATHD_ESTATE, "athd_profile_stop without start") : ATHD_EINVAL;
    const int rc = c->prof->collect();
    c->prof_done.agg = c->prof->agg;
    delete c->prof;
    c->prof = nullptr;
    return rc == 0 ? ATHD_OK : c->fail(ATHD_EHIP, "profile event query failed");
}

int athd_profile_count(athd_ctx* c) { return c ? (int)c->prof_done.agg.size() : 0; }

int athd_profile_get(athd_ctx* c, int i, const char** kernel, long long* launches, double* ms, double* flops,
                     double* bytes) {
    if (!c || i < 0 || i >= (int)c->prof_done.agg.size()) return ATHD_EINVAL;
    const auto& g = c->prof_done.agg[i];
    if (kernel) *kernel = g.label.c_str();
    if (launches) *launches = g.n;
    if (ms) *ms = g.ms;
    if (flops) *flops = g.flops;
    if (bytes) *bytes = g.bytes;
    return ATHD_OK;
}

const char* athd_last_error(athd_ctx* c) { return c ? c->err.c_str() : "null context"; }

void athd_destroy(athd_ctx* c) {
    if (!c) return;
    for (void* p : c->allocs) (void)hipFree(p);
    if (c->ev_f) (void)hipEventDestroy(c->ev_f);
    if (c->ev_t) (void)hipEventDestroy(c->ev_t);
    if (c->s_time) (void)hipStreamDestroy(c->s_time);
    delete c->prof;
    delete c;
}

}  // extern "C"
