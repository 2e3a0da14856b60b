// Shapes, workspace layout and the ATHD_DUMP debug aid of the forward.  The workspace layout is computed by the same
// code path in a sizing pass (athd_workspace_bytes).
#include "forward.h"

namespace athd_fwd {

Dims make_dims(const athd_ctx* c, int64_t B, int64_t T, int P) {
    Dims d;
    d.B = B; d.T = T; d.P = P;
    d.Tspec = (int)cdiv(T, 1024);
    d.L[0] = T;
    for (int i = 0; i < 4; ++i) d.L[i + 1] = cdiv(d.L[i], 4);
    d.Nf = 8LL * d.Tspec;
    d.Nt = d.L[4];
    d.Nmax = std::max(d.Nf, d.Nt);
    // (segment, prompt) items per decode chunk; the decoder's buffers scale with it.  Library default 64 (an 18 GB
    // workspace at B=64 x P=4); bench.py sets 256 = the whole bench batch in one chunk (51 GB, sized for the 288 GB
    // of HBM: fewer, larger decoder launches; measured 32 / 64 / 128 / 256 items: 1203 / 1238 / 1263 / 1284
    // segments/s).  ATHD_DECODE_ITEMS overrides the context's setting.
    int64_t items_per_chunk = c ? c->decode_items : 64;
    if (const char* e = std::getenv("ATHD_DECODE_ITEMS")) {
        const long v = std::strtol(e, nullptr, 10);
        if (v > 0) items_per_chunk = v;
    }
    d.Bc = std::max<int64_t>(1, std::min<int64_t>(B, items_per_chunk / P));
    d.chunks = cdiv(B, d.Bc);
    return d;
}

size_t plan(Arena& ar, const Dims& d, Bufs& b, bool actbf) {
    const int64_t B = d.B, Ts = d.Tspec;
    const size_t ab = actbf ? 2 : 4;
    auto act = [&](int64_t n) -> void* { return (void*)ar.take<char>(n * (int64_t)ab); };
    // stats pool
    int64_t ns = 0;
    for (int i = 0; i < 4; ++i) ns += 4 * (B * d.F[i + 1]) + 4 * B;
    ns += 10 * B + 4 * B;
    ns += d.chunks * 6 * d.Bc * d.P;
    b.nstats = ns;
    b.stats = ar.take<double>(2 * ns);
    b.specT = ar.take<float>(B * 2048 * Ts * 4);
    b.snorm = ar.take<float>(2 * B);
    b.tnorm_div = ar.take<float>(2 * B);
    b.tnorm_std = ar.take<float>(2 * B);
    int64_t ymax = 0, hmax = 0, ymax_t = 0, hmax_t = 0;
    for (int i = 0; i < 4; ++i) {
        const int64_t C = ENC_CH[i];
        b.saved[i] = act(B * d.F[i + 1] * Ts * C);
        b.saved_t[i] = act(B * d.L[i + 1] * C);
        const int64_t rows = B * d.F[i + 1] * Ts, rows_t = B * d.L[i + 1];
        ymax = std::max(ymax, rows * C);
        const int64_t hs = C <= 96 ? 16 : C / 8;     // (C = 48, 96: hidden rows padded to 16 for the MFMA passes)
        hmax = std::max(hmax, rows * hs);
        ymax_t = std::max(ymax_t, rows_t * C);
        hmax_t = std::max(hmax_t, rows_t * hs);
    }
    b.sk4 = act(B * d.F[1] * Ts * 4);
    b.sk4t = act(B * d.L[1] * 4);
    b.ybuf_t = act(ymax_t);
    b.hbuf_t = ar.take<float>(hmax_t);
    b.hbuf_b_t = ab == 2 ? ar.take<uint16_t>(hmax_t) : nullptr;
    b.ybuf = act(ymax);
    b.ea = (int)ab;
    b.hbuf = ar.take<float>(hmax);
    b.hbuf_b = ab == 2 ? ar.take<uint16_t>(hmax) : nullptr;
    b.X = ar.take<float>(B * d.Nf * 512);
    b.XT = ar.take<float>(B * d.Nt * 512);
    for (int i = 0; i < 4; ++i) b.H[i] = act(B * d.Nmax * 512);
    b.QKV = act(B * d.Nmax * 1536);
    b.O = act(B * d.Nmax * 512);
    b.F1 = act(B * d.Nmax * 2048);
    b.QKVt = act(B * d.Nmax * 1536);
    b.Ot = act(B * d.Nt * 512);
    b.F1t = act(B * d.Nt * 2048);
    b.pos2d = ar.take<float>(d.Nf * 512);
    b.pos1d = ar.take<float>(d.Nt * 512);
    b.x_enc = ar.take<float>(B * d.Nf * 384);
    b.xt_enc = ar.take<float>(B * d.Nt * 384);
    b.x_enc_b = actbf ? ar.take<uint16_t>(B * d.Nf * 384) : nullptr;
    b.xt_enc_b = actbf ? ar.take<uint16_t>(B * d.Nt * 384) : nullptr;
    // decode chunk
    const int64_t NI = d.Bc * d.P;
    b.avec = ar.take<float>(NI * 384);
    b.tc0 = ar.take<float>(NI * 384);
    b.tc2 = ar.take<float>(NI * 384);
    b.Hm = act(NI * d.Nf * 384);
    b.Yb = ar.take<float>(NI * d.Nf * 384);
    b.Hmt = act(NI * d.Nt * 384);
    b.Ybt = ar.take<float>(NI * d.Nt * 384);
    b.x_cond = ar.take<float>(NI * d.Nf * 384);
    b.xt_cond = ar.take<float>(NI * d.Nt * 384);
    // ConvT outputs (G, Gt) and merge outputs (D, Dt) of the largest level; d.T * 2: tdec_last output xt2 [NI][T][2]
    const int64_t gt = std::max<int64_t>({4 * d.Nt * 192, 4 * d.L[3] * 96, 4 * d.L[2] * 48, d.T * 2});
    const int64_t dmt = std::max<int64_t>({d.L[3] * 192, d.L[2] * 96, d.L[1] * 48});
    b.G = ar.take<float>(NI * std::max<int64_t>({32 * Ts * 192, 2 * Ts * Ts * 96, gt}));
    b.D = ar.take<float>(NI * std::max<int64_t>(Ts * Ts * 192, dmt));
    b.Gt = ar.take<float>(NI * gt);
    b.Dt = ar.take<float>(NI * dmt);
    b.S = act(NI * 32 * Ts * DEC_CH[1]);
    b.Z = act(NI * 32 * Ts * 8 * DEC_CH[2]);
    b.Zs = act(d.Bc * 8 * Ts * 8 * DEC_CH[2]);
    b.FO = ar.take<float>(NI * Ts * Ts * 2);
    if (d.chunks > 1) b.FO2 = ar.take<float>(NI * Ts * Ts * 2);
    b.ola_part = ar.take<float>(istft_ola_part_floats(NI, (int)Ts));
    b.lrsteps = ar.take<LrStep>(Ts + 1);
    b.gram = actbf ? ar.take<float>(fdec1_gram_floats(NI, (int)Ts)) : nullptr;
    b.gramq = actbf ? ar.take<double>(fdec1_gram_q_doubles()) : nullptr;
    for (int i = 0; i < 2; ++i) b.skw[i] = actbf ? ar.take<float>(SK_WS_BYTES / 4) : nullptr;
    return ar.off;
}

// n bytes at device pointer p -> <dir>/<name>; false when the copy failed
static bool dump_dev(const char* dir, const std::string& name, const void* p, size_t n) {
    std::vector<char> h(n);
    if (hipMemcpy(h.data(), p, n, hipMemcpyDeviceToHost) != hipSuccess) return false;
    FILE* f = std::fopen((std::string(dir) + "/" + name).c_str(), "wb");
    if (f) { std::fwrite(h.data(), 1, n, f); std::fclose(f); }
    return true;
}

// Debug aid: ATHD_DUMP=<dir> makes the forward synchronise at the end and write the main intermediates of the
// first decode chunk as raw little-endian arrays (<dir>/<name>.f32 / .f64) plus <dir>/index.txt with shapes.
void dump_all(const Dims& d, const Bufs& b, const float* xt2, size_t gap, hipStream_t s) {
    const char* dir = std::getenv("ATHD_DUMP");
    if (!dir || !*dir) return;
    if (hipStreamSynchronize(s) != hipSuccess) return;
    const int64_t B = d.B, Ts = d.Tspec, NI = std::min(d.B, d.Bc) * d.P;
    struct E { std::string name; const void* p; int64_t n; std::string shape; };
    std::vector<E> es = {
        {"specT", b.specT, B * Ts * 2048 * 4, "B,Ts,2048,4"},
        {"snorm", b.snorm, 2 * B, "B,2"}, {"tnorm_std", b.tnorm_std, 2 * B, "B,2"},
        {"x_enc", b.x_enc, B * d.Nf * 384, "B,Nf,384"}, {"xt_enc", b.xt_enc, B * d.Nt * 384, "B,Nt,384"},
        {"x_cond", b.x_cond, NI * d.Nf * 384, "NI,Nf,384"}, {"xt_cond", b.xt_cond, NI * d.Nt * 384, "NI,Nt,384"},
        {"FO", b.FO, NI * Ts * Ts * 2, "NI,t,row,2"}, {"XT2", xt2, NI * d.T * 2, "NI,T,2"},
    };
    for (int i = 0; i < 4; ++i) {
        const std::string si = std::to_string(i);
        const int64_t nf = B * d.F[i + 1] * Ts * ENC_CH[i], nt = B * d.L[i + 1] * ENC_CH[i];
        if (b.ea == 4) {         // encoder activations are f32 only in parity mode
            es.push_back({"saved" + si, b.saved[i], nf, "B,F,Ts,C"});
            es.push_back({"saved_t" + si, b.saved_t[i], nt, "B,L,C"});
        } else {                 // bf16 mode: the encoder levels as raw bf16 (<name>.bf16)
            dump_dev(dir, "saved" + si + ".bf16", b.saved[i], (size_t)nf * 2);
            dump_dev(dir, "saved_t" + si + ".bf16", b.saved_t[i], (size_t)nt * 2);
        }
    }
    // the decoder's scratch buffers as raw bytes (<name>.raw; sizes from the arena order in plan(), less Arena::gap)
    struct Rw { const char* name; const void* p; const void* end; };
    const Rw rws[] = {{"G", b.G, b.D}, {"D", b.D, b.Gt}, {"Gt", b.Gt, b.Dt}, {"Dt", b.Dt, b.S}, {"S", b.S, b.Z},
                      {"Z", b.Z, b.Zs}, {"Zs", b.Zs, b.FO}, {"stats", b.stats, b.specT}};
    for (const auto& e : rws)
        if (e.p && e.end && (const char*)e.end > (const char*)e.p + gap)
            dump_dev(dir, std::string(e.name) + ".raw", e.p, (size_t)((const char*)e.end - (const char*)e.p) - gap);
    FILE* fi = std::fopen((std::string(dir) + "/index.txt").c_str(), "w");
    for (const auto& e : es)
        if (dump_dev(dir, e.name + ".f32", e.p, (size_t)e.n * 4) && fi)
            std::fprintf(fi, "%s %lld %s\n", e.name.c_str(), (long long)e.n, e.shape.c_str());
    if (fi) std::fclose(fi);
}

}  // namespace athd_fwd
