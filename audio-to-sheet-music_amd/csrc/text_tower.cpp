// athd_text_*: the CLAP text tower behind the C ABI (include/athd.h) - a context of its own (athd_ctx does not grow),
// Hugging Face key names, validation and packing at finalize, and the stream-only encode over text_tower.hip.
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/athd.h"
#include "text_tower.h"

using namespace athd;

namespace {

struct KeySpec { std::string key; std::vector<int64_t> shape; };

const std::vector<KeySpec>& text_keys() {
    static const std::vector<KeySpec> ks = [] {
        std::vector<KeySpec> v;
        auto lin = [&](const std::string& p, int64_t n, int64_t k) {
            v.push_back({p + ".weight", {n, k}});
            v.push_back({p + ".bias", {n}});
        };
        auto ln = [&](const std::string& p) {
            v.push_back({p + ".weight", {TT_H}});
            v.push_back({p + ".bias", {TT_H}});
        };
        const std::string e = "text_model.embeddings.";
        v.push_back({e + "word_embeddings.weight", {TT_VOCAB, TT_H}});
        v.push_back({e + "position_embeddings.weight", {TT_NPOS, TT_H}});
        v.push_back({e + "token_type_embeddings.weight", {1, TT_H}});
        ln(e + "LayerNorm");
        for (int l = 0; l < TT_LAYERS; ++l) {
            const std::string p = "text_model.encoder.layer." + std::to_string(l) + ".";
            lin(p + "attention.self.query", TT_H, TT_H);
            lin(p + "attention.self.key", TT_H, TT_H);
            lin(p + "attention.self.value", TT_H, TT_H);
            lin(p + "attention.output.dense", TT_H, TT_H);
            ln(p + "attention.output.LayerNorm");
            lin(p + "intermediate.dense", TT_FFN, TT_H);
            lin(p + "output.dense", TT_H, TT_FFN);
            ln(p + "output.LayerNorm");
        }
        lin("text_model.pooler.dense", TT_H, TT_H);
        lin("text_projection.linear1", TT_PROJ, TT_H);
        lin("text_projection.linear2", TT_PROJ, TT_PROJ);
        return v;
    }();
    return ks;
}

struct HostT { std::vector<int64_t> shape; std::vector<float> v; };

uint16_t f2bf_host(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

struct Lin { const void* w = nullptr; const float* b = nullptr; const TtGemmPlan* plan = nullptr; };
struct Norm { const float* w = nullptr; const float* b = nullptr; };
struct Layer { Lin qkv, out, ffn1, ffn2; Norm ln1, ln2; };

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

struct athd_text_ctx {
    int device = 0, mode = ATHD_F32;
    bool finalized = false;
    std::string err;
    std::map<std::string, HostT> host;
    unsigned char* arena = nullptr;     // every packed weight, one allocation
    const float *word = nullptr, *pos = nullptr, *type0 = nullptr;
    Norm emb_ln;
    Layer layer[TT_LAYERS];
    Lin pooler, lin1, lin2;
    int fail(int code, const std::string& m) { err = m; return code; }
};

namespace {

// workspace: x (M,768) | y (M,768) | h (M,3072) | part (M, TT_MAX_SN), each 256-byte aligned
struct Ws { size_t x, y, h, part, total; };
Ws ws_layout(int P, int L) {
    const size_t M = (size_t)P * L;
    Ws w;
    size_t o = 0;
    w.x = o; o += align256(M * TT_H * 4);
    w.y = o; o += align256(M * TT_H * 4);
    w.h = o; o += align256(M * TT_FFN * 4);
    w.part = o; o += align256(M * TT_MAX_SN * 4);
    w.total = o;
    return w;
}

bool dims_ok(int P, int L) { return P >= 1 && P <= TT_MAX_P && L >= 1 && L <= TT_MAX_L; }

}  // namespace

extern "C" {

int athd_text_num_required_keys(void) { return (int)text_keys().size(); }

const char* athd_text_required_key(int i) {
    if (i < 0 || i >= (int)text_keys().size()) return nullptr;
    return text_keys()[i].key.c_str();
}

int athd_text_create(athd_text_ctx** out, int device, int dtype) {
    if (!out || (dtype != ATHD_F32 && dtype != ATHD_BF16)) return ATHD_EINVAL;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return ATHD_EHIP;
    athd_text_ctx* c = new athd_text_ctx();
    c->device = device;
    c->mode = dtype;
    *out = c;
    return ATHD_OK;
}

int athd_text_set_weight(athd_text_ctx* c, const char* key, const void* host, const int64_t* shape, int ndim,
                         int src_dtype) {
    if (!c || !key || !host || ndim < 0 || (ndim > 0 && !shape)) return ATHD_EINVAL;
    if (c->finalized) return c->fail(ATHD_ESTATE, "athd_text_set_weight after finalize");
    if (src_dtype != 0) return c->fail(ATHD_EINVAL, std::string("only fp32 host weights are accepted: ") + key);
    std::string k = key;
    if (k.compare(0, 5, "clap.") == 0) k = k.substr(5);
    bool needed = false;
    for (const auto& s : text_keys())
        if (s.key == k) { needed = true; break; }
    if (!needed) return ATHD_OK;        // position_ids, the audio tower, ...: ignored
    HostT t;
    int64_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        if (shape[i] < 0 || shape[i] > ((int64_t)1 << 32)) return c->fail(ATHD_EINVAL, "bad shape for " + k);
        t.shape.push_back(shape[i]);
        n *= shape[i];
        if (n > ((int64_t)1 << 32)) return c->fail(ATHD_EINVAL, "bad shape for " + k);
    }
    t.v.assign((const float*)host, (const float*)host + n);
    c->host[k] = std::move(t);
    return ATHD_OK;
}

int athd_text_finalize(athd_text_ctx* c) {
    if (!c) return ATHD_EINVAL;
    if (c->finalized) return c->fail(ATHD_ESTATE, "already finalized");
    for (const auto& s : text_keys()) {
        auto it = c->host.find(s.key);
        if (it == c->host.end()) return c->fail(ATHD_EKEY, "missing weight: " + s.key);
        if (it->second.shape != s.shape) return c->fail(ATHD_EKEY, "shape mismatch for " + s.key);
    }
    if (hipSetDevice(c->device) != hipSuccess) return c->fail(ATHD_EHIP, "hipSetDevice failed");
    if (tt_init() != 0) return c->fail(ATHD_EHIP, "attention LDS limit could not be set");
    const bool bf = c->mode == ATHD_BF16;
    const size_t wsz = bf ? 2 : 4;
    size_t total = 0;
    size_t off = 0;
    bool ok = true;
    std::vector<uint16_t> tmp;
    bool dry = true;                    // first pass: sizes only
    auto put = [&](const void* src, size_t bytes) -> const void* {
        void* dst = dry ? nullptr : c->arena + off;
        off += align256(bytes);
        if (!dry && (off > total || hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) != hipSuccess)) ok = false;
        return dst;
    };
    auto f32 = [&](const std::string& k) { const HostT& t = c->host[k]; return (const float*)put(t.v.data(), t.v.size() * 4); };
    auto mat = [&](const std::vector<const std::vector<float>*>& parts) -> const void* {   // rows concatenated
        if (dry) {
            size_t n = 0;
            for (auto* p : parts) n += p->size();
            return put(nullptr, n * wsz);
        }
        if (!bf && parts.size() == 1) return put(parts[0]->data(), parts[0]->size() * 4);
        if (!bf) {
            std::vector<float> cat;
            for (auto* p : parts) cat.insert(cat.end(), p->begin(), p->end());
            return put(cat.data(), cat.size() * 4);
        }
        tmp.clear();
        for (auto* p : parts)
            for (float x : *p) tmp.push_back(f2bf_host(x));
        return put(tmp.data(), tmp.size() * 2);
    };
    auto lin = [&](const std::string& p, int N, int K) {
        Lin l;
        l.w = mat({&c->host[p + ".weight"].v});
        l.b = f32(p + ".bias");
        l.plan = tt_gemm_plan(N, K);
        if (!l.plan) ok = false;
        return l;
    };
    auto norm = [&](const std::string& p) { Norm n; n.w = f32(p + ".weight"); n.b = f32(p + ".bias"); return n; };
    auto pack = [&] {
    const std::string e = "text_model.embeddings.";
    c->word = f32(e + "word_embeddings.weight");
    c->pos = f32(e + "position_embeddings.weight");
    c->type0 = f32(e + "token_type_embeddings.weight");
    c->emb_ln = norm(e + "LayerNorm");
    for (int l = 0; l < TT_LAYERS; ++l) {
        const std::string p = "text_model.encoder.layer." + std::to_string(l) + ".";
        Layer& y = c->layer[l];
        const std::string a = p + "attention.self.";
        y.qkv.w = mat({&c->host[a + "query.weight"].v, &c->host[a + "key.weight"].v, &c->host[a + "value.weight"].v});
        std::vector<float> b3;
        for (const char* n : {"query.bias", "key.bias", "value.bias"}) {
            const auto& v = c->host[a + n].v;
            b3.insert(b3.end(), v.begin(), v.end());
        }
        y.qkv.b = (const float*)put(b3.data(), b3.size() * 4);
        y.qkv.plan = tt_gemm_plan(3 * TT_H, TT_H);
        if (!y.qkv.plan) ok = false;
        y.out = lin(p + "attention.output.dense", TT_H, TT_H);
        y.ln1 = norm(p + "attention.output.LayerNorm");
        y.ffn1 = lin(p + "intermediate.dense", TT_FFN, TT_H);
        y.ffn2 = lin(p + "output.dense", TT_H, TT_FFN);
        y.ln2 = norm(p + "output.LayerNorm");
    }
    c->pooler = lin("text_model.pooler.dense", TT_H, TT_H);
    c->lin1 = lin("text_projection.linear1", TT_PROJ, TT_H);
    c->lin2 = lin("text_projection.linear2", TT_PROJ, TT_PROJ);
    };
    pack();
    total = off;
    if (!ok) return c->fail(ATHD_EINVAL, "no GEMM plan for a tower shape");
    if (hipMalloc((void**)&c->arena, total) != hipSuccess) return c->fail(ATHD_EHIP, "hipMalloc of the packed weights failed");
    dry = false;
    off = 0;
    pack();
    if (!ok || hipDeviceSynchronize() != hipSuccess) {
        (void)hipFree(c->arena);
        c->arena = nullptr;
        return c->fail(ATHD_EHIP, "upload of the packed weights failed");
    }
    c->host.clear();
    c->finalized = true;
    return ATHD_OK;
}

size_t athd_text_workspace_bytes(athd_text_ctx* c, int P, int L) {
    if (!c || !dims_ok(P, L)) return 0;
    return ws_layout(P, L).total;
}

int athd_text_encode(athd_text_ctx* c, const int32_t* input_ids, const int32_t* attention_mask, int P, int L,
                     int normalize, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!c) return ATHD_EINVAL;
    if (!c->finalized) return c->fail(ATHD_ESTATE, "athd_text_encode before athd_text_finalize");
    if (!dims_ok(P, L)) return c->fail(ATHD_EINVAL, "P must be 1..256 and L 1..128");
    if (!input_ids || !attention_mask || !out || !workspace) return c->fail(ATHD_EINVAL, "null pointer");
    const Ws w = ws_layout(P, L);
    if (workspace_bytes < w.total) return c->fail(ATHD_EWORKSPACE, "workspace too small");
    if (((uintptr_t)workspace & 15) || ((uintptr_t)out & 15)) return c->fail(ATHD_EINVAL, "workspace and out must be 16-byte aligned");
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || (cur != c->device && hipSetDevice(c->device) != hipSuccess))
        return c->fail(ATHD_EHIP, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    unsigned char* base = (unsigned char*)workspace;
    float* x = (float*)(base + w.x);
    float* y = (float*)(base + w.y);
    float* h = (float*)(base + w.h);
    float* part = (float*)(base + w.part);
    const int M = P * L;
    const bool bf = c->mode == ATHD_BF16;
    int rc = 0;
#define TT_DO(call)                                                                   \
    do {                                                                              \
        rc = (call);                                                                  \
        if (rc != 0) return c->fail(ATHD_EHIP, std::string("launch failed: ") + #call); \
    } while (0)
    auto gemm = [&](const Lin& l, const float* X, int64_t ldx, int rows) {
        return tt_gemm_launch(bf, l.w, X, ldx, rows, *l.plan, part, st);
    };
    TT_DO(tt_embed_launch(input_ids, P, L, c->word, c->type0, c->pos, c->emb_ln.w, c->emb_ln.b, x, st));
    for (int l = 0; l < TT_LAYERS; ++l) {
        const Layer& y_ = c->layer[l];
        TT_DO(gemm(y_.qkv, x, TT_H, M));
        TT_DO(tt_attn_launch(part, y_.qkv.plan->S, y_.qkv.b, attention_mask, P, L, y, st));
        TT_DO(gemm(y_.out, y, TT_H, M));
        TT_DO(tt_ln_launch(part, y_.out.plan->S, M, y_.out.b, x, y_.ln1.w, y_.ln1.b, x, st));
        TT_DO(gemm(y_.ffn1, x, TT_H, M));
        TT_DO(tt_reduce_launch(part, y_.ffn1.plan->S, M, TT_FFN, y_.ffn1.b, nullptr, 0, TT_GELU, h, TT_FFN, st));
        TT_DO(gemm(y_.ffn2, h, TT_FFN, M));
        TT_DO(tt_ln_launch(part, y_.ffn2.plan->S, M, y_.ffn2.b, x, y_.ln2.w, y_.ln2.b, x, st));
    }
    // pooler and projection on the P first-token rows (row stride L * 768)
    TT_DO(gemm(c->pooler, x, (int64_t)L * TT_H, P));
    TT_DO(tt_reduce_launch(part, c->pooler.plan->S, P, TT_H, c->pooler.b, nullptr, 0, TT_TANH, y, TT_H, st));
    TT_DO(gemm(c->lin1, y, TT_H, P));
    TT_DO(tt_reduce_launch(part, c->lin1.plan->S, P, TT_PROJ, c->lin1.b, nullptr, 0, TT_RELU, h, TT_PROJ, st));
    TT_DO(gemm(c->lin2, h, TT_PROJ, P));
    TT_DO(tt_final_launch(part, c->lin2.plan->S, P, c->lin2.b, normalize != 0, out, st));
#undef TT_DO
    return ATHD_OK;
}

const char* athd_text_last_error(athd_text_ctx* c) { return c ? c->err.c_str() : ""; }

void athd_text_destroy(athd_text_ctx* c) {
    if (!c) return;
    if (c->arena) (void)hipFree(c->arena);
    delete c;
}

}  // extern "C"
