// Evaluation embedding model on the device: T2MContrastiveModel_SMPLX
//   encode_motion   ActorAgnosticEncoder: skel_embedding -> [mu_token, logvar_token, frames] + sinusoid table ->
//                   post-LN nn.TransformerEncoder with the length mask as key-padding mask -> row 0 (mu = .loc)
//                                                                mogen/models/rnns/t2m_bigru_smplx.py:66-195,404-410
//   encode_text     DistilbertActorAgnosticEncoder after tokenisation: DistilBERT (embeddings LN, post-LN layers, eps
//                   1e-12, attention mask) -> ReLU -> Linear -> the same token/transformer tail
//                                                                mogen/models/rnns/t2m_bigru_smplx.py:198-394,412-414
// Both run on the generic encoder-layer schedule of mc_enc.h (fp32 MFMA GEMMs + masked streaming attention).
#include "mc_common.h"
#include "mc_gemm.h"
#include "mc_kernels.h"
#include "mc_enc.h"
#include "mc_params.h"
#include "../../include/motioncraft_amd.h"
#include <string>
#include <vector>

namespace {

// xs[b][0] = mu_token + pe[0]; xs[b][1] = logvar_token + pe[1]; xs[b][2 + t] = rows[b][t] (pe already added by the GEMM)
// valid[b][0..1] = 1; valid[b][2 + t] = t < lengths[b]  (or mask_in[b][t])
__global__ __launch_bounds__(256) void assemble_tokens_k(const float* __restrict__ rows, const float* __restrict__ mu_tok,
                                                         const float* __restrict__ lv_tok, const float* __restrict__ pe,
                                                         const int* __restrict__ lengths, const uint8_t* __restrict__ mask_in,
                                                         float* __restrict__ xs, uint8_t* __restrict__ valid, int B, int S, int d) {
    const int S2 = S + 2, d4 = d >> 2;
    const long n = (long)B * S2 * d4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % d4) * 4;
        const long r = i / d4;
        const int b = (int)(r / S2), t = (int)(r % S2);
        f32x4 v;
        if (t < 2) {
            const f32x4 tk = *reinterpret_cast<const f32x4*>((t == 0 ? mu_tok : lv_tok) + c);
            const f32x4 p = *reinterpret_cast<const f32x4*>(pe + (long)t * d + c);
            v = f32x4{tk[0] + p[0], tk[1] + p[1], tk[2] + p[2], tk[3] + p[3]};
        } else {
            v = *reinterpret_cast<const f32x4*>(rows + ((long)b * S + (t - 2)) * d + c);
        }
        *reinterpret_cast<f32x4*>(xs + r * d + c) = v;
        if (c == 0) valid[r] = t < 2 ? 1 : (lengths ? (uint8_t)((t - 2) < lengths[b]) : (uint8_t)(mask_in[(long)b * S + (t - 2)] != 0));
    }
}

__global__ __launch_bounds__(256) void relu_k(const float* __restrict__ X, float* __restrict__ Y, long n4) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const f32x4 v = reinterpret_cast<const f32x4*>(X)[i];
        reinterpret_cast<f32x4*>(Y)[i] = f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
    }
}

struct Tail {                       // mu/logvar tokens + sinusoid table + seqTransEncoder
    const float *mu = nullptr, *lv = nullptr, *pe = nullptr;
    std::vector<EncLayer> layers;
};

}  // namespace

struct mc_evalenc {
    mc_evalenc_config cfg;
    ParamStore params{"evaluation encoder"};      // derived: the padded skel_w and DistilBERT's stacked q | k | v
    Tail motion, text;
    const float *skel_w = nullptr, *skel_b = nullptr;        // skel_w zero padded to [d][Cp]
    const float *tok = nullptr, *pos = nullptr, *eln_g = nullptr, *eln_b = nullptr, *proj_w = nullptr, *proj_b = nullptr;
    std::vector<EncLayer> bert;
    int Cp = 0;
    bool finalized = false, has_text = false;
    Workspace ws;
};

namespace {

int bind_tail(ParamStore& ps, const mc_evalenc_config& c, const std::string& pre, Tail& t) {
    const int d = c.latent_dim;
    int r;
    if ((r = ps.bind({{&t.mu, pre + "mu_token", d}, {&t.lv, pre + "logvar_token", d},
                      {&t.pe, pre + "sequence_pos_encoding.pe", (int64_t)c.pe_len * d}})))
        return r;
    t.layers.assign(c.num_layers, EncLayer());
    for (int i = 0; i < c.num_layers; ++i)
        if ((r = bind_enc_layer(ps, pre + "seqTransEncoder.layers." + std::to_string(i) + ".", ENC_TORCH, d, c.ff_size, t.layers[i])))
            return r;
    return MC_OK;
}

// rows [B*S][d] (pe already added) -> tokens + transformer -> mu_out [B][d]
int run_tail(mc_evalenc* e, const Tail& t, const float* rows_in, const int* lengths, const uint8_t* mask_in, int B, int S,
             float* buf, float* mu_out, hipStream_t s) {
    const mc_evalenc_config& c = e->cfg;
    const int d = c.latent_dim, ff = c.ff_size, S2 = S + 2;
    const long rows = (long)B * S2;
    float* xs = buf;
    float* qkv = xs + rows * d;
    float* att = qkv + rows * 3 * d;
    float* y = att + rows * d;
    float* hid = y + rows * d;
    uint8_t* valid = reinterpret_cast<uint8_t*>(hid + rows * ff);
    hipLaunchKernelGGL(assemble_tokens_k, dim3((unsigned)std::min<long>(cdiv(rows * (d / 4), 256), 4096)), dim3(256), 0, s, rows_in,
                       t.mu, t.lv, t.pe, lengths, mask_in, xs, valid, B, S, d);
    MC_LAUNCH_CHECK();
    int r;
    for (int i = 0; i < c.num_layers; ++i)
        if ((r = mc_enc_layer(t.layers[i], xs, qkv, att, y, hid, rows, B, S2, d, c.num_heads, ff, false, ACT_GELU, 0, valid, 1e-5f, s)))
            return r;
    MC_HIP(hipMemcpy2DAsync(mu_out, (size_t)d * sizeof(float), xs, (size_t)S2 * d * sizeof(float), (size_t)d * sizeof(float), B,
                            hipMemcpyDeviceToDevice, s));
    return MC_OK;
}

size_t tail_floats(const mc_evalenc_config& c, int B, int S) {
    const size_t rows = (size_t)B * (S + 2);
    return rows * (size_t)(c.latent_dim * 6 + c.ff_size) + rows / 4 + 64;
}

}  // namespace

extern "C" {

int mc_evalenc_create(const mc_evalenc_config* cfg, mc_evalenc** out) {
    MC_REQUIRE(cfg && out, "null argument");
    MC_REQUIRE(cfg->nfeats >= 1 && cfg->num_layers >= 1 && cfg->latent_dim == cfg->num_heads * 64 && cfg->ff_size % 4 == 0,
               "evaluation encoder: latent_dim=%d with %d heads unsupported (head_dim must be 64)", cfg->latent_dim, cfg->num_heads);
    MC_REQUIRE(cfg->bert_dim == 0 || (cfg->bert_dim == cfg->bert_heads * 64 && cfg->bert_ff % 4 == 0 && cfg->bert_layers >= 1),
               "evaluation encoder: DistilBERT width %d with %d heads unsupported (head_dim must be 64)", cfg->bert_dim, cfg->bert_heads);
    MC_REQUIRE(cfg->pe_len >= 3, "evaluation encoder: pe_len=%d", cfg->pe_len);
    mc_evalenc* e = new mc_evalenc();
    e->cfg = *cfg;
    e->Cp = (cfg->nfeats + 3) / 4 * 4;
    *out = e;
    return MC_OK;
}

void mc_evalenc_destroy(mc_evalenc* e) { delete e; }

int mc_evalenc_set_param(mc_evalenc* e, const char* name, const float* host, int64_t numel) {
    MC_REQUIRE(e && name && host && numel > 0, "bad argument");
    const int r = e->params.set(name, host, numel);
    if (r == MC_OK) e->finalized = false;
    return r;
}

int mc_evalenc_finalize(mc_evalenc* e) {
    MC_REQUIRE(e, "null encoder");
    e->finalized = false;
    ParamStore& ps = e->params;
    ps.clear_derived();
    const mc_evalenc_config& c = e->cfg;
    const int d = c.latent_dim;
    int r;
    const float* w = nullptr;
    if ((r = ps.bind({{&w, "motionencoder.skel_embedding.weight", (int64_t)d * c.nfeats},
                      {&e->skel_b, "motionencoder.skel_embedding.bias", d}})))
        return r;
    if (e->Cp != c.nfeats) {                                   // GEMM rows are read 16 bytes at a time
        float* wp = nullptr;
        if ((r = ps.derived((size_t)d * e->Cp, &wp))) return r;
        MC_HIP(hipMemset(wp, 0, (size_t)d * e->Cp * sizeof(float)));
        MC_HIP(hipMemcpy2D(wp, (size_t)e->Cp * sizeof(float), w, (size_t)c.nfeats * sizeof(float), (size_t)c.nfeats * sizeof(float), d,
                           hipMemcpyDeviceToDevice));
        w = wp;
    }
    e->skel_w = w;
    if ((r = bind_tail(ps, c, "motionencoder.", e->motion))) return r;
    e->has_text = false;
    if (c.bert_dim > 0 && ps.has("textencoder.projection.1.weight")) {
        const int bw = c.bert_dim;
        const std::string t = "textencoder.text_model.";
        if ((r = ps.bind({{&e->tok, t + "embeddings.word_embeddings.weight", (int64_t)c.bert_vocab * bw},
                          {&e->pos, t + "embeddings.position_embeddings.weight", (int64_t)c.bert_max_pos * bw},
                          {&e->eln_g, t + "embeddings.LayerNorm.weight", bw}, {&e->eln_b, t + "embeddings.LayerNorm.bias", bw}})))
            return r;
        e->bert.assign(c.bert_layers, EncLayer());
        for (int i = 0; i < c.bert_layers; ++i)
            if ((r = bind_enc_layer(ps, t + "transformer.layer." + std::to_string(i) + ".", ENC_DISTILBERT, bw, c.bert_ff, e->bert[i])))
                return r;
        if ((r = ps.bind({{&e->proj_w, "textencoder.projection.1.weight", (int64_t)d * bw},
                          {&e->proj_b, "textencoder.projection.1.bias", d}})) ||
            (r = bind_tail(ps, c, "textencoder.", e->text)))
            return r;
        e->has_text = true;
    }
    e->finalized = true;
    return MC_OK;
}

int mc_evalenc_encode_motion(mc_evalenc* e, const float* motion, const int32_t* lengths, int32_t B, int32_t T, float* mu_out,
                             void* stream) {
    MC_REQUIRE(e && motion && lengths && mu_out && B >= 1 && T >= 1, "bad argument");
    MC_REQUIRE(e->finalized, "evaluation encoder not finalized");
    const mc_evalenc_config& c = e->cfg;
    MC_REQUIRE(T + 2 <= c.pe_len, "evaluation encoder: %d frames exceed the positional table (%d)", T, c.pe_len);
    hipStream_t s = (hipStream_t)stream;
    const int d = c.latent_dim, Cp = e->Cp;
    const long rows = (long)B * T;
    int r;
    const size_t head = (size_t)rows * (Cp + d) + 64;
    if ((r = e->ws.ensure(head + tail_floats(c, B, T), s))) return r;
    float* pad = e->ws.buf;
    float* emb = pad + rows * Cp;
    const float* A = motion;
    if (Cp != c.nfeats) {
        if ((r = mc_launch_pad_rows(motion, pad, rows, c.nfeats, Cp, s))) return r;
        A = pad;
    }
    GemmArgs g;                                       // emb[(b,t)] = skel_embedding(motion[b][t]) + pe[2 + t]
    g.A = A; g.lda = Cp; g.W = e->skel_w; g.ldw = Cp; g.bias = e->skel_b; g.C = emb; g.ldc = d;
    g.M = (int)rows; g.N = d; g.K = Cp; g.act = ACT_NONE;
    g.add = e->motion.pe + 2 * d; g.add_mod = T; g.ld_add = d;
    if ((r = mc_launch_gemm(GM_ENC, g, 1, 0, s))) return r;
    return run_tail(e, e->motion, emb, lengths, nullptr, B, T, e->ws.buf + head, mu_out, s);
}

int mc_evalenc_encode_text(mc_evalenc* e, const int32_t* ids, const uint8_t* mask, int32_t B, int32_t S, float* mu_out, void* stream) {
    MC_REQUIRE(e && ids && mask && mu_out && B >= 1 && S >= 1, "bad argument");
    MC_REQUIRE(e->finalized, "evaluation encoder not finalized");
    MC_REQUIRE(e->has_text, "evaluation encoder: no textencoder.* weights were loaded");
    const mc_evalenc_config& c = e->cfg;
    MC_REQUIRE(S <= c.bert_max_pos && S + 2 <= c.pe_len, "evaluation encoder: %d tokens exceed the position tables", S);
    hipStream_t s = (hipStream_t)stream;
    const int d = c.latent_dim, w = c.bert_dim, bf = c.bert_ff;
    const long rows = (long)B * S;
    int r;
    const size_t head = (size_t)rows * (w * 6 + bf + d) + 64;
    if ((r = e->ws.ensure(head + tail_floats(c, B, S), s))) return r;
    float* x = e->ws.buf;
    float* qkv = x + rows * w;
    float* att = qkv + rows * 3 * w;
    float* y = att + rows * w;
    float* hid = y + rows * w;
    float* emb = hid + rows * bf;
    if ((r = mc_enc_embed_tokens(ids, e->tok, e->pos, x, rows, S, w, c.bert_vocab, s))) return r;
    if ((r = mc_enc_ln(x, e->eln_g, e->eln_b, x, rows, w, 1e-12f, 0, s))) return r;
    for (int i = 0; i < c.bert_layers; ++i)
        if ((r = mc_enc_layer(e->bert[i], x, qkv, att, y, hid, rows, B, S, w, c.bert_heads, bf, false, ACT_GELU, 0, mask, 1e-12f, s)))
            return r;
    hipLaunchKernelGGL(relu_k, dim3((unsigned)std::min<long>(cdiv(rows * (w / 4), 256), 4096)), dim3(256), 0, s, x, y, rows * (w / 4));
    MC_LAUNCH_CHECK();
    GemmArgs g;                                       // emb[(b,j)] = projection(relu(h[b][j])) + pe[2 + j]
    g.A = y; g.lda = w; g.W = e->proj_w; g.ldw = w; g.bias = e->proj_b; g.C = emb; g.ldc = d;
    g.M = (int)rows; g.N = d; g.K = w; g.act = ACT_NONE;
    g.add = e->text.pe + 2 * d; g.add_mod = S; g.ld_add = d;
    if ((r = mc_launch_gemm(GM_ENC, g, 1, 0, s))) return r;
    return run_tail(e, e->text, emb, nullptr, mask, B, S, e->ws.buf + head, mu_out, s);
}

}  // extern "C"
