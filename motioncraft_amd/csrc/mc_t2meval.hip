// HumanML3D / KIT evaluation embedding model on the device: T2MContrastiveModel (mogen/models/rnns/t2m_bigru.py)
//   encode_motion   T2MMotionEncoder (:72-110): MovementConvEncoder (two Conv1d k=4 s=2 p=1 + LeakyReLU(0.2), Linear;
//                   :226-246) on motion[..., :-4], then MotionEncoderBiGRUCo (:249-282) with lengths // 4
//   encode_text     TextEncoderBiGRUCo (:186-223) on word vectors + pos_emb(one-hot)
// The convolutions are GEMMs over a zero-padded channels-last copy (row t of the im2col matrix is the contiguous
// 4 x C window starting at padded frame 2t: lda = 2C < K = 4C, one GEMM group per sample).  The GRU input products of
// all steps and both directions are one grouped GEMM; the recurrence is one grouped [B, H] x [H, 3H] GEMM + one gate
// kernel per step (both directions together).  A packed sequence = sample b is updated at steps s < len[b]; the
// reverse direction visits t = len[b]-1-s.
#include "mc_common.h"
#include "mc_gemm.h"
#include "mc_kernels.h"
#include "mc_enc.h"
#include "mc_params.h"
#include "../../include/motioncraft_amd.h"
#include <string>
#include <vector>

namespace {

// Y[b][0] = Y[b][T+1] = 0; Y[b][1+t][0:C] = X[b][t][0:C] (source rows of ldx floats), zero up to Cp
__global__ __launch_bounds__(256) void pad_time_k(const float* __restrict__ X, float* __restrict__ Y, int B, int T, int C, int ldx, int Cp) {
    const long n = (long)B * (T + 2) * Cp;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % Cp);
        const long r = i / Cp;
        const int t = (int)(r % (T + 2)) - 1, b = (int)(r / (T + 2));
        Y[i] = (t >= 0 && t < T && c < C) ? X[((long)b * T + t) * ldx + c] : 0.f;
    }
}

__global__ __launch_bounds__(256) void lrelu_k(float* __restrict__ X, long n, float slope) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float v = X[i];
        X[i] = v >= 0.f ? v : slope * v;
    }
}

// h[b][d][:] = hidden[d][:]
__global__ __launch_bounds__(256) void gru_init_k(const float* __restrict__ hidden, float* __restrict__ h, int B, int H) {
    const long n = (long)B * 2 * H;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) h[i] = hidden[i % (2 * H)];
}

// one recurrence step of both directions: gi [2][B*S][3H] (input products + b_ih), gh [B][2][3H] (W_hh h + b_hh), h [B][2][H]
__global__ __launch_bounds__(256) void gru_gate_k(const float* __restrict__ gi, const float* __restrict__ gh, float* __restrict__ h,
                                                  const int* __restrict__ lens, int len_div, int s, int B, int S, int H) {
    const long n = (long)B * 2 * H;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int j = (int)(i % H), d = (int)((i / H) % 2), b = (int)(i / (2L * H));
        int len = lens[b] / len_div;
        len = len > S ? S : len;
        if (s >= len) continue;
        const int t = d == 0 ? s : len - 1 - s;
        const float* a = gi + ((long)d * B * S + (long)b * S + t) * 3 * H;
        const float* g = gh + ((long)b * 2 + d) * 3 * H;
        const float r = 1.f / (1.f + expf(-(a[j] + g[j])));
        const float z = 1.f / (1.f + expf(-(a[H + j] + g[H + j])));
        const float nn = tanhf(a[2 * H + j] + r * g[2 * H + j]);
        h[i] = (1.f - z) * nn + z * h[i];
    }
}

struct Head {                        // input_emb + BiGRU + output_net
    int din = 0, hid = 0, dout = 0;
    const float *in_w = nullptr, *in_b = nullptr, *hidden = nullptr, *o0_w = nullptr, *o0_b = nullptr, *ln_g = nullptr, *ln_b = nullptr,
                *o3_w = nullptr, *o3_b = nullptr;
    float *wih = nullptr, *whh = nullptr, *bih = nullptr, *bhh = nullptr;      // [2][3H][H] / [2][3H], packed at finalize
};

int grid_for(long n) { return (int)std::min<long>(cdiv(n, 256), 4096); }

}  // namespace

struct mc_t2meval {
    mc_t2meval_config cfg;
    ParamStore params{"t2m evaluator"};           // derived: the heads' GRU weights packed per direction
    const float *c1_w = nullptr, *c1_b = nullptr, *c2_w = nullptr, *c2_b = nullptr, *mo_w = nullptr, *mo_b = nullptr;
    const float *pos_w = nullptr, *pos_b = nullptr;
    Head motion, text;
    int Cp = 0, Pp = 0;
    bool finalized = false, has_text = false;
    Workspace ws;
};

namespace {

int bind_head(ParamStore& ps, const std::string& pre, int din, int hid, int dout, Head& h) {
    int r;
    h.din = din; h.hid = hid; h.dout = dout;
    if ((r = ps.bind({{&h.in_w, pre + "input_emb.weight", (int64_t)hid * din}, {&h.in_b, pre + "input_emb.bias", hid},
                      {&h.hidden, pre + "hidden", 2 * hid},
                      {&h.o0_w, pre + "output_net.0.weight", (int64_t)hid * 2 * hid}, {&h.o0_b, pre + "output_net.0.bias", hid},
                      {&h.ln_g, pre + "output_net.1.weight", hid}, {&h.ln_b, pre + "output_net.1.bias", hid},
                      {&h.o3_w, pre + "output_net.3.weight", (int64_t)dout * hid}, {&h.o3_b, pre + "output_net.3.bias", dout}})))
        return r;
    const size_t wn = (size_t)3 * hid * hid, bn = (size_t)3 * hid;
    float** dst[4] = {&h.wih, &h.whh, &h.bih, &h.bhh};
    const char* base[4] = {"gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0"};
    for (int k = 0; k < 4; ++k) {
        const size_t n = k < 2 ? wn : bn;
        if ((r = ps.derived(2 * n, dst[k]))) return r;
        for (int d = 0; d < 2; ++d) {
            const float* src = nullptr;
            if ((r = ps.get(pre + base[k] + (d ? "_reverse" : ""), (int64_t)n, &src))) return r;
            MC_HIP(hipMemcpy(*dst[k] + d * n, src, n * sizeof(float), hipMemcpyDeviceToDevice));
        }
    }
    return MC_OK;
}

// recurrence steps [s0, s0 + steps) of both directions on h [B][2][H] in place: per step one grouped [B, H] x [H, 3H] GEMM into the
// scratch gh [B][2][3H] and the gate kernel.  whh [2][3H][H], bhh [2][3H]
int bigru_steps(const float* gi, const float* whh, const float* bhh, float* h, float* gh, const int* lens, int len_div, int B, int S,
                int H, int s0, int steps, hipStream_t s) {
    int r;
    GemmArgs q;                                        // gh[b][d] = h[b][d] W_hh[d]^T + b_hh[d]
    q.A = h; q.lda = 2 * H; q.a_gstride = H; q.W = whh; q.ldw = H; q.w_gstride = (long)3 * H * H; q.bias = bhh; q.b_gstride = 3 * H;
    q.C = gh; q.ldc = 6 * H; q.c_gstride = 3 * H; q.M = B; q.N = 3 * H; q.K = H;
    for (int st = s0; st < s0 + steps; ++st) {
        if ((r = mc_launch_gemm(GM_PLAIN, q, 2, 0, s))) return r;
        hipLaunchKernelGGL(gru_gate_k, dim3(grid_for((long)B * 2 * H)), dim3(256), 0, s, gi, gh, h, lens, len_div, st, B, S, H);
        MC_LAUNCH_CHECK();
    }
    return MC_OK;
}

// x [B*S][din] -> out [B][dout];  buf: emb [B*S][H] | gi [2][B*S][3H] | h [B][2H] | gh [B][6H] | y [B][H]
int run_head(const Head& p, const float* x, const int* lens, int len_div, int B, int S, float* buf, float* out, hipStream_t s) {
    const int H = p.hid;
    const long BS = (long)B * S;
    float* emb = buf;
    float* gi = emb + BS * H;
    float* h = gi + 2 * BS * 3 * H;
    float* gh = h + (long)B * 2 * H;
    float* y = gh + (long)B * 6 * H;
    int r;
    if ((r = mc_enc_dense(x, p.din, p.in_w, p.din, p.in_b, nullptr, 0, emb, H, BS, H, p.din, ACT_NONE, s))) return r;
    GemmArgs g;                                        // gi[d] = emb W_ih[d]^T + b_ih[d]
    g.A = emb; g.lda = H; g.W = p.wih; g.ldw = H; g.w_gstride = (long)3 * H * H; g.bias = p.bih; g.b_gstride = 3 * H;
    g.C = gi; g.ldc = 3 * H; g.c_gstride = BS * 3 * H; g.M = (int)BS; g.N = 3 * H; g.K = H;
    if ((r = mc_launch_gemm(GM_PLAIN, g, 2, 0, s))) return r;
    hipLaunchKernelGGL(gru_init_k, dim3(grid_for((long)B * 2 * H)), dim3(256), 0, s, p.hidden, h, B, H);
    MC_LAUNCH_CHECK();
    if ((r = bigru_steps(gi, p.whh, p.bhh, h, gh, lens, len_div, B, S, H, 0, S, s))) return r;
    if ((r = mc_enc_dense(h, 2 * H, p.o0_w, 2 * H, p.o0_b, nullptr, 0, y, H, B, H, 2 * H, ACT_NONE, s))) return r;
    if ((r = mc_enc_ln(y, p.ln_g, p.ln_b, y, B, H, 1e-5f, 0, s))) return r;
    hipLaunchKernelGGL(lrelu_k, dim3(grid_for((long)B * H)), dim3(256), 0, s, y, (long)B * H, 0.2f);
    MC_LAUNCH_CHECK();
    return mc_enc_dense(y, H, p.o3_w, H, p.o3_b, nullptr, 0, out, p.dout, B, p.dout, H, ACT_NONE, s);
}

// Conv1d(k = 4, s = 2, p = 1) + LeakyReLU(slope) over channels-last frames, T1 = (T - 2) / 2 + 1 outputs per sample.  xp != nullptr:
// x [B*T] rows of ldx floats, of which C are copied into the zero-padded xp [B][T + 2][Cp] first; xp == nullptr: x is that padded
// buffer already.  w tap-major [O][4][Cp].  pad_out: y is the padded input of a next convolution, [B][T1 + 2][O] with zero rows 0 and
// T1 + 1 (LeakyReLU keeps zeros: it runs over the whole buffer); else y [B][T1][O].
int conv_k4s2(const float* x, int ldx, int C, float* xp, const float* w, const float* bias, float* y, bool pad_out, int B, int T, int Cp,
              int O, float slope, hipStream_t s) {
    const int T1 = (T + 2 - 4) / 2 + 1;
    if (xp) {
        hipLaunchKernelGGL(pad_time_k, dim3(grid_for((long)B * (T + 2) * Cp)), dim3(256), 0, s, x, xp, B, T, C, ldx, Cp);
        MC_LAUNCH_CHECK();
    }
    const long yrows = pad_out ? T1 + 2 : T1, n_y = (long)B * yrows * O;
    if (pad_out) MC_HIP(hipMemsetAsync(y, 0, (size_t)n_y * sizeof(float), s));
    GemmArgs g;
    g.A = xp ? xp : x; g.lda = 2 * Cp; g.a_gstride = (long)(T + 2) * Cp; g.W = w; g.ldw = 4 * Cp; g.bias = bias;
    g.C = pad_out ? y + O : y; g.ldc = O; g.c_gstride = yrows * O; g.M = T1; g.N = O; g.K = 4 * Cp;
    if (int r = mc_launch_gemm(GM_PLAIN, g, B, 0, s)) return r;
    hipLaunchKernelGGL(lrelu_k, dim3(grid_for(n_y)), dim3(256), 0, s, y, n_y, slope);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

size_t head_floats(const Head& p, int B, int S) {
    return (size_t)B * S * p.hid * 7 + (size_t)B * p.hid * 9 + 64;
}

// host-side repack of an uploaded parameter: conv weight [O][C][4] -> tap-major [O][4][Cp]; pos_emb [O][P] -> [O][Pp]
std::vector<float> repack_conv(const float* w, int O, int C, int Cp) {
    std::vector<float> out((size_t)O * 4 * Cp, 0.f);
    for (int o = 0; o < O; ++o)
        for (int c = 0; c < C; ++c)
            for (int k = 0; k < 4; ++k) out[((size_t)o * 4 + k) * Cp + c] = w[((size_t)o * C + c) * 4 + k];
    return out;
}

}  // namespace

extern "C" {

int mc_t2meval_create(const mc_t2meval_config* cfg, mc_t2meval** out) {
    MC_REQUIRE(cfg && out, "null argument");
    MC_REQUIRE(cfg->input_size > 4 && cfg->movement_hidden % 4 == 0 && cfg->movement_latent % 4 == 0 && cfg->motion_hidden % 4 == 0 &&
                   cfg->motion_latent % 4 == 0,
               "t2m evaluator: motion widths must be multiples of 4");
    MC_REQUIRE(cfg->word_size == 0 || (cfg->word_size % 4 == 0 && cfg->text_hidden % 4 == 0 && cfg->text_out % 4 == 0 && cfg->pos_size >= 1),
               "t2m evaluator: text widths must be multiples of 4");
    mc_t2meval* e = new mc_t2meval();
    e->cfg = *cfg;
    e->Cp = (cfg->input_size - 4 + 3) / 4 * 4;
    e->Pp = (cfg->pos_size + 3) / 4 * 4;
    *out = e;
    return MC_OK;
}

void mc_t2meval_destroy(mc_t2meval* e) { delete e; }

int mc_op_bigru_steps(const float* gi, const float* whh, const float* bhh, float* h, const int32_t* lens, int32_t len_div, int32_t B,
                      int32_t S, int32_t H, int32_t s0, int32_t steps, void* stream) {
    MC_REQUIRE(gi && whh && bhh && h && lens && len_div >= 1 && B >= 1 && S >= 1 && H >= 4 && H % 4 == 0 && s0 >= 0 && steps >= 0,
               "bad bigru_steps args");
    hipStream_t s = (hipStream_t)stream;
    float* gh = nullptr;
    MC_HIP(hipMalloc((void**)&gh, sizeof(float) * (size_t)B * 6 * H));
    const int r = bigru_steps(gi, whh, bhh, h, gh, lens, len_div, B, S, H, s0, steps, s);
    (void)hipStreamSynchronize(s);
    (void)hipFree(gh);
    return r;
}

int mc_op_conv1d_k4s2(const float* x, int64_t ldx, const float* w_tapmajor, const float* bias, float* y_padded, int32_t B, int32_t T,
                      int32_t C, int32_t Cp, int32_t O, float slope, void* stream) {
    MC_REQUIRE(x && w_tapmajor && bias && y_padded && B >= 1 && T >= 2 && C >= 1 && ldx >= C && Cp >= C && Cp % 4 == 0 && O >= 4 &&
                   O % 4 == 0,
               "bad conv1d_k4s2 args");
    hipStream_t s = (hipStream_t)stream;
    float* xp = nullptr;
    MC_HIP(hipMalloc((void**)&xp, sizeof(float) * (size_t)B * (T + 2) * Cp));
    const int r = conv_k4s2(x, (int)ldx, C, xp, w_tapmajor, bias, y_padded, true, B, T, Cp, O, slope, s);
    (void)hipStreamSynchronize(s);
    (void)hipFree(xp);
    return r;
}

int mc_t2meval_set_param(mc_t2meval* e, const char* name, const float* host, int64_t numel) {
    MC_REQUIRE(e && name && host && numel > 0, "bad argument");
    const mc_t2meval_config& c = e->cfg;
    const std::string n = name;
    std::vector<float> packed;
    const int C = c.input_size - 4;
    if (n == "movement_encoder.main.0.weight") {
        MC_REQUIRE(numel == (int64_t)c.movement_hidden * C * 4, "t2m evaluator: %s has %ld elements", name, (long)numel);
        packed = repack_conv(host, c.movement_hidden, C, e->Cp);
    } else if (n == "movement_encoder.main.3.weight") {
        MC_REQUIRE(numel == (int64_t)c.movement_latent * c.movement_hidden * 4, "t2m evaluator: %s has %ld elements", name, (long)numel);
        packed = repack_conv(host, c.movement_latent, c.movement_hidden, c.movement_hidden);
    } else if (n == "text_encoder.pos_emb.weight") {
        MC_REQUIRE(numel == (int64_t)c.word_size * c.pos_size, "t2m evaluator: %s has %ld elements", name, (long)numel);
        packed.assign((size_t)c.word_size * e->Pp, 0.f);
        for (int o = 0; o < c.word_size; ++o)
            for (int k = 0; k < c.pos_size; ++k) packed[(size_t)o * e->Pp + k] = host[(size_t)o * c.pos_size + k];
    }
    if (!packed.empty()) { host = packed.data(); numel = (int64_t)packed.size(); }
    const int r = e->params.set(n, host, numel);
    if (r == MC_OK) e->finalized = false;
    return r;
}

int mc_t2meval_finalize(mc_t2meval* e) {
    MC_REQUIRE(e, "null evaluator");
    e->finalized = false;
    ParamStore& ps = e->params;
    ps.clear_derived();
    const mc_t2meval_config& c = e->cfg;
    int r;
    if ((r = ps.bind({{&e->c1_w, "movement_encoder.main.0.weight", (int64_t)c.movement_hidden * 4 * e->Cp},
                      {&e->c1_b, "movement_encoder.main.0.bias", c.movement_hidden},
                      {&e->c2_w, "movement_encoder.main.3.weight", (int64_t)c.movement_latent * 4 * c.movement_hidden},
                      {&e->c2_b, "movement_encoder.main.3.bias", c.movement_latent},
                      {&e->mo_w, "movement_encoder.out_net.weight", (int64_t)c.movement_latent * c.movement_latent},
                      {&e->mo_b, "movement_encoder.out_net.bias", c.movement_latent}})))
        return r;
    if ((r = bind_head(ps, "motion_encoder.", c.movement_latent, c.motion_hidden, c.motion_latent, e->motion))) return r;
    e->has_text = false;
    if (c.word_size > 0 && ps.has("text_encoder.pos_emb.weight")) {
        if ((r = ps.bind({{&e->pos_w, "text_encoder.pos_emb.weight", (int64_t)c.word_size * e->Pp},
                          {&e->pos_b, "text_encoder.pos_emb.bias", c.word_size}})) ||
            (r = bind_head(ps, "text_encoder.", c.word_size, c.text_hidden, c.text_out, e->text)))
            return r;
        e->has_text = true;
    }
    e->finalized = true;
    return MC_OK;
}

int mc_t2meval_encode_motion(mc_t2meval* e, const float* motion, const int32_t* lengths, int32_t B, int32_t T, float* out, void* stream) {
    MC_REQUIRE(e && motion && lengths && out && B >= 1 && T >= 4, "bad argument");
    MC_REQUIRE(e->finalized, "t2m evaluator not finalized");
    const mc_t2meval_config& c = e->cfg;
    hipStream_t s = (hipStream_t)stream;
    const int C = c.input_size - 4, Cp = e->Cp, Hm = c.movement_hidden, Lm = c.movement_latent;
    const int T1 = (T + 2 - 4) / 2 + 1, T2 = (T1 + 2 - 4) / 2 + 1;
    MC_REQUIRE(T2 >= 1, "t2m evaluator: %d frames are too few", T);
    const size_t n_pad1 = (size_t)B * (T + 2) * Cp + 4 * Cp, n_pad2 = (size_t)B * (T1 + 2) * Hm + 4 * Hm, n_c2 = (size_t)B * T2 * Lm;
    int r;
    if ((r = e->ws.ensure(n_pad1 + n_pad2 + 2 * n_c2 + head_floats(e->motion, B, T2) + 64, s))) return r;
    float* pad1 = e->ws.buf;
    float* pad2 = pad1 + n_pad1;
    float* c2 = pad2 + n_pad2;
    float* mov = c2 + n_c2;
    float* buf = mov + n_c2;
    // conv 1 -> rows 1 .. T1 of the padded buffer of conv 2; conv 2 -> c2
    if ((r = conv_k4s2(motion, c.input_size, C, pad1, e->c1_w, e->c1_b, pad2, true, B, T, Cp, Hm, 0.2f, s))) return r;
    if ((r = conv_k4s2(pad2, Hm, Hm, nullptr, e->c2_w, e->c2_b, c2, false, B, T1, Hm, Lm, 0.2f, s))) return r;
    if ((r = mc_enc_dense(c2, Lm, e->mo_w, Lm, e->mo_b, nullptr, 0, mov, Lm, (long)B * T2, Lm, Lm, ACT_NONE, s))) return r;
    return run_head(e->motion, mov, lengths, 4, B, T2, buf, out, s);
}

int mc_t2meval_encode_text(mc_t2meval* e, const float* word_emb, const float* pos_onehot, const int32_t* sent_len, int32_t B, int32_t S,
                           float* out, void* stream) {
    MC_REQUIRE(e && word_emb && pos_onehot && sent_len && out && B >= 1 && S >= 1, "bad argument");
    MC_REQUIRE(e->finalized, "t2m evaluator not finalized");
    MC_REQUIRE(e->has_text, "t2m evaluator: no text_encoder.* weights were loaded");
    const mc_t2meval_config& c = e->cfg;
    hipStream_t s = (hipStream_t)stream;
    const long BS = (long)B * S;
    int r;
    if ((r = e->ws.ensure((size_t)BS * c.word_size + head_floats(e->text, B, S) + 64, s))) return r;
    float* x = e->ws.buf;
    GemmArgs g;                                        // x = word_emb + pos_emb(pos_onehot)   (K = pos_size: unaligned rows)
    g.A = pos_onehot; g.lda = c.pos_size; g.W = e->pos_w; g.ldw = e->Pp; g.bias = e->pos_b; g.R = word_emb; g.ldr = c.word_size;
    g.C = x; g.ldc = c.word_size; g.M = (int)BS; g.N = c.word_size; g.K = c.pos_size;
    if ((r = mc_launch_gemm(GM_ENC, g, 1, 0, s))) return r;
    return run_head(e->text, x, sent_len, 1, B, S, x + BS * c.word_size, out, s);
}

}  // extern "C"
