// Host side of libmotioncraft_amd.so (C-ABI declared in include/motioncraft_amd.h): weight binding, the runtime option table, context
// create / destroy and workspace allocation, the hipGraph capture and every extern "C" entry point.  The per-step kernel schedule they
// call into is mc_step.hip; the model / context structs are in mc_ctx.h.
#include "mc_ctx.h"

#include <cstring>

namespace {

template <class T>
int ws_alloc(mc_ctx* c, T** p, size_t n) {
    void* d = nullptr;
    size_t bytes = (n * sizeof(T) + 255) & ~(size_t)255;
    if (bytes == 0) bytes = 256;
    MC_HIP(hipMalloc(&d, bytes));
    c->allocs.push_back(d);
    c->bytes += (int64_t)bytes;
    *p = (T*)d;
    return MC_OK;
}

int bind_moe(const mc_model* m, const std::string& pre, int din, int dout, int seq_rows, MoeW* w) {
    const int64_t E = m->cfg.num_experts;
    w->din = din;
    w->dout = dout;
    return m->params.bind({{&w->emb, pre + "emb", (int64_t)seq_rows * din},       {&w->gate_w, pre + "gate_w", 256 * din},
                           {&w->gate_b, pre + "gate_b", 256},                      {&w->sim_n, pre + "sim_n", 256 * E},
                           {&w->sim_nT, pre + "sim_nT", 32 * 256},                 {&w->scale, pre + "scale", 1},
                           {&w->fc1_w, pre + "fc1_w", E * 4 * din * din},          {&w->fc1_b, pre + "fc1_b", E * 4 * din},
                           {&w->fc2_wt, pre + "fc2_wt", E * din * 4 * din},        {&w->fc2_b, pre + "fc2_b", E * din},
                           {&w->proj_w, pre + "proj_w", (int64_t)dout * din},      {&w->proj_b, pre + "proj_b", dout}});
}

int bind_weights(mc_ctx* c) {
    const mc_model* m = c->m;
    const ParamStore& ps = m->params;
    const mc_model_config& g = m->cfg;
    const int L = g.latent_dim, H = g.num_parts, D = L * H, F = g.ffn_dim, Te = g.time_embed_dim, C = g.input_feats;
    const int64_t DD = (int64_t)D * D;
    int r;
    if ((r = ps.bind({{&c->enc_w, "enc.w", (int64_t)D * m->Cp},                 {&c->enc_b, "enc.b", D},
                      {&c->seq_emb, "seq_emb", (int64_t)g.max_seq_len * D},
                      {&c->time_w0, "time.w0", (int64_t)Te * D},                {&c->time_b0, "time.b0", Te},
                      {&c->time_w2, "time.w2", (int64_t)Te * Te},               {&c->time_b2, "time.b2", Te},
                      {&c->dec_w, "dec.w", (int64_t)C * D},                     {&c->dec_b, "dec.b", C}})))
        return r;
    if (ps.has("dec.wf") && ps.has("dec.bf")) {
        if ((r = ps.bind({{&c->dec_wf, "dec.wf", (int64_t)C * D}, {&c->dec_bf, "dec.bf", C}}))) return r;
    }
    c->NLA = g.num_layers + g.num_ctrl_layers;
    c->lw.resize(c->NLA);
    if (g.num_ctrl_layers > 0) {
        const int64_t n = (int64_t)D * ((g.ctrl_cond_feats + 3) / 4 * 4);
        if ((r = ps.bind({{&c->ctrl_in_w, "ctrl_in.w", n}, {&c->ctrl_in_b, "ctrl_in.b", D}}))) return r;
    }
    for (int i = 0; i < c->NLA; ++i) {
        LayerW& w = c->lw[i];
        const bool is_ctrl = i >= g.num_layers;
        const std::string p = (is_ctrl ? "c" + std::to_string(i - g.num_layers) : "l" + std::to_string(i)) + ".";
        if (is_ctrl) {
            if (i == g.num_layers && (r = ps.bind({{&w.before_w, p + "before_w", DD}, {&w.before_b, p + "before_b", D}}))) return r;
            if ((r = ps.bind({{&w.after_w, p + "after_w", DD}, {&w.after_b, p + "after_b", D}}))) return r;
        }
        if ((r = ps.bind({{&w.norm_g, p + "norm.g", L},                         {&w.norm_b, p + "norm.b", L},
                          {&w.tnorm_g, p + "text_norm.g", g.text_latent_dim},   {&w.tnorm_b, p + "text_norm.b", g.text_latent_dim},
                          {&w.wsm, p + "body_wsm", H * H}})))
            return r;
        if ((r = bind_moe(m, p + "mm.", L, 4 * L, g.max_seq_len * H, &w.mm))) return r;
        if ((r = bind_moe(m, p + "tm.", g.text_latent_dim, 2 * L, g.max_text_len, &w.tm))) return r;
        if ((r = ps.bind({{&w.dyn_g, p + "dyn.norm.g", L},                      {&w.dyn_b, p + "dyn.norm.b", L},
                          {&w.qkv_w, p + "dyn.qkv_w", 3 * L * L},               {&w.qkv_b, p + "dyn.qkv_b", 3 * L},
                          {&w.ca_film_w, p + "ca.film_w", (int64_t)2 * D * Te}, {&w.ca_film_b, p + "ca.film_b", 2 * D},
                          {&w.ca_ln_g, p + "ca.ln_g", D},                       {&w.ca_ln_b, p + "ca.ln_b", D},
                          {&w.ca_out_w, p + "ca.out_w", DD},                    {&w.ca_out_b, p + "ca.out_b", D},
                          {&w.ffn_w1, p + "ffn.w1", (int64_t)H * F * L},        {&w.ffn_b1, p + "ffn.b1", H * F},
                          {&w.ffn_w2, p + "ffn.w2", (int64_t)H * L * F},        {&w.ffn_b2, p + "ffn.b2", H * L},
                          {&w.ffn_film_w, p + "ffn.film_w", (int64_t)2 * D * Te}, {&w.ffn_film_b, p + "ffn.film_b", 2 * D},
                          {&w.ffn_ln_g, p + "ffn.ln_g", D},                     {&w.ffn_ln_b, p + "ffn.ln_b", D},
                          {&w.ffn_out_w, p + "ffn.out_w", DD},                  {&w.ffn_out_b, p + "ffn.out_b", D}})))
            return r;
    }
    return MC_OK;
}

// context-only derived weights (bind_weights itself is a pure lookup / validation pass, also run by mc_model_finalize):
// [2][C][D] = dec_w | dec_wf and [2][C] = dec_bf | 0 -- the folded decoder tail as ONE grouped GEMM
int build_ctx_weights(mc_ctx* c) {
    if (!c->dec_wf) return MC_OK;
    const mc_model_config& g = c->m->cfg;
    const int D = g.latent_dim * g.num_parts;
    const size_t wn = (size_t)g.input_feats * D, bn = (size_t)g.input_feats;
    int rr;
    if ((rr = ws_alloc(c, &c->dec_cat_w, 2 * wn)) != MC_OK || (rr = ws_alloc(c, &c->dec_cat_b, 2 * bn)) != MC_OK) return rr;
    MC_HIP(hipMemcpy(c->dec_cat_w, c->dec_w, wn * sizeof(float), hipMemcpyDeviceToDevice));
    MC_HIP(hipMemcpy(c->dec_cat_w + wn, c->dec_wf, wn * sizeof(float), hipMemcpyDeviceToDevice));
    MC_HIP(hipMemcpy(c->dec_cat_b, c->dec_bf, bn * sizeof(float), hipMemcpyDeviceToDevice));
    MC_HIP(hipMemset(c->dec_cat_b + bn, 0, bn * sizeof(float)));
    return MC_OK;
}

// fp16 hi / lo planes of weight `name` ([rows][K] fp32 on the device), built once per model; chain = K axis stored in the
// chain-permuted order of mc_half.h (second GEMM of the fused MLP)
int half_weight(mc_model* m, const std::string& name, long rows, int K, bool chain, HalfW* out) {
    // the plane cache belongs to the MODEL and is filled from per-context calls (mc_ctx_set_precision): one lock per model, so two
    // contexts switching precision from two threads build each plane once
    std::lock_guard<std::mutex> lock(m->half_mu);
    auto it = m->half.find(name);
    if (it != m->half.end()) { *out = it->second; return MC_OK; }
    const float* src = nullptr;
    int r = m->params.get(name, (int64_t)rows * K, &src);
    if (r != MC_OK) return r;
    mc_half* hi = nullptr;
    MC_HIP(hipMalloc((void**)&hi, sizeof(mc_half) * 2 * (size_t)rows * K));
    mc_half* lo = hi + (size_t)rows * K;
    r = chain ? mc_launch_split_f16_chainperm(src, hi, lo, rows, K, nullptr) : mc_launch_split_f16(src, hi, lo, rows * K, nullptr);
    if (r != MC_OK) { (void)hipFree(hi); return r; }
    MC_HIP(hipStreamSynchronize(nullptr));
    const HalfW h{hi, lo};
    m->half[name] = h;
    m->half_bytes += sizeof(mc_half) * 2 * (size_t)rows * K;
    *out = h;
    return MC_OK;
}

int bind_half_weights(mc_ctx* c) {
    mc_model* m = c->m;
    const mc_model_config& g = m->cfg;
    const int L = g.latent_dim, H = g.num_parts, D = L * H, F = g.ffn_dim, E = g.num_experts;
    int r;
    for (int i = 0; i < c->NLA; ++i) {
        LayerW& w = c->lw[i];
        const bool is_ctrl = i >= g.num_layers;
        const std::string p = (is_ctrl ? "c" + std::to_string(i - g.num_layers) : "l" + std::to_string(i)) + ".";
        if (D % 128 == 0) {
            if ((r = half_weight(m, p + "ca.out_w", D, D, false, &w.h_ca_out))) return r;
            if ((r = half_weight(m, p + "ffn.out_w", D, D, false, &w.h_ffn_out))) return r;
            if (is_ctrl && (r = half_weight(m, p + "after_w", D, D, false, &w.h_after))) return r;
        }
        if (mc_mlp_h_supported(L, 4 * L)) {
            if ((r = half_weight(m, p + "mm.proj_w", 4 * L, L, false, &w.h_proj))) return r;
            if ((r = half_weight(m, p + "dyn.qkv_w", 3 * L, L, true, &w.h_qkv))) return r;
            if ((r = half_weight(m, p + "mm.fc1_w", (long)E * 4 * L, L, false, &w.h_fc1))) return r;
            if ((r = half_weight(m, p + "mm.fc2_wt", (long)E * L, 4 * L, true, &w.h_fc2))) return r;
        }
        if (mc_mlp_h_supported(L, F)) {
            if ((r = half_weight(m, p + "ffn.w1", (long)H * F, L, false, &w.h_w1))) return r;
            if ((r = half_weight(m, p + "ffn.w2", (long)H * L, F, true, &w.h_w2))) return r;
        }
    }
    return MC_OK;
}

// The largest grid any routing call of this context can launch cooperatively (mc_ctx_create and mc_ctx_set_option("route_coop") share
// it): the motion MoE routes N tokens, the text MoE (mc_ctx_set_condition) Ntxt -- either may be the one inside route_coop_k's size
// range; sizes in the one-workgroup regime or beyond the kernel's range need nothing.  Counted at 10 pairs per thread, the larger of
// the two grids the launch may pick.
int coop_grid_needed(const mc_ctx* c) {
    int nwg = 0;
    for (long n : {c->N, c->Ntxt})
        if (!mc_route_is_small(c->opt, n) && mc_route_coop_wgs(n) > nwg) nwg = mc_route_coop_wgs(n);
    return nwg;
}

// ---- runtime options: one row per option (key, variable, alternative variable read when the first is unset, field, built-in
// default, validity check: "" = valid, else why not).  The check runs on mc_ctx_set_option and on every environment value; the docs
// (include/motioncraft_amd.h, NativeContext.set_option) list the same keys and defaults.
struct OptionDef {
    const char *key, *env, *env_alt;
    long McOptions::*field;
    long dflt;
    std::string (*check)(long v);
    int (*hook)(mc_ctx* c, long& v);      // mc_ctx_set_option only, before the store (c->opt still holds the old value); may adjust v
};

std::string check_chain(long v) {
    const long bad = v & ~kChainDefault;
    const int b = bad ? __builtin_ctzl((unsigned long)bad) : 0;
    return !bad ? "" : "chain bit " + std::to_string(b) + (b < kChainBits ? " is retired (DESIGN.md section 5)" : " is not defined");
}
std::string check_tune(long v) {
    const long bad = v & ~(long)kTuneBits;      // (v < 0: the sign bits)
    return !bad ? "" : v < 0 ? "gemm_tune: a bit mask (>= 0)" : "gemm_tune bit " + std::to_string(__builtin_ctzl(bad)) + " is not defined";
}
int chain_hook(mc_ctx* c, long& v) {       // bit 0 (the fused expert MLP) decides whether hbuf is free split-K scratch
    const int L = c->m->cfg.latent_dim;
    c->hbuf_floats = ((v >> kChainMlp) & 1) && mc_mlp_supported(L, 4 * L) ? c->hbuf_cap : 0;
    return MC_OK;
}
int route_coop_hook(mc_ctx* c, long& v) {      // off: give the reservation back; on: only if the grid can be reserved now
    if (!v) {
        if (c->coop_reserved) { mc_route_coop_release(c->device, c->coop_reserved); c->coop_reserved = 0; }
    } else if (!c->opt.route_coop) {
        const int nwg = coop_grid_needed(c);       // 0: no routing call of this context is in route_coop_k's size range (nothing to switch on)
        MC_REQUIRE(nwg == 0 || mc_route_coop_reserve(c->device, nwg), "route_coop: the cooperative routing grid cannot be reserved on this device");
        c->coop_reserved = nwg;
        v = nwg > 0;
    }
    return MC_OK;
}

const OptionDef kOptions[] = {
    {"chain", "MC_CHAIN", nullptr, &McOptions::chain, kChainDefault, check_chain, chain_hook},      // ChainBit mask (mc_options.h)
    // plain GEMMs of up to this many rows take the small-M kernels (round 4: 6400 -> 5600, measured per batch: at 6272 rows -- a sample
    // group of 32 x 196 frames -- gemm_wp_k / gemm_tail_k win, B=32 step 10.21 -> 10.03 ms; at 4704 rows (B=24) the small kernels, 7.85 vs 7.91)
    {"small_gemm_rows", "MC_SMALL_GEMM_ROWS", nullptr, &McOptions::small_gemm_rows, 5600},
    {"split_rows_expert", "MC_SPLIT_ROWS_EXPERT", nullptr, &McOptions::split_rows_expert, 2048},   // residual rows up to which the fused expert MLP
    {"split_rows_sffn", "MC_SPLIT_ROWS_SFFN", nullptr, &McOptions::split_rows_sffn, 8192},         // ... and the SFFN split their hidden dimension
    {"temporal_split", "MC_TEMPORAL_SPLIT", nullptr, &McOptions::temporal_split, 96},      // (sample, part) workgroups up to which temporal_k slices its columns
    {"big_tokens", "MC_BIG_TOKENS", nullptr, &McOptions::big_tokens, 65536},               // above this many motion tokens: the large-batch schedule
    {"rowchain_split", "MC_ROWCHAIN_SPLIT", nullptr, &McOptions::rowchain_split, 20480},   // tokens up to which rowchain_k slices its chunks over blockIdx.y
    {"gemm_tune", "MC_GEMM_TUNE", nullptr, &McOptions::gemm_tune, kTuneDefault, check_tune},       // kTune* bits (mc_gemm.h)
    {"small_tile_n", "MC_SMALL_TILE_N", nullptr, &McOptions::small_tile_n, 0,                      // small-M tile width; 0: the load model's per launch
     [](long v) -> std::string { return v == 0 || v == 48 || v == 64 || v == 96 ? "" : "small_tile_n: 0 (per-launch choice), 48, 64 or 96"; }},
    {"gemm_wp_grid", "MC_GEMM_WP_GRID", nullptr, &McOptions::gemm_wp_grid, 512},           // workgroups of the persistent gemm_wp_k; <= 0: one per tile
    {"half_min_rows", "MC_HALF_MIN_ROWS", nullptr, &McOptions::half_min_rows, 512},        // reduced precision: the fp32 kernels up to this many rows (use_half)
    {"gate_small", "MC_GATE_SMALL", nullptr, &McOptions::gate_small, 12000},               // up to this many tokens the gate runs as gate_small_k
    {"split_expert", "MC_SPLIT_EXPERT", nullptr, &McOptions::split_expert, 0},             // hidden split of the small-batch expert MLP (0: load model)
    {"split_sffn", "MC_SPLIT_SFFN", nullptr, &McOptions::split_sffn, 0},                   // ... of the SFFN (0: load model)
    {"route_reg", "MC_ROUTE_REG", nullptr, &McOptions::route_reg, 1},                      // 0: the L2-streaming one-workgroup routing kernel at every size
    {"route_coop", "MC_ROUTE_COOP", nullptr, &McOptions::route_coop, 1, nullptr, route_coop_hook},       // 0: the routing launch sequence, not route_coop_k
    // up to this many (token, choice) pairs the routing is one workgroup; those kernels assume token indices < 2^16.  Default = what fits
    // the register kernels (beyond: route_coop_k; B=3: 97.5 -> 90.4 ms vs the streaming form).  The tests set MC_ROUTE_SMALL_CTX
    {"route_small", "MC_ROUTE_SMALL_CTX", "MC_ROUTE_SMALL", &McOptions::route_small, 20480,
     [](long v) -> std::string { return v >= 0 && v <= 131072 ? "" : "route_small: 0 .. 131072 pairs (the one-workgroup kernels hold at most 131072)"; }},
    // two-stream schedule: each sample group's experts start behind its own gate, the whole-batch capacity cut runs beside them
    // (run_layer); 0: the groups join in front of the routing.  Inert in the one-stream schedules.  Applied where it helps, as
    // kChainStagger is: a context of an L = 64 model (M2D loses 0.45 ms per step with it) starts at 0 unless the variable says otherwise
    {"route_early", "MC_ROUTE_EARLY", nullptr, &McOptions::route_early, 1,
     [](long v) -> std::string { return v == 0 || v == 1 ? "" : "route_early: 0 or 1"; }},
    {"route_per", nullptr, nullptr, &McOptions::route_per, 0,                              // route_coop_k pairs per thread (0: 10 up to 256 workgroups, 16 beyond)
     [](long v) -> std::string { return v == 0 || v == 10 || v == 16 ? "" : "route_per: 0 (default), 10 or 16"; }},
    {"dbg_delay_us", nullptr, nullptr, &McOptions::dbg_delay_us, 0,                        // tests: hold the second (> 0) or first (< 0) group's stream
     [](long v) -> std::string { return v >= -100000 && v <= 100000 ? "" : "dbg_delay_us: -100000 .. 100000"; }},      // in front of every layer tail
};

// the built-in defaults, overridden by the environment; an invalid value is an error naming the variable
int seed_options(McOptions& o) {
    for (const OptionDef& d : kOptions) {
        const char *var = nullptr, *e = nullptr;
        for (const char* v : {d.env, d.env_alt})
            if (v && !e && (e = getenv(v))) var = v;
        const std::string why = e && d.check ? d.check(atol(e)) : "";
        MC_REQUIRE(why.empty(), "%s=%s: %s", var, e, why.c_str());
        o.*d.field = e ? atol(e) : d.dflt;
    }
    return MC_OK;
}

}  // namespace

const McOptions* mc_process_options() {
    static McOptions o;
    static const std::string err = seed_options(o) == MC_OK ? "" : mc_last_error();
    if (!err.empty()) mc_set_error("%s", err.c_str());
    return err.empty() ? &o : nullptr;
}

extern "C" {

int mc_device_count(int* n) {
    MC_HIP(hipGetDeviceCount(n));
    return MC_OK;
}
int mc_set_device(int dev) {
    MC_HIP(hipSetDevice(dev));
    return MC_OK;
}

int mc_model_create(const mc_model_config* cfg, mc_model** out) {
    MC_REQUIRE(cfg && out, "null argument");
    MC_REQUIRE(cfg->latent_dim == 32 || cfg->latent_dim == 64 || cfg->latent_dim == 128,
               "latent_dim=%d unsupported (32, 64, 128)", cfg->latent_dim);
    MC_REQUIRE(cfg->topk == 2, "topk=%d unsupported (reference configs use 2)", cfg->topk);
    MC_REQUIRE(cfg->num_experts >= 2 && cfg->num_experts <= 16, "num_experts=%d unsupported", cfg->num_experts);
    MC_REQUIRE(cfg->latent_dim % cfg->dyn_heads == 0, "latent_dim %% dyn_heads != 0");
    MC_REQUIRE(cfg->num_ctrl_layers >= 0 && cfg->num_ctrl_layers < cfg->num_layers, "copy_blocks_num=%d must be in [0, num_layers)", cfg->num_ctrl_layers);
    MC_REQUIRE(cfg->num_ctrl_layers == 0 || cfg->ctrl_cond_feats >= 1, "ctrl_cond_feats must be >= 1");
    MC_REQUIRE(cfg->ffn_dim % 4 == 0 && cfg->time_embed_dim % 4 == 0 && cfg->text_latent_dim % 4 == 0, "dims must be multiples of 4");
    {
        const int q = cfg->text_latent_dim / 4;
        MC_REQUIRE(q >= 1 && q <= 64 && (q & (q - 1)) == 0, "text_latent_dim=%d unsupported", cfg->text_latent_dim);
    }
    mc_model* m = new mc_model();
    m->cfg = *cfg;
    m->Cp = (cfg->input_feats + 31) / 32 * 32;
    *out = m;
    return MC_OK;
}

void mc_model_destroy(mc_model* m) {
    if (!m) return;
    for (auto& kv : m->half) (void)hipFree(const_cast<mc_half*>(kv.second.hi));
    delete m;
}

int mc_model_set_param(mc_model* m, const char* name, const float* host, int64_t numel) {
    MC_REQUIRE(m && name && host && numel > 0, "bad argument");
    // replacing a weight of a finalized model: contexts hold raw pointers into the old allocation and the fp16 planes built from it
    // would go stale -- the model is immutable once contexts can exist (build a new model for new weights).  Checked BEFORE anything
    // is allocated (a rejected call must not leak the new buffer).
    MC_REQUIRE(!m->finalized || !m->params.has(name), "mc_model_set_param(%s): the model is finalized; weights are immutable from then on", name);
    return m->params.set(name, host, numel);
}

int mc_model_finalize(mc_model* m) {
    MC_REQUIRE(m, "null model");
    mc_ctx probe;
    probe.m = m;
    int r = bind_weights(&probe);
    if (r != MC_OK) return r;
    m->finalized = true;
    return MC_OK;
}

int mc_ctx_create(mc_model* m, int32_t batch, int32_t frames, int32_t max_steps, mc_ctx** out) {
    MC_REQUIRE(m && out, "null argument");
    MC_REQUIRE(m->finalized, "model not finalized");
    MC_REQUIRE(batch >= 1 && frames >= 1 && frames <= m->cfg.max_seq_len, "bad batch/frames (%d, %d)", batch, frames);
    MC_REQUIRE(max_steps >= 1, "max_steps < 1");
    const mc_model_config& g = m->cfg;
    mc_ctx* c = new mc_ctx();
    if (int r = seed_options(c->opt)) { mc_ctx_destroy(c); return r; }
    if (m->cfg.latent_dim == 64 && !getenv("MC_ROUTE_EARLY")) c->opt.route_early = 0;      // (measured per width: see kOptions)
    c->m = m;
    c->B = batch;
    c->T = frames;
    c->maxS = max_steps;
    c->cap_factor = g.capacity_factor;
    const int L = g.latent_dim, H = g.num_parts, D = L * H, F = g.ffn_dim, Te = g.time_embed_dim, Dt = g.text_latent_dim;
    const long B2 = 2L * batch;
    c->rows = B2 * frames;
    c->N = c->rows * H;
    c->Ntxt = B2 * g.max_text_len;
    int r = bind_weights(c);
    if (r == MC_OK) r = build_ctx_weights(c);
    if (r != MC_OK) { mc_ctx_destroy(c); return r; }
    bool cand_ok = true;
    for (int k = 0; k < mc_ctx::SIDE_CAND; ++k) cand_ok = cand_ok && hipStreamCreateWithFlags(&c->side_cand[k], hipStreamNonBlocking) == hipSuccess;
    c->side = c->side_cand[0];
    for (hipEvent_t* e : {&c->ev_fork, &c->ev_join, &c->ev_side, &c->ev_stag, &c->ev_gate1, &c->ev_sel, &c->ev_front}) cand_ok = cand_ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
    if (!cand_ok) {
        mc_set_error("could not create the side stream / events");
        mc_ctx_destroy(c);
        return MC_ERR_HIP;
    }
    const long Nmax = c->N > c->Ntxt ? c->N : c->Ntxt;
    const size_t zsz = (size_t)(c->N * L > c->Ntxt * Dt ? c->N * L : c->Ntxt * Dt);
    const size_t hsz = (size_t)(2 * c->N * 4 * L > 2 * c->Ntxt * 4 * Dt ? 2 * c->N * 4 * L : 2 * c->Ntxt * 4 * Dt);
#define WS(p, n) do { if ((r = ws_alloc(c, &(p), (size_t)(n))) != MC_OK) { mc_ctx_destroy(c); return r; } } while (0)
    WS(c->h, c->rows * D);
    WS(c->z, zsz);
    WS(c->proj, Nmax * 256);
    WS(c->hbuf, hsz);
    c->hbuf_cap = hsz;
    if (chain_on(c, kChainMlp) && mc_mlp_supported(L, 4 * L)) c->hbuf_floats = hsz;   // (the text MoE only touches hbuf in set_condition)
    WS(c->y2, 2 * zsz);
    WS(c->mf, (c->N + 128) * 4 * L);        // + 128 padding rows: projqkv_k stores unconditionally (invalid lanes land there)
    WS(c->qkv, (c->N + 128) * 3 * L);
    WS(c->ys, c->rows * D);
    WS(c->yt, c->rows * D);
    WS(c->a, c->rows * D);
    WS(c->z2, c->rows * D);
    WS(c->fh, c->rows * H * F);
    WS(c->out2, c->rows * g.input_feats);
    WS(c->xpad, (long)batch * frames * m->Cp);
    WS(c->xfn, c->Ntxt * Dt);
    WS(c->mask_own, (long)batch * frames);
    WS(c->tf, (long)c->NLA * c->Ntxt * 2 * L);
    WS(c->t_orig, max_steps);
    WS(c->te, (long)max_steps * D);
    WS(c->e1, (long)max_steps * Te);
    WS(c->emb, (long)max_steps * Te);
    WS(c->semb, (long)max_steps * Te);
    WS(c->ss, (long)c->NLA * 2 * max_steps * 2 * D);
    if (g.num_ctrl_layers > 0) {
        WS(c->hc, c->rows * D);
        WS(c->cb, c->rows * D);
        WS(c->cenc, (long)batch * frames * D);
    }
    WS(c->rb.idx, 2 * Nmax);
    WS(c->rb.gate, 2 * Nmax);
    WS(c->rb.key, Nmax);
    WS(c->rb.comb_w, 2 * Nmax);
    WS(c->rb.src_row, 2 * Nmax);
    WS(c->rb.dst_row, 2 * Nmax);
    c->rb.max_tiles = cdiv(2 * Nmax, 128) + g.num_experts;
    WS(c->rb.tile_group, 2 * c->rb.max_tiles);
    WS(c->rb.tile_row0, 2 * c->rb.max_tiles);
    WS(c->rb.tile_nrows, 2 * c->rb.max_tiles);
    WS(c->rb.state, mc_route_state_ints(g.num_experts));
    MC_HIP(hipMemset(c->rb.state + mc_route_barrier_offset(), 0, mc_route_barrier_ints() * sizeof(int)));      // grid-barrier words of the cooperative routing kernel
    // the cooperative routing kernel needs its whole grid resident: reserve it out of what the device holds, or run the
    // launch sequence instead (no env var needed: a fifth concurrent B = 64 context, or a CPX partition, simply falls back)
    // Reserved for the LARGEST grid any routing call of this context can launch cooperatively: the motion MoE routes N tokens, the
    // text MoE (mc_ctx_set_condition) Ntxt -- either may be the one inside route_coop_k's size range.  Nothing to reserve (both in
    // the one-workgroup regime or beyond the kernel's range) or no room -> coop off for the context, so no unreserved grid can launch.
    MC_HIP(hipGetDevice(&c->device));
    if (c->opt.route_coop) {
        const int nwg = coop_grid_needed(c);
        if (nwg > 0 && mc_route_coop_reserve(c->device, nwg)) c->coop_reserved = nwg;
        else c->opt.route_coop = 0;
    }
#undef WS
    *out = c;
    return MC_OK;
}

static void graph_release(mc_ctx* c) {       // the captured sampler step (mc_ctx_graph_capture)
    if (c->graph_exec) { (void)hipGraphExecDestroy(c->graph_exec); c->graph_exec = nullptr; }
    if (c->graph) { (void)hipGraphDestroy(c->graph); c->graph = nullptr; }
    c->graph_steps = 0;
    c->graph_multistep = false;
    c->graph_k1.clear();
}
static void prof_clear(mc_ctx* c) {
    for (auto& p : c->prof) { if (p.e0) (void)hipEventDestroy(p.e0); if (p.e1) (void)hipEventDestroy(p.e1); }
    c->prof.clear();
}

void mc_ctx_destroy(mc_ctx* c) {
    if (!c) return;
    graph_release(c);
    if (c->coop_reserved) { mc_route_coop_release(c->device, c->coop_reserved); c->coop_reserved = 0; }
    prof_clear(c);
    for (int k = 0; k < mc_ctx::SIDE_CAND; ++k)
        if (c->side_cand[k]) { (void)hipStreamSynchronize(c->side_cand[k]); (void)hipStreamDestroy(c->side_cand[k]); }
    for (hipEvent_t e : {c->ev_fork, c->ev_join, c->ev_side, c->ev_stag, c->ev_gate1, c->ev_sel, c->ev_front})
        if (e) (void)hipEventDestroy(e);
    if (c->rs_ev) { (void)hipEventSynchronize(c->rs_ev); (void)hipEventDestroy(c->rs_ev); }
    if (c->rs_stage) (void)hipHostFree(c->rs_stage);
    for (void* p : c->allocs) (void)hipFree(p);
    delete c;
}

int64_t mc_ctx_workspace_bytes(const mc_ctx* c) { return c ? (int64_t)(c->bytes + (c->prec != MC_PREC_F32 ? c->m->half_bytes : 0)) : 0; }

int mc_ctx_check(mc_ctx* c, void* stream) {
    MC_REQUIRE(c, "null context");
    int flag = 0;
    MC_HIP(hipMemcpyAsync(&flag, c->rb.state + mc_route_error_offset(), sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    MC_HIP(hipStreamSynchronize((hipStream_t)stream));
    if (flag != 0) {
        mc_set_error("the cooperative routing kernel's grid barrier timed out (its workgroups were not all resident: another process "
                     "is holding the GPU with barrier kernels of its own); the results of this context are invalid -- destroy it and "
                     "create the context with MC_ROUTE_COOP=0");
        return MC_ERR_STATE;
    }
    return MC_OK;
}

int mc_ctx_effective_precision(const mc_ctx* c) { return c ? (use_half(c) ? c->prec : MC_PREC_F32) : MC_PREC_F32; }

int mc_ctx_uses_coop_routing(const mc_ctx* c) { return c && c->opt.route_coop && c->coop_reserved > 0 ? 1 : 0; }

int mc_ctx_profile(mc_ctx* c, int32_t on) {
    MC_REQUIRE(c, "null context");
    MC_REQUIRE(!c->graph_mode, "profiling inside a graph capture");
    prof_clear(c);
    c->prof_on = on != 0;
    return MC_OK;
}

int mc_ctx_profile_read(mc_ctx* c, int64_t rows_filter, double* avg_us, int32_t* count, double* gflop_per_launch) {
    MC_REQUIRE(c && avg_us && count && gflop_per_launch, "null argument");
    const int D = c->m->cfg.latent_dim * c->m->cfg.num_parts;
    double sum = 0.0, rows = 0.0;
    int n = 0;
    for (auto& p : c->prof) {
        MC_HIP(hipEventSynchronize(p.e1));
        if (rows_filter > 0 && p.rows != rows_filter) continue;
        float ms = 0.f;
        MC_HIP(hipEventElapsedTime(&ms, p.e0, p.e1));
        sum += ms * 1e3;
        rows += (double)p.rows;
        ++n;
    }
    *count = n;
    *avg_us = n ? sum / n : 0.0;
    *gflop_per_launch = n ? 2.0 * (rows / n) * D * D / 1e9 : 0.0;
    return MC_OK;
}

int mc_ctx_set_tie_policy(mc_ctx* c, int32_t policy) {
    MC_REQUIRE(c, "null context");
    MC_REQUIRE(policy == MC_TIE_STABLE || policy == MC_TIE_REVERSE, "tie policy %d (MC_TIE_STABLE or MC_TIE_REVERSE)", policy);
    c->rb.tie_xor = policy == MC_TIE_STABLE ? 0xFFFFFFFFu : 0u;
    c->have_cond = false;      // the hoisted text K/V were routed under the previous policy: set the condition again
    return MC_OK;
}

int mc_ctx_set_capacity_factor(mc_ctx* c, float cf) {
    MC_REQUIRE(c, "null context");
    MC_REQUIRE(cf >= 0.f, "capacity factor %g: > 0 (tutel's formula with it) or 0 (nothing dropped); tutel's negative form is not built", (double)cf);      // (NaN fails too)
    if (c->graph_exec) {
        mc_set_error("mc_ctx_set_capacity_factor: a captured graph holds the old routing launches (mc_ctx_graph_release first)");
        return MC_ERR_STATE;
    }
    c->keep_all = cf == 0.f;
    c->cap_factor = cf;
    c->have_cond = false;      // the hoisted text K/V were routed under the previous capacity: set the condition again
    hist_set(c, false);     // (multistep sampler: the previous x0 was predicted under it too)
    return MC_OK;
}
float mc_ctx_capacity_factor(const mc_ctx* c) { return c ? c->cap_factor : 0.f; }

int mc_ctx_set_precision(mc_ctx* c, int32_t precision) {
    MC_REQUIRE(c, "null context");
    MC_REQUIRE(precision == MC_PREC_F32 || precision == MC_PREC_F16 || precision == MC_PREC_F16X3, "precision %d", precision);
    if (precision != MC_PREC_F32) {
        int r = bind_half_weights(c);
        if (r != MC_OK) return r;
        if (!c->a_tail && (r = ws_alloc(c, &c->a_tail, (size_t)c->rows * c->m->cfg.latent_dim * c->m->cfg.num_parts)) != MC_OK) return r;
    }
    c->prec = precision;
    return MC_OK;
}

// Per-context kernel-selection switches (the MC_* environment variables only seed the defaults of contexts created later): kOptions.
int mc_ctx_set_option(mc_ctx* c, const char* key, int64_t value) {
    MC_REQUIRE(c && key, "null argument");
    MC_REQUIRE(!c->graph_exec, "mc_ctx_set_option: a captured graph holds the old kernel selection (mc_ctx_graph_release first)");
    for (const OptionDef& d : kOptions) {
        if (std::string(d.key) != key) continue;
        long v = (long)value;
        const std::string why = d.check ? d.check(v) : "";
        MC_REQUIRE(why.empty(), "%s", why.c_str());
        if (d.hook)
            if (int r = d.hook(c, v)) return r;
        c->opt.*d.field = v;
        return MC_OK;
    }
    mc_set_error("mc_ctx_set_option: unknown key '%s'", key);
    return MC_ERR_ARG;
}

int mc_ctx_enable_capture(mc_ctx* c) {
    MC_REQUIRE(c, "null context");
    if (c->cap_idx) return MC_OK;
    int r;
    if ((r = ws_alloc(c, &c->cap_idx, (size_t)c->NLA * 2 * c->N)) != MC_OK) return r;
    return ws_alloc(c, &c->cap_w, (size_t)c->NLA * 2 * c->N);
}

// time_embed (diffusion_transformer.py:89-93,206-208) and every StylizationBlock.emb_layers
// (stylization_block.py:17-20,34-35) depend only on the timestep, which is identical for the whole
// batch -> evaluated once for all S steps of the schedule as M = S row GEMMs.
int mc_ctx_set_timesteps(mc_ctx* c, const int32_t* t_orig_host, int32_t S, void* stream) {
    MC_REQUIRE(c && t_orig_host, "null argument");
    MC_REQUIRE(S >= 1 && S <= c->maxS, "num_steps=%d exceeds context max_steps=%d", S, c->maxS);
    hist_set(c, false);       // (multistep sampler: the previous x0 belongs to the old schedule)
    hipStream_t s = (hipStream_t)stream;
    const mc_model_config& g = c->m->cfg;
    const int D = g.latent_dim * g.num_parts, Te = g.time_embed_dim;
    MC_HIP(hipMemcpyAsync(c->t_orig, t_orig_host, sizeof(int) * S, hipMemcpyHostToDevice, s));
    MC_HIP(hipStreamSynchronize(s));  // t_orig_host may be a temporary of the caller
    int r;
    if ((r = mc_launch_timestep_embedding(c->t_orig, c->te, S, D, s))) return r;
    if ((r = dense(c, c->te, D, c->time_w0, D, c->time_b0, nullptr, 0, c->e1, Te, S, Te, D, ACT_SILU, s))) return r;
    if ((r = dense(c, c->e1, Te, c->time_w2, Te, c->time_b2, nullptr, 0, c->emb, Te, S, Te, Te, ACT_NONE, s))) return r;
    if ((r = mc_launch_silu(c->emb, c->semb, (long)S * Te, s))) return r;
    for (int i = 0; i < c->NLA; ++i) {
        const LayerW& w = c->lw[i];
        float* ss0 = c->ss + ((long)(i * 2 + 0) * c->maxS) * 2 * D;
        float* ss1 = c->ss + ((long)(i * 2 + 1) * c->maxS) * 2 * D;
        if ((r = dense(c, c->semb, Te, w.ca_film_w, Te, w.ca_film_b, nullptr, 0, ss0, 2 * D, S, 2 * D, Te, ACT_NONE, s))) return r;
        if ((r = dense(c, c->semb, Te, w.ffn_film_w, Te, w.ffn_film_b, nullptr, 0, ss1, 2 * D, S, 2 * D, Te, ACT_NONE, s))) return r;
    }
    c->S = S;
    return MC_OK;
}

// Step-invariant text K/V of every layer (st_attention.py:116-118): text_moe over the CFG-doubled
// condition batch (the MoE capacity couples both halves, so both are routed together).
int mc_ctx_set_condition(mc_ctx* c, const float* xf_out_dev, const float* mask_dev, void* stream) {
    MC_REQUIRE(c && xf_out_dev && mask_dev, "null argument");
    hist_set(c, false);       // (multistep sampler: the previous x0 belongs to the old condition)
    hipStream_t s = (hipStream_t)stream;
    const mc_model_config& g = c->m->cfg;
    const int L = g.latent_dim, Dt = g.text_latent_dim, Nt = g.max_text_len;
    const long half = (long)c->B * Nt;
    MC_HIP(hipMemcpyAsync(c->mask_own, mask_dev, sizeof(float) * c->B * c->T, hipMemcpyDeviceToDevice, s));
    c->mask = c->mask_own;
    int r;
    for (int i = 0; i < c->NLA; ++i) {
        const LayerW& w = c->lw[i];
        if ((r = mc_launch_ln_rows(xf_out_dev, Dt, 0, w.tnorm_g, w.tnorm_b, w.tm.emb, Nt, c->xfn, Dt, half, Dt, s))) return r;
        MC_HIP(hipMemcpyAsync(c->xfn + half * Dt, c->xfn, sizeof(float) * half * Dt, hipMemcpyDeviceToDevice, s));
        if ((r = run_moe(c, w.tm, c->xfn, c->Ntxt, c->tf + (long)i * c->Ntxt * 2 * L, 2 * L, false, false, c->Ntxt, s, nullptr, nullptr))) return r;      // (the text MoE has no fp16 planes)
    }
    c->have_cond = true;
    return MC_OK;
}

// ControlT2MHalf.forward_c (controlnet.py:186-199) with condition_pre_encoder = identity, followed by
// `c * all_cond_type` (controlnet.py:377-379) and controlnet[0].before_proj (controlnet.py:66): all
// step-invariant, evaluated once per condition batch.
int mc_ctx_set_control(mc_ctx* c, const float* c_feat_dev, int32_t Tc, void* stream) {
    MC_REQUIRE(c, "null context");
    hist_set(c, false);       // (multistep sampler: the previous x0 belongs to the old control condition)
    const mc_model_config& g = c->m->cfg;
    if (!c_feat_dev) { c->have_ctrl = false; return MC_OK; }
    MC_REQUIRE(g.num_ctrl_layers > 0, "the model has no control branch");
    MC_REQUIRE(Tc >= 1 && Tc <= c->T, "control length %d outside [1, %d]", Tc, c->T);
    hipStream_t s = (hipStream_t)stream;
    const int D = g.latent_dim * g.num_parts, Fc = g.ctrl_cond_feats;
    const long BT = (long)c->B * c->T;
    int r;
    MC_HIP(hipMemsetAsync(c->cenc, 0, sizeof(float) * BT * D, s));           // zero padding for t >= Tc
    {
        GemmArgs e;
        mc_gemm_opts(c->opt, e);   // per sample: [Tc, Fc] x [D, Fc]^T + bias + sequence_embedding[:Tc]
        e.A = c_feat_dev; e.lda = Fc; e.a_gstride = (long)Tc * Fc;
        e.W = c->ctrl_in_w; e.ldw = (Fc + 3) / 4 * 4; e.bias = c->ctrl_in_b;
        e.add = c->seq_emb; e.add_mod = Tc; e.ld_add = D;
        e.C = c->cenc; e.ldc = D; e.c_gstride = (long)c->T * D; e.dup_rows = 0;
        e.M = Tc; e.N = D; e.K = Fc;
        if ((r = mc_launch_gemm(GM_ENC, e, c->B, 0, s))) return r;
    }
    const LayerW& w0 = c->lw[g.num_layers];
    // text-conditioned half: before_proj(c); unconditional half: before_proj(c * 0) = bias when condition_cfg
    if ((r = dense(c, c->cenc, D, w0.before_w, D, w0.before_b, nullptr, 0, c->cb, D, BT, D, D, ACT_NONE, s))) return r;
    if (g.ctrl_condition_cfg) {
        if ((r = mc_launch_add_rows(c->cb + BT * D, nullptr, nullptr, w0.before_b, BT, D, s))) return r;
    } else {
        MC_HIP(hipMemcpyAsync(c->cb + BT * D, c->cb, sizeof(float) * BT * D, hipMemcpyDeviceToDevice, s));
    }
    c->have_ctrl = true;
    return MC_OK;
}

int mc_denoise(mc_ctx* c, const float* x_t, int32_t step, float* out2_dev, int32_t stop_after, void* stream) {
    return denoise_impl(c, x_t, step, out2_dev, stop_after, stream, nullptr);
}


// ---- multistep sampler (mode 2): the context's history buffer and its "history valid" flag ----
static bool is_multistep(const mc_step_coefs* k) { return k->mode == MC_SAMPLER_MULTISTEP; }
static int check_mode(const mc_step_coefs* k) {
    MC_REQUIRE(k->mode == MC_SAMPLER_DDPM || k->mode == MC_SAMPLER_DDIM || k->mode == MC_SAMPLER_MULTISTEP, "unknown sampler mode %d", k->mode);
    return MC_OK;
}
// allocated by the first mode-2 call: contexts that never use the mode keep their workspace size
static int hist_alloc(mc_ctx* c) {
    return c->x0_hist ? MC_OK : ws_alloc(c, &c->x0_hist, (size_t)c->B * c->T * c->m->cfg.input_feats);
}
// before a mode-2 step with coefficient k1 of the previous x0
static int hist_require(const mc_ctx* c, float k1, int32_t step) {
    if (k1 != 0.f && !c->hist_valid) {
        mc_set_error("multistep step at schedule index %d reads the previous x0 (k1 = %g), but the context holds none: no multistep step ran since "
                     "the condition / control / timesteps were set", step, (double)k1);
        return MC_ERR_STATE;
    }
    return MC_OK;
}

// ---- coupled windows (sampler_seam_k): the seam table of a context / of the context-free op ----
// B windows of T frames at global first frames ff[b], neighbours sharing `ov` frames -> per-row flags (bit 0: left neighbour, bit 1: right)
// and the right-window weights.  Rows b, b + 1 are neighbours when ff[b + 1] == ff[b] + T - ov and must otherwise be disjoint.
static int seam_plan(const char* who, int B, int T, int ov, const int32_t* ff, const float* w, std::vector<int>* flags, std::vector<float>* wt) {
    MC_REQUIRE(B >= 1 && T >= 1, "%s: %d windows of %d frames", who, B, T);
    MC_REQUIRE(ov > 0 && 2L * ov <= T, "%s: overlap %d outside (0, T / 2 = %d] (a frame may lie in two windows at most)", who, ov, T / 2);
    MC_REQUIRE(ff, "%s: null first_frame", who);
    const long stride = T - ov;
    flags->assign(B, 0);
    for (int b = 0; b < B; ++b) {
        MC_REQUIRE(ff[b] >= 0, "%s: first_frame[%d] = %d is negative", who, b, ff[b]);
        if (b + 1 == B) break;
        const long gap = (long)ff[b + 1] - ff[b];
        if (gap == stride) { (*flags)[b] |= 2; (*flags)[b + 1] |= 1; }
        else MC_REQUIRE(gap >= T, "%s: first_frame[%d] = %d after first_frame[%d] = %d: neither its neighbour (+%ld) nor disjoint from it (>= +%d)",
                        who, b + 1, ff[b + 1], b, ff[b], stride, T);
    }
    wt->resize(ov);
    for (int f = 0; f < ov; ++f) {
        if (w) MC_REQUIRE(w[f] >= 0.f && w[f] <= 1.f, "%s: weight[%d] = %g outside [0, 1]", who, f, (double)w[f]);
        (*wt)[f] = w ? w[f] : (float)((double)(f + 1) / (double)(ov + 1));
    }
    return MC_OK;
}
static int seam_refuse(const mc_ctx* c, const char* who) {
    if (c->seam_ov > 0) {
        mc_set_error("%s: the context has a seam table set (mc_ctx_set_seams): coupled windows take mc_sample_step / mc_sample_loop only; clear it with overlap = 0", who);
        return MC_ERR_STATE;
    }
    return MC_OK;
}

// ---- edited rows (mc_ctx_set_edit_rows): every entry without a rows form refuses while a table is set ----
static int edit_refuse(const mc_ctx* c, const char* who) {
    if (c->edit_set) {
        mc_set_error("%s: the context has an edit table set (mc_ctx_set_edit_rows): edited rows take mc_sample_rows only; clear it with gt_dev = keep_dev = NULL", who);
        return MC_ERR_STATE;
    }
    return MC_OK;
}

// ---- seam-coupled windows in rows mode (mc_ctx_set_seam_rows): every entry without a rows form refuses while a table is set ----
static int seam_rows_refuse(const mc_ctx* c, const char* who) {
    if (c->seam_rows_ov > 0) {
        mc_set_error("%s: the context has a row seam table set (mc_ctx_set_seam_rows): coupled request rows take mc_sample_rows only; clear it with overlap = 0", who);
        return MC_ERR_STATE;
    }
    return MC_OK;
}
// B request rows, right[b] = the row holding the next window of b's request (any row, or -1), ff[b] = the global frame of b's frame 0
// -> the device entries and the right-window weights.  Every rule is checked on the host: right[b] in [-1, B) and != b; a row is the
// right neighbour of at most one row; ff[right[b]] == ff[b] + T - ov (first frames grow strictly along a chain, so no chain closes
// into a cycle: a walk of more than B links is refused all the same); the has-left flags are derived from right[], consistent by that.
static int seam_rows_plan(const char* who, int B, int T, int ov, const int32_t* right, const int32_t* ff, const float* w,
                          std::vector<SeamRow>* rows, std::vector<float>* wt) {
    MC_REQUIRE(B >= 1 && T >= 1, "%s: %d rows of %d frames", who, B, T);
    MC_REQUIRE(ov > 0 && 2L * ov <= T, "%s: overlap %d outside (0, T / 2 = %d] (a frame may lie in two windows at most)", who, ov, T / 2);
    MC_REQUIRE(right && ff, "%s: null right / first_frame", who);
    const long stride = T - ov;
    rows->assign((size_t)B, SeamRow{-1, 0, 0, 0});
    for (int b = 0; b < B; ++b) {
        MC_REQUIRE(ff[b] >= 0, "%s: first_frame[%d] = %d is negative", who, b, ff[b]);
        MC_REQUIRE(right[b] >= -1 && right[b] < B && right[b] != b, "%s: right[%d] = %d (another row in [0, %d), or -1)", who, b, right[b], B);
        (*rows)[b].right = right[b];
        (*rows)[b].first_frame = ff[b];
    }
    for (int b = 0; b < B; ++b) {
        const int rb = right[b];
        if (rb < 0) continue;
        MC_REQUIRE(!(*rows)[rb].has_left, "%s: row %d is the right neighbour of two rows (three-way overlaps are not served)", who, rb);
        (*rows)[rb].has_left = 1;
        MC_REQUIRE((long)ff[rb] == (long)ff[b] + stride, "%s: first_frame[%d] = %d, the right neighbour of row %d at %d: not one stride (%ld) behind it",
                   who, rb, ff[rb], b, ff[b], stride);
    }
    for (int b = 0; b < B; ++b) {
        int len = 0;
        for (int v = right[b]; v >= 0; v = right[v]) MC_REQUIRE(++len < B, "%s: the chain from row %d does not end (a cycle)", who, b);
    }
    wt->resize(ov);
    for (int f = 0; f < ov; ++f) {
        if (w) MC_REQUIRE(w[f] >= 0.f && w[f] <= 1.f, "%s: weight[%d] = %g outside [0, 1]", who, f, (double)w[f]);
        (*wt)[f] = w ? w[f] : (float)((double)(f + 1) / (double)(ov + 1));
    }
    return MC_OK;
}

int mc_ctx_set_seam_rows(mc_ctx* c, int32_t overlap, const int32_t* right, const int32_t* first_frame, const float* weight, void* stream) {
    MC_REQUIRE(c, "null context");
    if (overlap == 0) { c->seam_rows_ov = 0; c->seam_rows_right.clear(); return MC_OK; }      // (no history flag is touched: the rows walk on)
    if (c->graph_mode || c->graph_exec) {
        mc_set_error("mc_ctx_set_seam_rows: the context holds a captured graph (mc_ctx_graph_release first): row steps are not replayed");
        return MC_ERR_STATE;
    }
    if (!c->long_edits) { if (int re = edit_refuse(c, "mc_ctx_set_seam_rows")) return re; }
    if (int rs = seam_refuse(c, "mc_ctx_set_seam_rows")) return rs;
    std::vector<SeamRow> rows;
    std::vector<float> wt;
    int r;
    if ((r = seam_rows_plan("mc_ctx_set_seam_rows", c->B, c->T, overlap, right, first_frame, weight, &rows, &wt))) return r;
    MC_REQUIRE((long)c->B * c->T * c->m->cfg.input_feats <= 0x7fffffffL && (long)c->T * c->m->cfg.input_feats >= 4,
               "mc_ctx_set_seam_rows: a batch of %d x %d x %d floats", c->B, c->T, c->m->cfg.input_feats);
    if (!c->seam_rows_tab && (r = ws_alloc(c, &c->seam_rows_tab, (size_t)c->B + ((size_t)c->T / 2 + 3) / 4)) != MC_OK) return r;
    hipStream_t s = (hipStream_t)stream;
    // every check has passed.  A copy that fails half way (MC_ERR_HIP) would leave new rows beside old weights and the old host right[]:
    // no table is the safe state then, as in mc_ctx_set_seams
    c->seam_rows_ov = 0;
    c->seam_rows_right.clear();
    MC_HIP(hipMemcpyAsync(c->seam_rows_tab, rows.data(), sizeof(SeamRow) * c->B, hipMemcpyHostToDevice, s));
    MC_HIP(hipMemcpyAsync(c->seam_rows_tab + c->B, wt.data(), sizeof(float) * overlap, hipMemcpyHostToDevice, s));
    MC_HIP(hipStreamSynchronize(s));                 // (the two vectors are temporaries)
    c->seam_rows_ov = overlap;
    c->seam_rows_right.assign(right, right + c->B);
    return MC_OK;
}

int mc_ctx_set_seams(mc_ctx* c, int32_t overlap, const int32_t* first_frame, const float* weight, void* stream) {
    MC_REQUIRE(c, "null context");
    if (overlap == 0) {
        if (c->seam_ov > 0) hist_set(c, false);       // (multistep sampler: the previous x0 belongs to the coupled walk)
        c->seam_ov = 0;
        return MC_OK;
    }
    if (int re = edit_refuse(c, "mc_ctx_set_seams")) return re;
    if (int rr = seam_rows_refuse(c, "mc_ctx_set_seams")) return rr;
    std::vector<int> flags;
    std::vector<float> wt;
    int r;
    if ((r = seam_plan("mc_ctx_set_seams", c->B, c->T, overlap, first_frame, weight, &flags, &wt))) return r;
    if (c->graph_exec) {
        mc_set_error("mc_ctx_set_seams: the context holds a captured graph of the uncoupled step (mc_ctx_graph_release first)");
        return MC_ERR_STATE;
    }
    if (!c->seam_tab && (r = ws_alloc(c, &c->seam_tab, (size_t)c->B + (size_t)c->T / 2)) != MC_OK) return r;
    hipStream_t s = (hipStream_t)stream;
    c->seam_ov = 0;
    MC_HIP(hipMemcpyAsync(c->seam_tab, flags.data(), sizeof(int) * c->B, hipMemcpyHostToDevice, s));
    MC_HIP(hipMemcpyAsync(c->seam_tab + c->B, wt.data(), sizeof(float) * overlap, hipMemcpyHostToDevice, s));
    MC_HIP(hipStreamSynchronize(s));                 // (the two vectors are temporaries)
    c->seam_ov = overlap;
    hist_set(c, false);
    return MC_OK;
}

int mc_sample_step(mc_ctx* c, const float* x_t, int32_t step, const mc_step_coefs* k, const float* noise,
                   float* x_prev, float* x0, void* stream) {
    MC_REQUIRE(c && x_t && k && x_prev, "null argument");
    int r;
    if ((r = edit_refuse(c, "mc_sample_step"))) return r;
    if (int rq = seam_rows_refuse(c, "mc_sample_step")) return rq;
    if ((r = check_mode(k))) return r;
    const bool ms = c->graph_mode ? c->graph_multistep : is_multistep(k);
    MC_REQUIRE(noise || ms, "null argument (noise_dev may be NULL in mode 2 only)");
    if (ms && !c->graph_mode) {
        if ((r = hist_require(c, k->eta, step))) return r;
        if ((r = hist_alloc(c))) return r;
    }
    X0Parts p;
    if ((r = denoise_combined(c, x_t, step, k, stream, &p))) return r;
    if ((r = sampler_update(c, x_t, p, k, noise, x_prev, x0, (hipStream_t)stream))) return r;
    if (ms && !c->graph_mode) hist_set(c, true);
    return MC_OK;
}

static RngArgs rng_args(uint64_t seed, uint64_t draw) {
    RngArgs r;
    r.seed_lo = (uint32_t)seed; r.seed_hi = (uint32_t)(seed >> 32); r.draw_lo = (uint32_t)draw; r.draw_hi = (uint32_t)(draw >> 32);
    return r;
}

// The whole p_sample_loop / ddim_sample_loop of the reference (gaussian_diffusion.py:698-797, 925-1049) as ONE call: x is updated in
// place through the schedule indices step_indices[0 .. num_steps) (the reference walks num_timesteps-1 .. 0), no return to the host
// language between steps.  The per-step randn_like (gaussian_diffusion.py:684, 847) is either read from noise_dev
// [num_steps][B,T,C] (parity runs on the reference's seeds) or, noise_dev == NULL, drawn inside the sampler-update kernel
// (Philox4x32-10, draw index noise_draw0 + k): no noise tensor, no generator launch.
int mc_sample_loop(mc_ctx* c, float* x, const int32_t* step_indices, const mc_step_coefs* coefs, int32_t num_steps,
                   const float* noise, uint64_t seed, uint64_t noise_draw0, float* x0_last, void* stream) {
    MC_REQUIRE(c && x && step_indices && coefs, "null argument");
    MC_REQUIRE(num_steps >= 0, "num_steps < 0");
    if (int re = edit_refuse(c, "mc_sample_loop")) return re;
    if (int rq = seam_rows_refuse(c, "mc_sample_loop")) return rq;
    const long n = (long)c->B * c->T * c->m->cfg.input_feats;
    // the sampler update of step k also writes x_{t-1} at the padded row stride the pose-encoder GEMM of step k + 1 stages from
    // (no pad_rows_k launch between the steps; the first step of a loop pads, which also zeroes the pad columns)
    PadOut po;
    po.xpad = c->xpad; po.C = c->m->cfg.input_feats; po.Cp = c->m->Cp;
    const bool fold_pad = c->xpad != nullptr;
    c->xpad_ready = false;
    for (int k = 0; k < num_steps; ++k) {
        int r = check_mode(&coefs[k]);
        if (r == MC_OK && is_multistep(&coefs[k])) r = hist_alloc(c);
        if (r != MC_OK) return r;
    }
    for (int k = 0; k < num_steps; ++k) {
        const bool ms = is_multistep(&coefs[k]);
        int r = ms ? hist_require(c, coefs[k].eta, step_indices[k]) : MC_OK;
        if (r != MC_OK) { c->xpad_ready = false; return r; }
        X0Parts p;
        r = denoise_combined(c, x, step_indices[k], &coefs[k], stream, &p);
        if (r != MC_OK) { c->xpad_ready = false; return r; }
        const RngArgs rng = rng_args(seed, noise_draw0 + (uint64_t)k);
        const bool more = fold_pad && k + 1 < num_steps;
        r = sampler_update(c, x, p, &coefs[k], noise ? noise + (long)k * n : nullptr, x, k + 1 == num_steps ? x0_last : nullptr, (hipStream_t)stream,
                           noise ? nullptr : &rng, more ? &po : nullptr);
        if (r != MC_OK) { c->xpad_ready = false; return r; }
        if (ms) hist_set(c, true);
        c->xpad_ready = more;
    }
    c->xpad_ready = false;
    return MC_OK;
}

// ---- row-keyed noise: the seed table of a context ----
int mc_ctx_set_row_seeds(mc_ctx* c, const uint64_t* seeds, void* stream) {
    MC_REQUIRE(c, "null context");
    if (!seeds) { c->row_seeds_set = false; return MC_OK; }
    int r;
    if (!c->row_seeds && (r = ws_alloc(c, &c->row_seeds, (size_t)c->B)) != MC_OK) return r;
    hipStream_t s = (hipStream_t)stream;
    c->row_seeds_set = false;
    MC_HIP(hipMemcpyAsync(c->row_seeds, seeds, sizeof(uint64_t) * c->B, hipMemcpyHostToDevice, s));
    MC_HIP(hipStreamSynchronize(s));                 // (the caller's array may be a temporary)
    c->row_seeds_host.assign(seeds, seeds + c->B);
    c->row_seeds_set = true;
    return MC_OK;
}
int mc_ctx_draw_rows(mc_ctx* c, float* out, uint64_t draw, void* stream) {
    MC_REQUIRE(c && out, "null argument");
    if (!c->row_seeds_set) { mc_set_error("mc_ctx_draw_rows: no seed table set (mc_ctx_set_row_seeds)"); return MC_ERR_STATE; }
    const long TC = (long)c->T * c->m->cfg.input_feats;
    MC_REQUIRE(TC <= 0x7fffffffL, "mc_ctx_draw_rows: a row of %ld floats", TC);
    return mc_launch_philox_rows_fill(out, c->B, RowKeys{reinterpret_cast<const uint32_t*>(c->row_seeds), (int)TC}, rng_args(0, draw), (hipStream_t)stream);
}

int mc_op_philox_normal(float* out, uint32_t* bits, int64_t n, uint64_t seed, uint64_t draw, void* stream) {
    MC_REQUIRE(out || bits, "null argument");
    return mc_launch_philox_fill(out, bits, n, rng_args(seed, draw), (hipStream_t)stream);
}

// ---- per-row schedules: every request row of the batch at its own schedule index and guidance scale ----
// Not in this mode: graph capture / replay (a context that holds a captured graph, or a capturing stream, is MC_ERR_STATE), the
// whole-batch seam table of mc_ctx_set_seams (MC_ERR_STATE), the inpaint and seeded steps (they have no rows entry).  Windows of a long
// request ARE in this mode, through the row seam table of mc_ctx_set_seam_rows (section 4q).
static int rows_refuse(const mc_ctx* c, const char* who, hipStream_t s) {
    if (c->graph_mode || c->graph_exec) {
        mc_set_error("%s: the context holds a captured graph (mc_ctx_graph_release first): row steps are not replayed", who);
        return MC_ERR_STATE;
    }
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) { (void)hipGetLastError(); st = hipStreamCaptureStatusNone; }
    if (st != hipStreamCaptureStatusNone) { mc_set_error("%s: the stream is capturing: row steps are not captured", who); return MC_ERR_STATE; }
    if (c->seam_ov > 0) { mc_set_error("%s: the context has a seam table set (mc_ctx_set_seams): clear it with overlap = 0", who); return MC_ERR_STATE; }
    if (!c->have_cond) { mc_set_error("%s: mc_ctx_set_condition not called", who); return MC_ERR_STATE; }
    return MC_OK;
}
// device tables [maxS][B] and their pinned staging, on the first call of the mode
static int rows_tables(mc_ctx* c) {
    if (c->rs_stage) return MC_OK;
    const size_t n = (size_t)c->maxS * c->B;
    int r;
    if (!c->rs_step && (r = ws_alloc(c, &c->rs_step, n)) != MC_OK) return r;
    if (!c->rs_coefs && (r = ws_alloc(c, &c->rs_coefs, n)) != MC_OK) return r;
    if (!c->rs_draw && (r = ws_alloc(c, &c->rs_draw, n)) != MC_OK) return r;
    if (!c->rs_ev) MC_HIP(hipEventCreateWithFlags(&c->rs_ev, hipEventDisableTiming));
    MC_HIP(hipHostMalloc(&c->rs_stage, n * (sizeof(int) + sizeof(SamplerCoefs) + sizeof(uint64_t)), hipHostMallocDefault));
    return MC_OK;
}
// n = ticks * B entries of each table -> staging -> device on `s`.  The staging is free once the previous upload's copies are done:
// the call waits for the event behind them, never for the device.
static int rows_upload(mc_ctx* c, size_t n, const int32_t* step, const mc_step_coefs* coefs, const uint64_t* draw, hipStream_t s) {
    const size_t cap = (size_t)c->maxS * c->B;
    MC_HIP(hipEventSynchronize(c->rs_ev));      // (never recorded: returns at once)
    uint64_t* sd = reinterpret_cast<uint64_t*>(c->rs_stage);
    SamplerCoefs* sc = reinterpret_cast<SamplerCoefs*>(sd + cap);
    int* si = reinterpret_cast<int*>(sc + cap);
    for (size_t i = 0; i < n; ++i) si[i] = step[i];
    MC_HIP(hipMemcpyAsync(c->rs_step, si, sizeof(int) * n, hipMemcpyHostToDevice, s));
    if (coefs) {
        for (size_t i = 0; i < n; ++i) sc[i] = to_coefs(&coefs[i]);
        MC_HIP(hipMemcpyAsync(c->rs_coefs, sc, sizeof(SamplerCoefs) * n, hipMemcpyHostToDevice, s));
    }
    if (draw) {
        for (size_t i = 0; i < n; ++i) sd[i] = draw[i];
        MC_HIP(hipMemcpyAsync(c->rs_draw, sd, sizeof(uint64_t) * n, hipMemcpyHostToDevice, s));
    }
    MC_HIP(hipEventRecord(c->rs_ev, s));
    return MC_OK;
}
static RowTab rows_tick(const mc_ctx* c, int k) {
    RowTab t;
    t.step = c->rs_step + (size_t)k * c->B; t.coefs = c->rs_coefs + (size_t)k * c->B; t.draw = c->rs_draw + (size_t)k * c->B;
    t.B = c->B; t.T = c->T;
    return t;
}

int mc_denoise_rows(mc_ctx* c, const float* x_t, const int32_t* step_index, float* out2_dev, void* stream) {
    MC_REQUIRE(c && x_t && step_index, "null argument");
    hipStream_t s = (hipStream_t)stream;
    int r;
    if ((r = rows_refuse(c, "mc_denoise_rows", s))) return r;
    for (int b = 0; b < c->B; ++b)
        MC_REQUIRE(step_index[b] >= 0 && step_index[b] < c->S, "row %d: step_index %d outside the %d-step schedule", b, step_index[b], c->S);
    if ((r = rows_tables(c))) return r;
    if ((r = rows_upload(c, (size_t)c->B, step_index, nullptr, nullptr, s))) return r;
    c->rowtab = rows_tick(c, 0);
    c->rows_mode = true;
    r = denoise_impl(c, x_t, 0, out2_dev, -1, stream, nullptr);
    c->rows_mode = false;
    return r;
}

int mc_sample_rows(mc_ctx* c, float* x, int32_t num_ticks, const int32_t* step_index, const mc_step_coefs* coefs, const uint64_t* draw,
                   const float* noise, float* x0_last, void* stream) {
    MC_REQUIRE(c && x && step_index && coefs, "null argument");
    MC_REQUIRE(num_ticks >= 0 && num_ticks <= c->maxS, "num_ticks=%d outside [0, max_steps=%d]", num_ticks, c->maxS);
    hipStream_t s = (hipStream_t)stream;
    int r;
    if ((r = rows_refuse(c, "mc_sample_rows", s))) return r;
    if (num_ticks == 0) return MC_OK;
    const int B = c->B;
    const size_t ne = (size_t)num_ticks * B;
    // every check before the first launch: a refused call leaves the context as it found it
    for (size_t i = 0; i < ne; ++i) {
        if ((r = check_mode(&coefs[i]))) return r;
        MC_REQUIRE(coefs[i].mode == coefs[0].mode, "tick %d row %d: sampler mode %d beside mode %d (one mode per call)", (int)(i / B), (int)(i % B),
                   coefs[i].mode, coefs[0].mode);
        MC_REQUIRE(step_index[i] >= 0 && step_index[i] < c->S, "tick %d row %d: step_index %d outside the %d-step schedule", (int)(i / B), (int)(i % B),
                   step_index[i], c->S);
    }
    const bool ms = is_multistep(&coefs[0]);
    MC_REQUIRE(!(c->edit_set && coefs[0].mode == MC_SAMPLER_DDIM && noise),
               "mc_sample_rows: with an edit table set, mode 1 takes noise_dev == NULL (the kept region's noise is a draw of the row's seed)");
    if (!ms && !noise) {
        if (!c->row_seeds_set) { mc_set_error("mc_sample_rows: noise_dev == NULL needs a seed table (mc_ctx_set_row_seeds)"); return MC_ERR_STATE; }
        MC_REQUIRE(draw, "mc_sample_rows: noise_dev == NULL needs draw_host");
    }
    std::vector<uint8_t> flags = c->hist_rows;
    flags.resize((size_t)B, 0);
    // a row seam table (mc_ctx_set_seam_rows): the two rows of a seam walk together -- equal step index, coefficient bytes and draw
    // number in every tick, one seed, one history flag.  The kernel then takes the owner's (the left row's) entry for both.
    if (c->seam_rows_ov > 0) {
        for (int b = 0; b < B; ++b) {
            const int rb = c->seam_rows_right[b];
            if (rb < 0) continue;
            for (int k = 0; k < num_ticks; ++k) {
                const size_t i = (size_t)k * B + b, j = (size_t)k * B + rb;
                MC_REQUIRE(step_index[i] == step_index[j] && memcmp(&coefs[i], &coefs[j], sizeof(mc_step_coefs)) == 0,
                           "mc_sample_rows: tick %d: rows %d and %d share a seam but not their step index / coefficients", k, b, rb);
                MC_REQUIRE(ms || noise || draw[i] == draw[j], "mc_sample_rows: tick %d: rows %d and %d share a seam but not their draw number", k, b, rb);
            }
            MC_REQUIRE(ms || noise || c->row_seeds_host[b] == c->row_seeds_host[rb],
                       "mc_sample_rows: rows %d and %d share a seam but not their seed (every row of a request carries the request's)", b, rb);
            MC_REQUIRE(!ms || flags[b] == flags[rb], "mc_sample_rows: rows %d and %d share a seam but not their multistep history flag", b, rb);
        }
    }
    if (ms) {
        for (size_t i = 0; i < ne; ++i) {
            const int b = (int)(i % B);
            if (coefs[i].eta != 0.f && !flags[b]) {
                mc_set_error("mc_sample_rows: tick %d, row %d reads the previous x0 (k1 = %g) but holds none: no multistep step of this row since its "
                             "condition was set", (int)(i / B), b, (double)coefs[i].eta);
                return MC_ERR_STATE;
            }
            flags[b] = 1;
        }
        if ((r = hist_alloc(c))) return r;
    }
    if ((r = rows_tables(c))) return r;
    if ((r = rows_upload(c, ne, step_index, coefs, !ms && !noise ? draw : nullptr, s))) return r;
    const long n = (long)B * c->T * c->m->cfg.input_feats;
    PadOut po;
    po.xpad = c->xpad; po.C = c->m->cfg.input_feats; po.Cp = c->m->Cp;
    const bool fold_pad = c->xpad != nullptr;
    c->xpad_ready = false;
    const RngArgs rng;         // (rows mode reads the draw numbers from the table)
    r = MC_OK;
    int ran = 0;               // ticks whose launches were all enqueued
    for (int k = 0; k < num_ticks && r == MC_OK; ++k) {
        const mc_step_coefs* ck = coefs + (size_t)k * B;
        c->rowtab = rows_tick(c, k);
        c->rows_mode = true;
        X0Parts p;
        r = denoise_combined(c, x, 0, ck, stream, &p);
        const bool more = fold_pad && k + 1 < num_ticks;
        if (r == MC_OK)
            r = sampler_update(c, x, p, ck, noise ? noise + (long)k * n : nullptr, x, k + 1 == num_ticks ? x0_last : nullptr, s,
                               noise || ms ? nullptr : &rng, more ? &po : nullptr);
        c->rows_mode = false;
        c->xpad_ready = r == MC_OK && more;
        if (r == MC_OK) ++ran;
    }
    c->xpad_ready = false;
    // a launch failure in tick k leaves x and the history advanced by ticks [0, k): their flags are kept (every tick updates every row)
    if (ms && ran == num_ticks) c->hist_rows = flags;
    else if (ms && ran > 0) c->hist_rows.assign((size_t)B, 1);
    return r;
}

int mc_ctx_set_condition_rows(mc_ctx* c, const float* xf_out_dev, const float* mask_dev, const uint8_t* fresh, void* stream) {
    MC_REQUIRE(c && xf_out_dev && mask_dev && fresh, "null argument");
    std::vector<uint8_t> keep = c->hist_rows;
    keep.resize((size_t)c->B, 0);
    const int r = mc_ctx_set_condition(c, xf_out_dev, mask_dev, stream);      // (clears the context's flag and every row's)
    if (r != MC_OK) return r;
    for (int b = 0; b < c->B; ++b) c->hist_rows[b] = fresh[b] ? 0 : keep[b];
    return MC_OK;
}

// The kept region of every request row: rows with fresh[b] != 0 (NULL: all) are copied device to device into the
// context's tables on `s`; the others keep what they hold.  The tables are zeroed when they are allocated, so a row never set keeps nothing.
int mc_ctx_set_edit_rows(mc_ctx* c, const float* gt, const uint8_t* keep, const uint8_t* fresh, void* stream) {
    MC_REQUIRE(c, "null context");
    if (!gt && !keep) {
        // nothing stays kept behind a clear: a later upload of some fresh rows must not bring a retired row's region back
        if (c->edit_keep) MC_HIP(hipMemsetAsync(c->edit_keep, 0, (size_t)c->B * c->T * c->m->cfg.input_feats, (hipStream_t)stream));
        c->edit_set = false;
        return MC_OK;
    }
    MC_REQUIRE(gt && keep, "mc_ctx_set_edit_rows: gt_dev and keep_dev are both given, or both NULL (which clears the table)");
    if (c->graph_mode || c->graph_exec) {
        mc_set_error("mc_ctx_set_edit_rows: the context holds a captured graph (mc_ctx_graph_release first): edited rows are not replayed");
        return MC_ERR_STATE;
    }
    if (c->seam_ov > 0) { mc_set_error("mc_ctx_set_edit_rows: the context has a seam table set (mc_ctx_set_seams): clear it with overlap = 0"); return MC_ERR_STATE; }
    if (!c->long_edits) { if (int rq = seam_rows_refuse(c, "mc_ctx_set_edit_rows")) return rq; }
    const size_t TC = (size_t)c->T * c->m->cfg.input_feats, n = (size_t)c->B * TC;
    hipStream_t s = (hipStream_t)stream;
    int r;
    if (!c->edit_gt) {
        if ((r = ws_alloc(c, &c->edit_gt, n)) != MC_OK) return r;
        MC_HIP(hipMemsetAsync(c->edit_gt, 0, sizeof(float) * n, s));
    }
    if (!c->edit_keep) {
        if ((r = ws_alloc(c, &c->edit_keep, n)) != MC_OK) return r;
        MC_HIP(hipMemsetAsync(c->edit_keep, 0, n, s));
    }
    for (int b = 0; b < c->B;) {          // one copy per run of fresh rows
        if (fresh && !fresh[b]) { ++b; continue; }
        int e = b + 1;
        while (e < c->B && (!fresh || fresh[e])) ++e;
        MC_HIP(hipMemcpyAsync(c->edit_gt + b * TC, gt + b * TC, sizeof(float) * TC * (e - b), hipMemcpyDeviceToDevice, s));
        MC_HIP(hipMemcpyAsync(c->edit_keep + b * TC, keep + b * TC, TC * (e - b), hipMemcpyDeviceToDevice, s));
        b = e;
    }
    c->edit_set = true;
    return MC_OK;
}

// Kept regions on long requests: the one switch under which the edit table and the row seam table may be set
// side by side.  Off (the default) each refuses the other as ever.  No table, no history flag is touched.
int mc_ctx_set_long_edits(mc_ctx* c, int32_t on) {
    MC_REQUIRE(c, "null context");
    if (!on && c->edit_set && c->seam_rows_ov > 0) {
        mc_set_error("mc_ctx_set_long_edits: the context has an edit table and a row seam table set: clear one of them first");
        return MC_ERR_STATE;
    }
    c->long_edits = on != 0;
    return MC_OK;
}

// ---- hipGraph replay of mc_sample_step -------------------------------------------------------------------------------
int mc_ctx_graph_capture(mc_ctx* c, float* x_dev, const float* noise_dev, const mc_step_coefs* coefs_host, int32_t num_steps,
                         void* stream) {
    MC_REQUIRE(c && x_dev && coefs_host, "null argument");
    if (int rs = seam_refuse(c, "mc_ctx_graph_capture")) return rs;
    if (int re = edit_refuse(c, "mc_ctx_graph_capture")) return re;
    if (int rq = seam_rows_refuse(c, "mc_ctx_graph_capture")) return rq;
    MC_REQUIRE(c->have_cond, "mc_ctx_set_condition not called");
    MC_REQUIRE(num_steps >= 1 && num_steps == c->S, "num_steps=%d must equal the schedule set by mc_ctx_set_timesteps (%d)", num_steps, c->S);
    MC_REQUIRE(!c->cap_idx, "routing capture (tests) and graph replay are mutually exclusive");
    hipStream_t s = (hipStream_t)stream;
    MC_REQUIRE(s != nullptr, "graph capture needs a non-default stream");
    int r;
    // the update kernel is baked into the graph and the mode comes from the device table: one graph per table, all of it mode 2 or none of it
    int n_ms = 0;
    for (int i = 0; i < num_steps; ++i) {
        if ((r = check_mode(&coefs_host[i]))) return r;
        n_ms += is_multistep(&coefs_host[i]) ? 1 : 0;
    }
    MC_REQUIRE(n_ms == 0 || n_ms == num_steps, "the table mixes mode 2 (%d entries) with other modes (%d): capture one graph per table", n_ms, num_steps - n_ms);
    MC_REQUIRE(noise_dev || n_ms, "null argument (noise_dev may be NULL for a mode-2 table only)");
    graph_release(c);
    if (n_ms && (r = hist_alloc(c))) return r;
    c->graph_multistep = n_ms != 0;
    c->graph_k1.assign(num_steps, 0.f);
    for (int i = 0; i < num_steps; ++i) c->graph_k1[i] = n_ms ? coefs_host[i].eta : 0.f;
    if (!c->gstep && (r = ws_alloc(c, &c->gstep, 1)) != MC_OK) return r;
    if (!c->gcoefs && (r = ws_alloc(c, &c->gcoefs, (size_t)c->maxS)) != MC_OK) return r;
    std::vector<SamplerCoefs> tab(num_steps);
    for (int i = 0; i < num_steps; ++i) tab[i] = to_coefs(&coefs_host[i]);
    MC_HIP(hipMemcpyAsync(c->gcoefs, tab.data(), sizeof(SamplerCoefs) * num_steps, hipMemcpyHostToDevice, s));
    MC_HIP(hipMemsetAsync(c->gstep, 0, sizeof(int), s));
    MC_HIP(hipStreamSynchronize(s));                 // (`tab` is a temporary)
    MC_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    c->graph_mode = true;
    c->cnt_clean = false;        // a replay must not assume anything about the routing counts it starts from: the first gate clears them
    r = mc_sample_step(c, x_dev, 0, &coefs_host[0], noise_dev, x_dev, nullptr, stream);     // in place: x_prev aliases x_t
    c->graph_mode = false;
    c->cnt_clean = false;        // (nothing of the captured step ran)
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(s, &g);
    if (r != MC_OK) { if (g) (void)hipGraphDestroy(g); return r; }
    if (e != hipSuccess || !g) { mc_set_error("hipStreamEndCapture: %s", hipGetErrorString(e)); return MC_ERR_HIP; }
    c->graph = g;
    const hipError_t ei = hipGraphInstantiate(&c->graph_exec, g, nullptr, nullptr, 0);
    if (ei != hipSuccess) { mc_set_error("hipGraphInstantiate: %s", hipGetErrorString(ei)); graph_release(c); return MC_ERR_HIP; }
    c->graph_steps = num_steps;
    return MC_OK;
}

int mc_ctx_graph_step(mc_ctx* c, int32_t step, void* stream) {
    MC_REQUIRE(c, "null context");
    if (int re = edit_refuse(c, "mc_ctx_graph_step")) return re;
    if (int rq = seam_rows_refuse(c, "mc_ctx_graph_step")) return rq;
    MC_REQUIRE(c->graph_exec, "no captured graph (mc_ctx_graph_capture)");
    MC_REQUIRE(step >= 0 && step < c->graph_steps, "step_index %d outside the %d captured steps", step, c->graph_steps);
    hipStream_t s = (hipStream_t)stream;
    int r;
    if (c->graph_multistep && (r = hist_require(c, c->graph_k1[step], step))) return r;
    if ((r = mc_launch_set_int(c->gstep, step, s))) return r;
    MC_HIP(hipGraphLaunch(c->graph_exec, s));
    if (c->graph_multistep) hist_set(c, true);
    return MC_OK;
}

int mc_ctx_graph_release(mc_ctx* c) {
    MC_REQUIRE(c, "null context");
    graph_release(c);
    return MC_OK;
}

int mc_sample_step_seeded(mc_ctx* c, float* x_t, int32_t step, const mc_step_coefs* k, const float* noise,
                          const mc_seed* sd, float* x_prev, float* x0, void* stream) {
    MC_REQUIRE(c && x_t && k && noise && x_prev && sd, "null argument");
    if (int rs = seam_refuse(c, "mc_sample_step_seeded")) return rs;
    if (int re = edit_refuse(c, "mc_sample_step_seeded")) return re;
    if (int rq = seam_rows_refuse(c, "mc_sample_step_seeded")) return rq;
    MC_REQUIRE(!is_multistep(k), "mc_sample_step_seeded: the multistep sampler (mode 2) has no pre_seq / transl_req seeding");
    MC_REQUIRE(sd->pre_len >= 0 && sd->pre_len <= c->T, "pre_seq has %d frames, the window %d", sd->pre_len, c->T);
    MC_REQUIRE(sd->num_transl >= 0 && sd->num_transl <= MC_MAX_TRANSL, "num_transl=%d outside [0, %d]", sd->num_transl, MC_MAX_TRANSL);
    MC_REQUIRE(sd->num_transl == 0 || c->T >= 2, "transl_req seeds frames 0 and 1: the window has %d", c->T);
    SeedArgs a;
    a.pre = sd->pre_seq_dev; a.pre_noise = sd->pre_noise_dev; a.pre_len = sd->pre_len; a.T = c->T;
    a.sqrt_ab = sd->sqrt_ab; a.sqrt_1mab = sd->sqrt_1mab; a.num_transl = sd->num_transl;
    for (int i = 0; i < sd->num_transl; ++i) {
        MC_REQUIRE(sd->transl_channel[i] >= 0 && sd->transl_channel[i] < c->m->cfg.input_feats, "transl_req channel %d", sd->transl_channel[i]);
        a.transl_channel[i] = sd->transl_channel[i];
        a.transl_value[i][0] = sd->transl_value[i][0];
        a.transl_value[i][1] = sd->transl_value[i][1];
    }
    X0Parts p;
    if (int r = denoise_combined(c, x_t, step, k, stream, &p, &a)) return r;
    const long n = (long)c->B * c->T * c->m->cfg.input_feats;
    SamplerForm f;
    f.x_t = x_t; f.out_text = p.a; f.out_none = p.second(); f.noise = noise; f.x_prev = x_prev; f.x0_out = x0; f.n = n;
    f.c = p.coefs(k); f.mode = MC_SAMPLER_DDPM;          // (multistep is refused above: sampler_update_k, which reads the entry's own mode)
    return mc_launch_sampler(f, (hipStream_t)stream);
}

int mc_sample_step_inpaint(mc_ctx* c, const float* x_t, int32_t step, const mc_step_coefs* k, const float* noise,
                           const mc_inpaint* ip, float* x_prev, float* x0, void* stream) {
    MC_REQUIRE(c && x_t && k && noise && x_prev && ip, "null argument");
    if (int rs = seam_refuse(c, "mc_sample_step_inpaint")) return rs;
    if (int re = edit_refuse(c, "mc_sample_step_inpaint")) return re;
    if (int rq = seam_rows_refuse(c, "mc_sample_step_inpaint")) return rq;
    MC_REQUIRE(!is_multistep(k), "mc_sample_step_inpaint: the multistep sampler (mode 2) has no outpainting (RePaint) form");
    X0Parts p;
    if (int r = denoise_combined(c, x_t, step, k, stream, &p)) return r;
    const int C = c->m->cfg.input_feats;
    const long n = (long)c->B * c->T * C;
    InpaintArgs a;
    a.gt = ip->gt_dev; a.keep = ip->keep_dev; a.gt_noise = ip->gt_noise_dev; a.blend_w = ip->blend_w_dev;
    a.blend_len = ip->blend_len; a.T = c->T; a.C = C;
    MC_REQUIRE(a.blend_len >= 0 && a.blend_len <= c->T, "blend_len %d outside the %d-frame window", a.blend_len, c->T);
    return mc_launch_sampler_inpaint(x_t, p.a, p.second(), noise, a, x_prev, x0, n, p.coefs(k), (hipStream_t)stream);
}

int mc_postprocess_smplx(const float* pred, const int32_t* lengths, const double* mean, const double* stdv,
                         const double* taps, const int32_t radius[4], int32_t stats_f32, int32_t B, int32_t T, int32_t C,
                         double* poses, double* expr, double* trans, void* stream) {
    MC_REQUIRE(pred && mean && stdv && taps && radius && poses && expr && trans, "null argument");
    static_assert(MC_POST_MAXTAP == 129, "header / kernel tap table size");
    MC_REQUIRE(mc_smplx_post_maxtap() == MC_POST_MAXTAP, "tap table size mismatch");
    return mc_launch_smplx_post(pred, lengths, nullptr, mean, stdv, taps, radius, stats_f32, B, T, C, poses, expr, trans,
                                (hipStream_t)stream);
}

int mc_postprocess_smplx_stitched(const float* pred, const int32_t* rows, int32_t n_frames, const double* mean,
                                  const double* stdv, const double* taps, const int32_t radius[4], int32_t stats_f32,
                                  int32_t C, double* poses, double* expr, double* trans, void* stream) {
    MC_REQUIRE(pred && rows && mean && stdv && taps && radius && poses && expr && trans && n_frames >= 0, "bad argument");
    MC_REQUIRE(mc_smplx_post_maxtap() == MC_POST_MAXTAP, "tap table size mismatch");
    return mc_launch_smplx_post(pred, nullptr, rows, mean, stdv, taps, radius, stats_f32, 1, n_frames, C, poses, expr,
                                trans, (hipStream_t)stream);
}

int mc_postprocess_t2m_joints(const float* pred, const int32_t* lengths, const double* mean, const double* stdv,
                              const double* taps, int32_t radius, int32_t stats_f32, int32_t B, int32_t T, int32_t C,
                              int32_t joints_num, float* joints, void* stream) {
    MC_REQUIRE(pred && mean && stdv && joints && (taps || radius < 0), "null argument");
    MC_REQUIRE(mc_smplx_post_maxtap() == MC_POST_MAXTAP, "tap table size mismatch");
    return mc_launch_t2m_joints(pred, lengths, nullptr, mean, stdv, taps, radius, stats_f32, B, T, C, joints_num, nullptr,
                                joints, (hipStream_t)stream);
}

int mc_postprocess_t2m_joints_stitched(const float* pred, const int32_t* rows, int32_t n_frames, const double* mean,
                                       const double* stdv, const double* taps, int32_t radius, int32_t stats_f32,
                                       int32_t C, int32_t joints_num, double* work, float* joints, void* stream) {
    MC_REQUIRE(pred && rows && mean && stdv && work && joints && (taps || radius < 0) && n_frames >= 0, "bad argument");
    MC_REQUIRE(mc_smplx_post_maxtap() == MC_POST_MAXTAP, "tap table size mismatch");
    return mc_launch_t2m_joints(pred, nullptr, rows, mean, stdv, taps, radius, stats_f32, 1, n_frames, C, joints_num, work,
                                joints, (hipStream_t)stream);
}

int mc_op_renoise(const float* x, const float* noise, float a, float b, float* out, int64_t n, void* stream) {
    MC_REQUIRE(x && noise && out && n >= 0, "bad argument");
    return mc_launch_axpby(x, noise, a, b, out, (long)n, (hipStream_t)stream);
}

int mc_ctx_get_buffer(mc_ctx* c, const char* name, int32_t layer, void** dev_ptr, int64_t* numel) {
    MC_REQUIRE(c && name && dev_ptr && numel, "null argument");
    const mc_model_config& g = c->m->cfg;
    const int L = g.latent_dim, H = g.num_parts, D = L * H;
    const std::string n(name);
    void* p = nullptr;
    int64_t cnt = 0;
    if (n == "h") { p = c->h; cnt = c->rows * D; }
    else if (n == "z") { p = c->z; cnt = c->N * L; }
    else if (n == "proj") { p = c->proj; cnt = c->N * 256; }
    else if (n == "mf") { p = c->mf; cnt = c->N * 4 * L; }
    else if (n == "qkv") { p = c->qkv; cnt = c->N * 3 * L; }
    else if (n == "y2") { p = c->y2; cnt = c->N * 2 * L; }
    else if (n == "ys") { p = c->ys; cnt = c->rows * D; }
    else if (n == "yt") { p = c->yt; cnt = c->rows * D; }
    else if (n == "a") {
        // reduced-precision contexts keep fp16 hi | lo PLANES in `a` (film_block): not the fp32 [rows][D] rows this call promises
        MC_REQUIRE(!a_holds_planes(c), "buffer 'a' holds fp16 planes in a reduced-precision context (clear chain bit 17 to read fp32 rows)");
        p = c->a; cnt = c->rows * D;
    }
    else if (n == "a_tail") { p = deferred_a(c); cnt = c->rows * D; }
    else if (n == "z2") { p = c->z2; cnt = c->rows * D; }
    else if (n == "out2") { p = c->out2; cnt = c->rows * g.input_feats; }
    else if (n == "emb") { p = c->emb; cnt = (int64_t)c->S * g.time_embed_dim; }
    else if (n == "ss") { p = c->ss + (long)layer * c->maxS * 2 * D; cnt = (int64_t)c->S * 2 * D; }
    else if (n == "tf") { p = c->tf + (long)layer * c->Ntxt * 2 * L; cnt = c->Ntxt * 2 * L; }
    else if (n == "idx") { p = c->rb.idx; cnt = 2 * c->N; }
    else if (n == "gate") { p = c->rb.gate; cnt = 2 * c->N; }
    else if (n == "comb_w") { p = c->rb.comb_w; cnt = 2 * c->N; }
    else if (n == "key") { p = c->rb.key; cnt = c->N; }
    else if (n == "hc" && c->hc) { p = c->hc; cnt = c->rows * D; }
    else if (n == "cb" && c->cb) { p = c->cb; cnt = c->rows * D; }
    else if (n == "cap_idx" && c->cap_idx) { p = c->cap_idx + (long)layer * 2 * c->N; cnt = 2 * c->N; }
    else if (n == "cap_w" && c->cap_w) { p = c->cap_w + (long)layer * 2 * c->N; cnt = 2 * c->N; }
    else if (n == "x0_hist") {
        if (!c->x0_hist) { mc_set_error("buffer 'x0_hist' does not exist before the context's first multistep (mode 2) call"); return MC_ERR_STATE; }
        p = c->x0_hist; cnt = (int64_t)c->B * c->T * g.input_feats;
    }
    else if (n == "src_row") { p = c->rb.src_row; cnt = 2 * c->N; }
    else if (n == "dst_row") { p = c->rb.dst_row; cnt = 2 * c->N; }
    else if (n == "tile_group") { p = c->rb.tile_group; cnt = 2L * c->rb.max_tiles; }
    else if (n == "tile_row0") { p = c->rb.tile_row0; cnt = 2L * c->rb.max_tiles; }
    else if (n == "tile_nrows") { p = c->rb.tile_nrows; cnt = 2L * c->rb.max_tiles; }
    else if (n == "num_tiles") { p = const_cast<int*>(mc_route_num_tiles_ptr(c->rb, 0)); cnt = 2; }
    else if (n == "route_split") { p = const_cast<int*>(mc_route_split_flag_ptr(c->rb)); cnt = 1; }
    else { mc_set_error("unknown buffer '%s'", name); return MC_ERR_ARG; }
    *dev_ptr = p;
    *numel = cnt;
    return MC_OK;
}

int mc_op_gemm(const float* a, const float* w, const float* bias, const float* res, float* cdev, int32_t M, int32_t N,
               int32_t K, int32_t ldw, int32_t act, void* stream) {
    MC_REQUIRE(a && w && cdev && M > 0 && N > 0 && K > 0 && K % 4 == 0 && ldw % 4 == 0 && ldw >= K, "bad gemm args");
    return dense(nullptr, a, K, w, ldw, bias, res, N, cdev, N, M, N, K, act, (hipStream_t)stream);
}

int mc_op_gemm_strided(int32_t mode, int32_t groups, const mc_gemm_strided* a, void* stream) {
    MC_REQUIRE(a && (mode == GM_PLAIN || mode == GM_ENC) && groups >= 1, "gemm_strided: mode %d (0 plain, 4 encoder), groups %d", mode, groups);
    MC_REQUIRE(a->a_dev && a->w_dev && a->c_dev && a->M > 0 && a->N > 0 && a->K > 0 && a->lda > 0 && a->ldc >= a->N && a->ldw >= a->K &&
                   a->ldw % 4 == 0 && a->add_mod >= 1 && a->dup_rows >= 0 && (!a->res_dev || a->ldr >= a->N) && (!a->add_dev || a->ld_add >= a->N),
               "bad gemm_strided args");
    GemmArgs g;
    g.A = a->a_dev; g.lda = a->lda; g.a_gstride = a->a_gstride;
    g.W = a->w_dev; g.ldw = a->ldw; g.w_gstride = a->w_gstride;
    g.bias = a->bias_dev; g.b_gstride = a->b_gstride;
    g.C = a->c_dev; g.ldc = a->ldc; g.c_gstride = a->c_gstride;
    g.R = a->res_dev; g.ldr = a->ldr; g.r_gstride = a->r_gstride;
    g.act = a->act; g.act_after_res = a->act_after_res;
    g.add = a->add_dev; g.add_mod = a->add_mod; g.ld_add = a->ld_add; g.dup_rows = a->dup_rows;
    g.M = a->M; g.N = a->N; g.K = a->K;
    return mc_launch_gemm(mode, g, groups, 0, (hipStream_t)stream);
}

// the two fp16 GEMM ops: `g` holds the A operand (fp32 rows or fp16 planes); the fp32 weight is split into temporary planes here
static int gemm_f16_op(GemmHArgs g, const float* w, const float* bias, const float* res, float* cdev, int M, int N, int K, bool split, hipStream_t s) {
    mc_half* planes = nullptr;
    MC_HIP(hipMalloc((void**)&planes, sizeof(mc_half) * 2 * (size_t)N * K));
    int r = mc_launch_split_f16(w, planes, planes + (size_t)N * K, (long)N * K, s);
    if (r == MC_OK) {
        g.Wh = planes; g.Wl = planes + (size_t)N * K; g.bias = bias; g.R = res; g.ldr = N; g.C = cdev; g.ldc = N;
        g.M = M; g.N = N; g.K = K;
        r = mc_launch_gemm_h(g, split, s);
    }
    (void)hipStreamSynchronize(s);
    (void)hipFree(planes);
    return r;
}

int mc_op_gemm_f16(const float* a, const float* w, const float* bias, const float* res, float* cdev, int32_t M, int32_t N,
                   int32_t K, int32_t split, void* stream) {
    MC_REQUIRE(a && w && cdev && M > 0 && N > 0 && K > 0, "bad gemm args");
    GemmHArgs g;
    g.A = a; g.lda = K;
    return gemm_f16_op(g, w, bias, res, cdev, M, N, K, split != 0, (hipStream_t)stream);
}

int mc_op_gemm_f16_planes(const void* a_hi, const void* a_lo, const float* w, const float* bias, const float* res, float* cdev, int32_t M,
                          int32_t N, int32_t K, int32_t split, int32_t pre, int32_t frag_major, void* stream) {
    MC_REQUIRE(a_hi && (!split || a_lo) && w && cdev && M > 0 && N > 0 && K > 0, "bad gemm args");
    GemmHArgs g;
    g.Ah = (const mc_half*)a_hi; g.Al = (const mc_half*)a_lo; g.a_fm = frag_major != 0; g.pre = pre != 0;
    return gemm_f16_op(g, w, bias, res, cdev, M, N, K, split != 0, (hipStream_t)stream);
}

int mc_op_gemm_tail(const float* h, const float* a, const float* w, const float* bias, float* cdev, float* c2dev, int32_t M, int32_t N,
                    int32_t K, float wc, float wu, int32_t variant, void* stream) {
    MC_REQUIRE(h && a && w && bias && cdev && M > 0 && N > 0 && K > 0 && K % 32 == 0, "bad gemm_tail args");
    MC_REQUIRE(variant >= 0 && variant <= 2, "gemm_tail variant %d (0 default, 1 column tiles, 2 block ranges)", variant);
    TailArgs t;
    t.H = h; t.Af = a; t.half = (long)M * K; t.lda = K; t.W = w; t.ldw = K; t.w_gstride = (long)N * K; t.bias = bias; t.b_gstride = N;
    t.C = cdev; t.ldc = N; t.M = M; t.N = N; t.K = K; t.wc = wc; t.wu = wu;
    const McOptions* o = mc_process_options();
    if (!o) return MC_ERR_ARG;
    t.tune = (int)o->gemm_tune;
    if (variant) t.tune = variant == 1 ? (t.tune & ~kTuneTail2) : (t.tune | kTuneTail2);
    t.C2 = c2dev;
    MC_REQUIRE(variant != 2 || c2dev, "gemm_tail variant 2 needs the scratch output c2_dev [M][N]");
    MC_REQUIRE(variant != 2 || mc_gemm_tail_two_outputs(t),
               "gemm_tail variant 2: the block-range form is not eligible for M=%d N=%d K=%d (N <= 336, K %% 16 == 0, K >= 48, <= 17 blocks per wave)", M, N, K);
    int r = mc_launch_gemm_tail(t, (hipStream_t)stream);
    if (r == MC_OK && mc_gemm_tail_two_outputs(t))       // the sampler-update kernel adds the two partial products in the step; here: C += C2
        r = mc_launch_axpby(cdev, c2dev, 1.f, 1.f, cdev, (long)M * N, (hipStream_t)stream);
    return r;
}

int mc_op_ln_rows(const float* x, int64_t ldx, const float* gamma, const float* beta, const float* add, int32_t add_mod,
                  float* y, int64_t rows, int32_t L, void* stream) {
    return mc_launch_ln_rows(x, ldx, 0, gamma, beta, add, add_mod, y, L, rows, L, (hipStream_t)stream);
}

int mc_op_body_attention(const float* mf, int64_t ldmf, const float* qkv, const float* wsm, float* ys, int64_t frames, int32_t H, int32_t L,
                         int64_t twin_from, const int32_t* split_flag, int64_t frame0, void* stream) {
    MC_REQUIRE(mf && qkv && wsm && ys && frames >= 0 && ldmf >= L && twin_from >= 0 && frame0 >= 0, "bad body_attention args");
    TwinAlias alias;
    alias.split_flag = split_flag;
    alias.from = twin_from;
    return mc_launch_body(mf, ldmf, qkv, wsm, ys, frames, H, L, 8, (hipStream_t)stream, alias, frame0);
}

int mc_op_temporal_attention(const float* mf, const float* tf, const float* mask, float* yt, int32_t b0, int32_t nb, int32_t B, int32_t T,
                             int32_t Nt, int32_t H, int32_t L, int32_t form, int32_t skip_text, const int32_t* twin_flag, void* stream) {
    MC_REQUIRE(mf && tf && mask && yt && B > 0 && T > 0 && Nt > 0 && H > 0 && b0 >= 0 && nb >= 0 && b0 + nb <= 2 * B,
               "bad temporal_attention args");
    MC_REQUIRE(L == 32 || L == 64 || L == 128, "temporal_attention: latent_dim=%d unsupported (32, 64, 128)", L);
    hipStream_t s = (hipStream_t)stream;
    const bool sk = skip_text != 0;
    switch (form) {
    case MC_TEMPORAL_STEP: {         // the fp32 step's own choice
        const McOptions* o = mc_process_options();
        if (!o) return MC_ERR_ARG;
        return mc_launch_temporal(mf, tf, mask, yt, b0, nb, B, T, Nt, H, L, s, twin_flag, o->temporal_split, (o->chain >> kChainTemporalPair) & 1, sk);
    }
    case MC_TEMPORAL_WHOLE:
        return mc_launch_temporal(mf, tf, mask, yt, b0, nb, B, T, Nt, H, L, s, twin_flag, -1, false, sk);
    case MC_TEMPORAL_LSPLIT:
        MC_REQUIRE(L >= 64, "temporal_attention form LSPLIT: no column-sliced kernel at latent_dim=%d (64, 128)", L);
        return mc_launch_temporal(mf, tf, mask, yt, b0, nb, B, T, Nt, H, L, s, twin_flag, (long)nb * H, false, sk);
    case MC_TEMPORAL_PAIR:
        MC_REQUIRE(L == 64 && H % 2 == 0, "temporal_attention form PAIR: no two-part kernel at latent_dim=%d, num_parts=%d (64, even)", L, H);
        return mc_launch_temporal(mf, tf, mask, yt, b0, nb, B, T, Nt, H, L, s, twin_flag, -1, true, sk);
    case MC_TEMPORAL_F16X3:
    case MC_TEMPORAL_F16:
        MC_REQUIRE(L >= 64, "temporal_attention form %s: no fp16 kernel at latent_dim=%d (64, 128)", form == MC_TEMPORAL_F16X3 ? "F16X3" : "F16", L);
        return mc_launch_temporal_h(mf, tf, mask, yt, b0, nb, B, T, Nt, H, L, form == MC_TEMPORAL_F16X3, s, twin_flag, sk);
    }
    mc_set_error("temporal_attention: form %d (0 step, 1 WHOLE, 2 LSPLIT, 3 PAIR, 4 F16X3, 5 F16)", form);
    return MC_ERR_ARG;
}

// ---- the sampler family as context-free ops (tests, tools): every form through mc_launch_sampler ----
static SamplerForm op_form(const float* x_t, const float* ot, const float* on, const float* noise, float* x0_hist, float* x_prev, float* x0, long n,
                           const mc_step_coefs* k) {
    SamplerForm f;
    f.x_t = x_t; f.out_text = ot; f.out_none = on; f.x_prev = x_prev; f.x0_out = x0; f.n = n;
    f.c = to_coefs(k);
    f.mode = k->mode;
    if (is_multistep(k)) f.x0_hist = x0_hist; else f.noise = noise;
    return f;
}

int mc_op_sampler_update(const float* x_t, const float* ot, const float* on, const float* noise, float* x_prev, float* x0,
                         int64_t n, const mc_step_coefs* k, void* stream) {
    MC_REQUIRE(x_t && ot && on && noise && x_prev && k, "null argument");
    SamplerForm f = op_form(x_t, ot, on, noise, nullptr, x_prev, x0, n, k);
    f.noise = noise; f.mode = MC_SAMPLER_DDPM;          // (this entry is sampler_update_k whatever k->mode says: the kernel reads the entry's own mode)
    return mc_launch_sampler(f, (hipStream_t)stream);
}

int mc_op_sampler_multistep(const float* x_t, const float* ot, const float* on, float* x0_hist, float* x_prev, float* x0, int64_t n,
                            const mc_step_coefs* k, void* stream) {
    MC_REQUIRE(x_t && ot && on && x0_hist && x_prev && k && n >= 0, "bad argument");
    MC_REQUIRE(is_multistep(k), "mc_op_sampler_multistep: coefficients of mode %d (MC_SAMPLER_MULTISTEP = 2 expected)", k->mode);
    return mc_launch_sampler(op_form(x_t, ot, on, nullptr, x0_hist, x_prev, x0, n, k), (hipStream_t)stream);
}

// A temporary device table of an op entry: uploaded before the launch, given back on every path once the stream has drained (the
// launch reads it), so the ops that take one synchronise.
}  // extern "C"
namespace {
struct TempTable {
    void* p = nullptr;
    hipStream_t s;
    explicit TempTable(hipStream_t s_) : s(s_) {}
    TempTable(const TempTable&) = delete;
    TempTable& operator=(const TempTable&) = delete;
    ~TempTable() {
        (void)hipStreamSynchronize(s);
        if (p) (void)hipFree(p);
    }
    int alloc(size_t bytes, const char* what) {
        if (hipMalloc(&p, bytes) == hipSuccess) return MC_OK;
        p = nullptr;
        mc_set_error("%s: temporary table allocation failed", what);
        return MC_ERR_HIP;
    }
    int upload(const void* host, size_t bytes, const char* what, const void* more = nullptr, size_t more_bytes = 0) {      // (`more`: a second piece right behind the first)
        if (int r = alloc(bytes + more_bytes, what)) return r;
        if (hipMemcpyAsync(p, host, bytes, hipMemcpyHostToDevice, s) == hipSuccess &&
            (!more_bytes || hipMemcpyAsync(static_cast<char*>(p) + bytes, more, more_bytes, hipMemcpyHostToDevice, s) == hipSuccess) &&
            hipStreamSynchronize(s) == hipSuccess) return MC_OK;
        mc_set_error("%s: temporary table upload failed", what);
        return MC_ERR_HIP;
    }
};
}  // namespace
extern "C" {
// the per-row forms: one mode per call ...
static int rows_one_mode(const char* what, const mc_step_coefs* coefs, int B) {
    for (int b = 0; b < B; ++b) {
        if (int r = check_mode(&coefs[b])) return r;
        MC_REQUIRE(coefs[b].mode == coefs[0].mode, "%s: row %d in mode %d beside mode %d (one mode per call)", what, b, coefs[b].mode, coefs[0].mode);
    }
    return MC_OK;
}
// ... their coefficient table rt->coefs [B] ...
static int rows_tab_upload(const char* what, const mc_step_coefs* coefs, int B, TempTable* t, RowTab* rt) {
    std::vector<SamplerCoefs> tab((size_t)B);
    for (int b = 0; b < B; ++b) tab[b] = to_coefs(&coefs[b]);
    if (int r = t->upload(tab.data(), sizeof(SamplerCoefs) * B, what)) return r;
    rt->coefs = static_cast<const SamplerCoefs*>(t->p);
    return MC_OK;
}
// ... and, for noise drawn in the kernel, [B] keys | [B] draw numbers (rk->keys, rt->draw)
static int rows_keys_upload(const char* what, const uint64_t* seeds, const uint64_t* draw, int B, int TC, TempTable* t, RowTab* rt, RowKeys* rk) {
    std::vector<uint64_t> h((size_t)2 * B);
    for (int b = 0; b < B; ++b) { h[b] = seeds[b]; h[(size_t)B + b] = draw[b]; }
    if (int r = t->upload(h.data(), sizeof(uint64_t) * 2 * B, what)) return r;
    rk->keys = static_cast<const uint32_t*>(t->p); rk->TC = TC;
    rt->draw = static_cast<const uint64_t*>(t->p) + B;
    return MC_OK;
}

int mc_op_gemm_tail_rows(const float* h, const float* a, const float* w, const float* bias, float* cdev, float* c2dev, int32_t M, int32_t N,
                         int32_t K, const mc_step_coefs* coefs, int32_t T, int32_t variant, void* stream) {
    MC_REQUIRE(h && a && w && bias && cdev && coefs && M > 0 && N > 0 && K > 0 && K % 32 == 0, "bad gemm_tail_rows args");
    MC_REQUIRE(T > 0 && M % T == 0, "gemm_tail_rows: M=%d rows are no whole request rows of T=%d", M, T);
    MC_REQUIRE(variant >= 1 && variant <= 3, "gemm_tail_rows variant %d (1 column tiles, 2 block ranges, 3 pair combine + grouped GEMM)", variant);
    MC_REQUIRE(variant == 1 || c2dev, "gemm_tail_rows variants 2 and 3 need the scratch output c2_dev [M][N]");
    hipStream_t s = (hipStream_t)stream;
    const McOptions* o = mc_process_options();
    if (!o) return MC_ERR_ARG;
    RowTab rt;
    rt.B = M / T; rt.T = T;
    TempTable tab(s), scratch(s);
    int r;
    if ((r = rows_tab_upload("gemm_tail_rows", coefs, rt.B, &tab, &rt))) return r;
    if (variant == 3) {
        // the small-batch form of denoise_combined: h_c | a_c by axpby_pair_rows_k, then the two skinny products as one grouped GEMM
        const long MK = (long)M * K;
        if ((r = scratch.alloc(sizeof(float) * 2 * MK, "gemm_tail_rows"))) return r;
        float* const comb = static_cast<float*>(scratch.p);
        r = mc_launch_axpby_pair_rows(h, h + MK, comb, a, a + MK, comb + MK, rt, K, MK, s);
        GemmArgs t;
        mc_gemm_opts(*o, t);
        t.A = comb; t.lda = K; t.a_gstride = MK; t.W = w; t.ldw = K; t.w_gstride = (long)N * K;
        t.bias = bias; t.b_gstride = N; t.C = cdev; t.ldc = N; t.c_gstride = (long)(c2dev - cdev);
        t.M = M; t.N = N; t.K = K;
        if (r == MC_OK) r = mc_launch_gemm_small(t, s, 2);
        if (r == MC_OK) r = mc_launch_axpby(cdev, c2dev, 1.f, 1.f, cdev, (long)M * N, s);
    } else {
        TailArgs t;
        t.H = h; t.Af = a; t.half = (long)M * K; t.lda = K; t.W = w; t.ldw = K; t.w_gstride = (long)N * K; t.bias = bias; t.b_gstride = N;
        t.C = cdev; t.ldc = N; t.M = M; t.N = N; t.K = K; t.C2 = c2dev;
        t.coef_table = reinterpret_cast<const float*>(rt.coefs) + offsetof(SamplerCoefs, text_coef) / sizeof(float);
        t.coef_stride = sizeof(SamplerCoefs) / sizeof(float);
        t.rows_T = T; t.rows_B = rt.B;
        t.tune = variant == 1 ? ((int)o->gemm_tune & ~kTuneTail2) : ((int)o->gemm_tune | kTuneTail2);
        if (variant == 2 && !mc_gemm_tail_two_outputs(t)) {
            mc_set_error("gemm_tail_rows variant 2: the block-range form is not eligible for M=%d N=%d K=%d", M, N, K);
            r = MC_ERR_ARG;
        }
        if (r == MC_OK) r = mc_launch_gemm_tail(t, s);
        if (r == MC_OK && mc_gemm_tail_two_outputs(t)) r = mc_launch_axpby(cdev, c2dev, 1.f, 1.f, cdev, (long)M * N, s);
    }
    return r;
}

int mc_op_sampler_rows(const float* x_t, const float* ot, const float* on, const float* noise, float* x0_hist, float* x_prev, float* x0,
                       int32_t B, int32_t TC, const mc_step_coefs* coefs, void* stream) {
    MC_REQUIRE(x_t && ot && on && x_prev && coefs && B >= 1 && TC >= 1, "mc_op_sampler_rows: bad argument");
    int r;
    if ((r = rows_one_mode("mc_op_sampler_rows", coefs, B))) return r;
    MC_REQUIRE(is_multistep(&coefs[0]) ? x0_hist != nullptr : noise != nullptr, "mc_op_sampler_rows: mode 2 needs x0_hist_dev, the other modes noise_dev");
    hipStream_t s = (hipStream_t)stream;
    RowTab rt;
    rt.B = B; rt.T = 1;
    TempTable tab(s);
    if ((r = rows_tab_upload("mc_op_sampler_rows", coefs, B, &tab, &rt))) return r;
    SamplerForm f = op_form(x_t, ot, on, noise, x0_hist, x_prev, x0, (long)B * TC, &coefs[0]);
    f.c.text_coef = f.c.none_coef = 1.f;
    f.rt = &rt; f.TC = TC;
    return mc_launch_sampler(f, s);
}

int mc_op_sampler_edit_rows(const float* x_t, const float* ot, const float* on, const float* noise, const float* gt_noise, const float* gt,
                            const uint8_t* keep, const uint64_t* seeds, const uint64_t* draw, float* x0_hist, float* x_prev, float* x0, int32_t B,
                            int32_t TC, const mc_step_coefs* coefs, void* stream) {
    MC_REQUIRE(x_t && ot && on && gt && keep && x_prev && coefs && B >= 1 && TC >= 1, "mc_op_sampler_edit_rows: bad argument");
    int r;
    if ((r = rows_one_mode("mc_op_sampler_edit_rows", coefs, B))) return r;
    const bool ms = is_multistep(&coefs[0]);
    const bool dev_rng = seeds != nullptr || draw != nullptr;
    if (ms) MC_REQUIRE(x0_hist && !noise && !gt_noise && !dev_rng, "mc_op_sampler_edit_rows: mode 2 needs x0_hist_dev and takes no noise");
    else {
        MC_REQUIRE(!dev_rng || (seeds && draw && !noise && !gt_noise), "mc_op_sampler_edit_rows: (seeds_host, draw_host) come together and exclude the noise tensors");
        MC_REQUIRE(dev_rng || noise, "mc_op_sampler_edit_rows: modes 0 / 1 need noise_dev, or (seeds_host, draw_host)");
        MC_REQUIRE(dev_rng || coefs[0].mode == MC_SAMPLER_DDPM || gt_noise, "mc_op_sampler_edit_rows: mode 1 beside noise_dev needs gt_noise_dev");
    }
    hipStream_t s = (hipStream_t)stream;
    RowTab rt;
    rt.B = B; rt.T = 1;
    RowKeys rk;
    TempTable tab(s), kd(s);
    if ((r = rows_tab_upload("mc_op_sampler_edit_rows", coefs, B, &tab, &rt))) return r;
    if (dev_rng && (r = rows_keys_upload("mc_op_sampler_edit_rows", seeds, draw, B, TC, &kd, &rt, &rk))) return r;
    EditTab et;
    et.gt = gt; et.keep = keep; et.gt_noise = gt_noise;
    SamplerForm f = op_form(x_t, ot, on, noise, x0_hist, x_prev, x0, (long)B * TC, &coefs[0]);
    f.c.text_coef = f.c.none_coef = 1.f;
    f.rt = &rt; f.TC = TC; f.edit = &et;
    if (dev_rng) f.keys = &rk;
    return mc_launch_sampler(f, s);
}

int mc_op_sampler_seam(const float* x_t, const float* ot, const float* on, const float* noise, uint64_t seed, uint64_t draw, float* x0_hist,
                       float* x_prev, float* x0, int32_t B, int32_t T, int32_t C, int32_t overlap, const int32_t* first_frame,
                       const float* weight, const mc_step_coefs* k, void* stream) {
    MC_REQUIRE(x_t && ot && on && x_prev && k && C >= 1, "mc_op_sampler_seam: bad argument");
    int r;
    if ((r = check_mode(k))) return r;
    const bool ms = is_multistep(k);
    MC_REQUIRE(ms || !noise || (seed == 0 && draw == 0), "mc_op_sampler_seam: noise_dev and a Philox draw (seed / draw) are mutually exclusive");
    MC_REQUIRE(!ms || x0_hist, "mc_op_sampler_seam: mode 2 needs x0_hist_dev");
    std::vector<int> flags;
    std::vector<float> wt;
    if ((r = seam_plan("mc_op_sampler_seam", B, T, overlap, first_frame, weight, &flags, &wt))) return r;
    hipStream_t s = (hipStream_t)stream;
    // one temporary block: [B] flags | [overlap] weights
    TempTable tab(s);
    if ((r = tab.upload(flags.data(), sizeof(int) * B, "mc_op_sampler_seam", wt.data(), sizeof(float) * overlap))) return r;
    SeamTab st;
    st.flags = static_cast<const int*>(tab.p); st.w = reinterpret_cast<const float*>(st.flags + B); st.T = T; st.C = C; st.ov = overlap;
    const RngArgs rng = rng_args(seed, draw);
    SamplerForm f = op_form(x_t, ot, on, noise, x0_hist, x_prev, x0, (long)B * T * C, k);
    f.seam = &st;
    if (!noise) f.rng = &rng;
    return mc_launch_sampler(f, s);
}

int mc_op_sampler_seam_rows(const float* x_t, const float* ot, const float* on, const float* noise, const uint64_t* seeds, const uint64_t* draw,
                            float* x0_hist, float* x_prev, float* x0, int32_t B, int32_t T, int32_t C, int32_t overlap, const int32_t* right,
                            const int32_t* first_frame, const float* weight, const mc_step_coefs* coefs, void* stream) {
    MC_REQUIRE(x_t && ot && on && x_prev && coefs && B >= 1 && C >= 1, "mc_op_sampler_seam_rows: bad argument");
    int r;
    if ((r = rows_one_mode("mc_op_sampler_seam_rows", coefs, B))) return r;
    const bool ms = is_multistep(&coefs[0]);
    const bool dev_rng = seeds != nullptr || draw != nullptr;
    if (ms) MC_REQUIRE(x0_hist && !noise && !dev_rng, "mc_op_sampler_seam_rows: mode 2 needs x0_hist_dev and takes no noise");
    else {
        MC_REQUIRE(!dev_rng || (seeds && draw && !noise), "mc_op_sampler_seam_rows: (seeds_host, draw_host) come together and exclude noise_dev");
        MC_REQUIRE(dev_rng || noise, "mc_op_sampler_seam_rows: modes 0 / 1 need noise_dev, or (seeds_host, draw_host)");
    }
    std::vector<SeamRow> rows;
    std::vector<float> wt;
    if ((r = seam_rows_plan("mc_op_sampler_seam_rows", B, T, overlap, right, first_frame, weight, &rows, &wt))) return r;
    for (int b = 0; b < B; ++b) {
        const int rb = right[b];
        if (rb < 0) continue;
        MC_REQUIRE(memcmp(&coefs[b], &coefs[rb], sizeof(mc_step_coefs)) == 0, "mc_op_sampler_seam_rows: rows %d and %d share a seam but not their coefficients", b, rb);
        MC_REQUIRE(!dev_rng || (seeds[b] == seeds[rb] && draw[b] == draw[rb]), "mc_op_sampler_seam_rows: rows %d and %d share a seam but not their seed / draw number", b, rb);
    }
    hipStream_t s = (hipStream_t)stream;
    RowTab rt;
    rt.B = B; rt.T = 1;
    RowKeys rk;
    TempTable tab(s), blk(s), kd(s);
    if ((r = rows_tab_upload("mc_op_sampler_seam_rows", coefs, B, &tab, &rt))) return r;
    if (dev_rng && (r = rows_keys_upload("mc_op_sampler_seam_rows", seeds, draw, B, (int)((long)T * C), &kd, &rt, &rk))) return r;
    // one temporary block: [B] SeamRow | [overlap] weights
    if ((r = blk.upload(rows.data(), sizeof(SeamRow) * B, "mc_op_sampler_seam_rows", wt.data(), sizeof(float) * overlap))) return r;
    SeamRowsTab st;
    st.rows = static_cast<const SeamRow*>(blk.p); st.w = reinterpret_cast<const float*>(st.rows + B); st.T = T; st.C = C; st.ov = overlap;
    SamplerForm f = op_form(x_t, ot, on, noise, x0_hist, x_prev, x0, (long)B * T * C, &coefs[0]);
    f.c.text_coef = f.c.none_coef = 1.f;
    f.rt = &rt; f.seam_rows = &st;
    if (dev_rng) f.keys = &rk;
    return mc_launch_sampler(f, s);
}

// mc_op_sampler_seam_rows with a kept region (sampler_seam_edit_rows_k): the noise sources follow mc_op_sampler_edit_rows
int mc_op_sampler_seam_edit_rows(const float* x_t, const float* ot, const float* on, const float* noise, const float* gt_noise, const float* gt,
                                 const uint8_t* keep, const uint64_t* seeds, const uint64_t* draw, float* x0_hist, float* x_prev, float* x0,
                                 int32_t B, int32_t T, int32_t C, int32_t overlap, const int32_t* right, const int32_t* first_frame,
                                 const float* weight, const mc_step_coefs* coefs, void* stream) {
    MC_REQUIRE(x_t && ot && on && gt && keep && x_prev && coefs && B >= 1 && C >= 1, "mc_op_sampler_seam_edit_rows: bad argument");
    int r;
    if ((r = rows_one_mode("mc_op_sampler_seam_edit_rows", coefs, B))) return r;
    const bool ms = is_multistep(&coefs[0]);
    const bool dev_rng = seeds != nullptr || draw != nullptr;
    if (ms) MC_REQUIRE(x0_hist && !noise && !gt_noise && !dev_rng, "mc_op_sampler_seam_edit_rows: mode 2 needs x0_hist_dev and takes no noise");
    else {
        MC_REQUIRE(!dev_rng || (seeds && draw && !noise && !gt_noise), "mc_op_sampler_seam_edit_rows: (seeds_host, draw_host) come together and exclude the noise tensors");
        MC_REQUIRE(dev_rng || noise, "mc_op_sampler_seam_edit_rows: modes 0 / 1 need noise_dev, or (seeds_host, draw_host)");
        MC_REQUIRE(dev_rng || coefs[0].mode == MC_SAMPLER_DDPM || gt_noise, "mc_op_sampler_seam_edit_rows: mode 1 beside noise_dev needs gt_noise_dev");
    }
    std::vector<SeamRow> rows;
    std::vector<float> wt;
    if ((r = seam_rows_plan("mc_op_sampler_seam_edit_rows", B, T, overlap, right, first_frame, weight, &rows, &wt))) return r;
    for (int b = 0; b < B; ++b) {
        const int rb = right[b];
        if (rb < 0) continue;
        MC_REQUIRE(memcmp(&coefs[b], &coefs[rb], sizeof(mc_step_coefs)) == 0, "mc_op_sampler_seam_edit_rows: rows %d and %d share a seam but not their coefficients", b, rb);
        MC_REQUIRE(!dev_rng || (seeds[b] == seeds[rb] && draw[b] == draw[rb]), "mc_op_sampler_seam_edit_rows: rows %d and %d share a seam but not their seed / draw number", b, rb);
    }
    hipStream_t s = (hipStream_t)stream;
    RowTab rt;
    rt.B = B; rt.T = 1;
    RowKeys rk;
    TempTable tab(s), blk(s), kd(s);
    if ((r = rows_tab_upload("mc_op_sampler_seam_edit_rows", coefs, B, &tab, &rt))) return r;
    if (dev_rng && (r = rows_keys_upload("mc_op_sampler_seam_edit_rows", seeds, draw, B, (int)((long)T * C), &kd, &rt, &rk))) return r;
    if ((r = blk.upload(rows.data(), sizeof(SeamRow) * B, "mc_op_sampler_seam_edit_rows", wt.data(), sizeof(float) * overlap))) return r;
    SeamRowsTab st;
    st.rows = static_cast<const SeamRow*>(blk.p); st.w = reinterpret_cast<const float*>(st.rows + B); st.T = T; st.C = C; st.ov = overlap;
    EditTab et;
    et.gt = gt; et.keep = keep; et.gt_noise = gt_noise;
    SamplerForm f = op_form(x_t, ot, on, noise, x0_hist, x_prev, x0, (long)B * T * C, &coefs[0]);
    f.c.text_coef = f.c.none_coef = 1.f;
    f.rt = &rt; f.seam_rows = &st; f.edit = &et;
    if (dev_rng) f.keys = &rk;
    return mc_launch_sampler(f, s);
}

}  // extern "C"
