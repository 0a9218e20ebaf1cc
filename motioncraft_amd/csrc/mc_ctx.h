// The model / context handles of libmotioncraft_amd.so and what the two translation units that work on them share: mc_model.hip (weight
// binding, option table, context life cycle, graph capture, the extern "C" entry points) and mc_step.hip (the per-step kernel schedule).
//
// HBM layout (all fp32, row-major; B2 = 2B CFG-doubled batch, N = B2*T*H tokens, rows = B2*T):
//   h    [rows, D]      residual stream (text-conditioned half first, stmogen.py:736-744)
//   z    [N, L]         LN(x) + motion_moe.embedding            proj [N, 256] cosine projector out
//   hbuf [2N, 4L]       expert hidden, slot-major               y2   [N, 2, L] expert outputs per choice
//   mf   [N, 4L]        [body_value | key | value | query]      qkv  [N, 3L]   dynamic-topology q,k,v
//   ys/yt/a/z2 [rows,D] static+dynamic / temporal / FiLM prologue / SFFN output
//   fh   [rows, H*F]    SFFN hidden                             out2 [rows, C]  pose decoder output
//   tf[layer] [B2*Nt, 2L]  step-invariant text K/V              ss[layer][blk][S][2D] FiLM scale|shift
#pragma once
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/motioncraft_amd.h"
#include "mc_common.h"
#include "mc_gemm.h"
#include "mc_kernels.h"
#include "mc_chain.h"
#include "mc_half.h"
#include "mc_options.h"
#include "mc_params.h"

struct mc_model {
    mc_model_config cfg;
    ParamStore params{""};
    std::map<std::string, HalfW> half;     // built on the first mc_ctx_set_precision(.., MC_PREC_F16*) (shared by all contexts)
    std::mutex half_mu;                    // guards `half` (filled from per-context calls)
    size_t half_bytes = 0;                 // device bytes of the fp16 hi / lo planes (reported by mc_ctx_workspace_bytes of a reduced-precision context)
    bool finalized = false;
    int Cp = 0;  // input_feats padded to a multiple of 32 (row stride of enc.w and of the padded pose rows)
};

struct MoeW {
    const float *emb, *gate_w, *gate_b, *sim_n, *sim_nT, *scale, *fc1_w, *fc1_b, *fc2_wt, *fc2_b, *proj_w, *proj_b;
    int din, dout;
};

struct LayerW {
    const float *norm_g, *norm_b, *tnorm_g, *tnorm_b, *wsm;
    MoeW mm, tm;
    const float *dyn_g, *dyn_b, *qkv_w, *qkv_b;
    const float *ca_film_w, *ca_film_b, *ca_ln_g, *ca_ln_b, *ca_out_w, *ca_out_b;
    const float *ffn_w1, *ffn_b1, *ffn_w2, *ffn_b2;
    const float *ffn_film_w, *ffn_film_b, *ffn_ln_g, *ffn_ln_b, *ffn_out_w, *ffn_out_b;
    // control-branch copies only (ControlT2MBlock): zero-init projections around the copied DecoderLayer
    const float *before_w = nullptr, *before_b = nullptr, *after_w = nullptr, *after_b = nullptr;
    // fp16 planes of the per-step GEMM weights (reduced-precision mode; null until mc_ctx_set_precision builds them)
    HalfW h_ca_out, h_ffn_out, h_fc1, h_fc2, h_w1, h_w2, h_after, h_proj, h_qkv;
};

struct ProfRec { hipEvent_t e0 = nullptr, e1 = nullptr; long rows = 0; };

struct mc_ctx {
    mc_model* m = nullptr;
    McOptions opt{};             // kernel selection (mc_ctx_set_option), seeded by mc_ctx_create from the option table
    int B = 0, T = 0, S = 0, maxS = 0;
    long N = 0, rows = 0, Ntxt = 0;
    std::vector<LayerW> lw;
    const float *enc_w, *enc_b, *seq_emb, *time_w0, *time_b0, *time_w2, *time_b2, *dec_w, *dec_b;
    const float *dec_wf = nullptr, *dec_bf = nullptr;   // decoder folded with the last StylizationBlock Linear (optional)
    float *dec_cat_w = nullptr, *dec_cat_b = nullptr;   // [2][C][D] = dec_w | dec_wf and [2][C] = dec_bf | 0: the folded tail as ONE grouped GEMM
    const float *ctrl_in_w = nullptr, *ctrl_in_b = nullptr;
    int NLA = 0;                 // base + control layers (weights, text K/V and FiLM tables are per layer slot)
    float *hc = nullptr, *cb = nullptr, *cenc = nullptr;   // control stream, before_proj(c) [rows,D], forward_c(c) [B*T,D]
    bool have_ctrl = false;
    // workspace
    std::vector<void*> allocs;
    int64_t bytes = 0;
    float *h, *z, *proj, *hbuf, *y2, *mf, *qkv, *ys, *yt, *a, *z2, *fh, *out2, *xpad;
    // reduced-precision contexts: the fp32 rows of the DEFERRED last FiLM block (defer_last_gemm) get their own array -- `a` holds the
    // fp16 hi | lo planes of BOTH sample groups there, and fp32 rows written into it by one group's stream would land on the plane rows
    // the other group's gemm_hd_k may still be reading; null in fp32 contexts (then `a` itself holds fp32 rows only)
    float* a_tail = nullptr;
    size_t hbuf_cap = 0;        // floats allocated behind hbuf
    size_t hbuf_floats = 0;     // > 0: hbuf is free scratch (fused expert path), used for split-K partial sums
    bool cnt_clean = false;     // the routing state's (choice, expert) counts are known to be zero on the stream (route_small_k cleans up after itself)
    long led_nsrc = 0, led_gsplit = 0;      // FLOP ledger only: routed source tokens of the last routing and its slot-group boundary
    float *xfn, *tf;          // tf: [NL][B2*Nt][2L]
    const float* mask = nullptr;   // = mask_own after mc_ctx_set_condition (a private copy: the pointer is baked into captured graphs)
    float* mask_own = nullptr;
    int* t_orig;
    float *te, *e1, *emb, *semb, *ss;   // ss: [NL][2][maxS][2D]
    RouteBufs rb;
    int device = 0;             // the HIP device the context was created on (reservations are per device)
    int coop_reserved = 0;      // resident route_coop_k workgroups this context holds (mc_route_coop_reserve)
    bool prof_on = false;       // mc_ctx_profile: HIP events around the FiLM out_layers GEMM launches (bench.py's dominant-kernel figure)
    std::vector<ProfRec> prof;
    bool have_cond = false;
    // side stream: the temporal branch of STMA needs only the motion-MoE output, so it runs beside
    // (LN + qkv -> body attention) of the same layer (fork after the MoE projection, join before proj_out);
    // large batches: the second sample group (CFG half) runs on it, the first one on the caller's stream
    hipStream_t side = nullptr;
    bool xpad_ready = false;           // mc_sample_loop: xpad already holds this step's padded x_t (written by the previous sampler update)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev_side = nullptr;      // the side stream's work so far (recorded on it for a join / cross-join)
    hipEvent_t ev_stag = nullptr;      // chain bit 26: the first group's first FiLM row kernel is done (the second group's tail starts behind it)
    // early routing (option route_early, run_layer): the second group's gate and slot fill are done / the whole-batch selection is done /
    // the twin layer's second CFG half has read the first half's expert rows (the next layer's experts overwrite them)
    hipEvent_t ev_gate1 = nullptr, ev_sel = nullptr, ev_front = nullptr;
    bool early_clean = false;   // both groups' counts and fill cursors are known to be zero on the stream (the selection-only routing cleans up after itself)
    bool no_alias = false;          // introspection runs (stop_after_layers < num_layers): every intermediate row is materialised
    bool defer_last_gemm = false;   // sampler entry points: the last FiLM GEMM runs on the CFG-combined rows (see denoise_combined)
    // Two HIP streams only overlap when the runtime maps them to different HARDWARE queues (GPU_MAX_HW_QUEUES, default 4, handed out round-robin as streams
    // are created): with an RCCL process group initialised in the host process the caller's stream and the one side stream of round 5 landed on the SAME
    // queue and the two-stream schedule ran serially (+7 % step time at B=64: 19.05 -> 20.47 ms, profiles/r06_hw_queue_collision.txt).  The context creates
    // SIDE_CAND candidates back to back (they cover consecutive queues) and times, once per caller stream, which of them really runs beside it.
    static constexpr int SIDE_CAND = 4;
    hipStream_t side_cand[SIDE_CAND] = {nullptr, nullptr, nullptr, nullptr};
    hipStream_t side_for = nullptr;         // the caller stream the current `side` was picked for
    bool side_picked = false;
    float side_probe_ms[SIDE_CAND] = {0.f, 0.f, 0.f, 0.f};
    // earlier answers (a host that alternates between a few caller streams must not re-probe -- and re-synchronise -- on every call)
    static constexpr int SIDE_MEMO = 4;
    hipStream_t side_memo_for[SIDE_MEMO] = {nullptr, nullptr, nullptr, nullptr};
    int side_memo_pick[SIDE_MEMO] = {-1, -1, -1, -1};
    int side_memo_n = 0;
    // hipGraph replay of the sampler step (mc_ctx_graph_capture / _step): ONE graph for all steps of the schedule; the step
    // index lives in device memory (gstep) and the per-step tables are addressed inside the kernels (StepRef)
    int* gstep = nullptr;
    SamplerCoefs* gcoefs = nullptr;     // [S] schedule coefficients of every step
    bool graph_mode = false;            // set while capturing: launch with device-indexed step parameters
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    int graph_steps = 0;
    // multistep sampler (mode 2): the x0 of the step taken before, [B,T,C]; null until the context's first mode-2 call allocates it
    float* x0_hist = nullptr;
    bool hist_valid = false;            // x0_hist holds the x0 of the previous step of THIS condition / schedule (a mode-2 step sets it)
    bool graph_multistep = false;       // the captured graph's table is mode 2 (a graph is captured for one table: its update kernel is fixed)
    std::vector<float> graph_k1;        // ... and its k1 per schedule index: mc_ctx_graph_step checks hist_valid on the host
    // window coupling (mc_ctx_set_seams): while seam_ov > 0 sampler_update launches sampler_seam_k.  One device block, allocated by the
    // first call that sets a table: [B] neighbour flags (ints), then [T / 2] right-window weights (floats)
    int* seam_tab = nullptr;
    int seam_ov = 0;
    // independent requests: the capacity factor every MoE of this context routes with (the model's unless
    // mc_ctx_set_capacity_factor changed it; 0 = nothing dropped), and the rows' Philox keys [B] (allocated by the first mc_ctx_set_row_seeds)
    float cap_factor = 0.f;
    bool keep_all = false;      // set by mc_ctx_set_capacity_factor(0) only: a MODEL whose own factor is 0 keeps today's meaning (capacity 0)
    uint64_t* row_seeds = nullptr;
    bool row_seeds_set = false;
    // per-row schedules (mc_sample_rows / mc_denoise_rows).  rows_mode is set for the launches of one tick only:
    // film_block, denoise_combined and sampler_update then hand `rowtab` (the tick's slices of the device tables) to the same kernel
    // forms they pick anyway.  The tables [maxS][B] and their pinned staging are allocated by the first call of the mode; rs_ev is
    // recorded behind every upload, so the next call waits for that copy alone before it rewrites the staging.
    bool rows_mode = false;
    RowTab rowtab;
    int* rs_step = nullptr;
    SamplerCoefs* rs_coefs = nullptr;
    uint64_t* rs_draw = nullptr;
    void* rs_stage = nullptr;           // pinned: [maxS][B] ints | SamplerCoefs | uint64
    hipEvent_t rs_ev = nullptr;
    std::vector<uint8_t> hist_rows;     // multistep "history valid" per request row (all cleared / set wherever hist_valid is)
    // edited rows (mc_ctx_set_edit_rows): the kept region per request row, gt [B,T,C] floats and keep [B,T,C]
    // bytes, allocated by the first call that sets a table.  While edit_set, sampler_update launches the edit kernels in rows mode and
    // every entry without a rows form refuses (edit_refuse).
    float* edit_gt = nullptr;
    uint8_t* edit_keep = nullptr;
    bool edit_set = false;
    // seam-coupled windows in rows mode (mc_ctx_set_seam_rows): one device block, allocated by the first call
    // that sets a table and replaced as a whole by every later one -- [B] SeamRow entries, then [T / 2] right-window weights.  While
    // seam_rows_ov > 0 sampler_update launches sampler_seam_rows_k in rows mode and every entry without a rows form refuses
    // (seam_rows_refuse).  seam_rows_right is the host's copy of right[]: mc_sample_rows checks that the two rows of a seam carry equal
    // entries; row_seeds_host (mc_ctx_set_row_seeds) lets it check that they carry one seed.
    SeamRow* seam_rows_tab = nullptr;
    int seam_rows_ov = 0;
    std::vector<int> seam_rows_right;
    std::vector<uint64_t> row_seeds_host;
    // kept regions on long requests (mc_ctx_set_long_edits): off, the edit table and the row seam table refuse
    // each other; on, both may be set and sampler_update launches sampler_seam_edit_rows_k in rows mode
    bool long_edits = false;
    int prec = MC_PREC_F32;     // MFMA operand precision of the per-step GEMM-shaped kernels (mc_ctx_set_precision)
    int* cap_idx = nullptr;      // [NL][2N] routing capture (tests): expert ids ...
    float* cap_w = nullptr;      // ... and combine weights (0 = dropped) of every layer
};

// ---- shared by mc_model.hip and mc_step.hip (defined in mc_step.hip; hidden: not part of the library's dynamic symbol list) ----
#pragma GCC visibility push(hidden)
inline bool chain_on(const mc_ctx* c, ChainBit which) { return (c->opt.chain >> which) & 1; }
bool use_half(const mc_ctx* c);
int dense(const mc_ctx* c, const float* A, long lda, const float* W, long ldw, const float* bias, const float* R, long ldr,
          float* C, long ldc, long M, int N, int K, int act, hipStream_t s);
int run_moe(mc_ctx* c, const MoeW& w, const float* z, long Ntok, float* out, long ldout, bool gated, bool twin, long gsplit,
            hipStream_t s, const HalfW* hw, const HalfW* hw2);
// the multistep history flags: the context's one and every request row's move together wherever an entry of the uniform mode sets or
// clears the flag (mc_sample_rows / mc_ctx_set_condition_rows work on single rows)
inline void hist_set(mc_ctx* c, bool valid) { c->hist_valid = valid; c->hist_rows.assign((size_t)c->B, valid ? 1 : 0); }
inline float* deferred_a(const mc_ctx* c) { return c->a_tail ? c->a_tail : c->a; }      // where the deferred last FiLM block's fp32 rows live
bool a_holds_planes(const mc_ctx* c);
int denoise_impl(mc_ctx* c, const float* x_t, int32_t step, float* out2_dev, int32_t stop_after, void* stream, const SeedArgs* seed);
SamplerCoefs to_coefs(const mc_step_coefs* k);

// x0 of a sampler step as denoise_combined leaves it: one array, or the two partial products of the folded tail (b != null), which the
// sampler kernels add.  In a SamplerForm:  out_text = x0.a, out_none = x0.second(), c = x0.coefs(k)
struct X0Parts {
    const float *a = nullptr, *b = nullptr;
    const float* second() const { return b ? b : a; }
    SamplerCoefs coefs(const mc_step_coefs* k) const {
        SamplerCoefs sc = to_coefs(k);
        sc.text_coef = 1.f; sc.none_coef = b ? 1.f : 0.f;      // x0 is already the CFG-combined prediction, or the sum of its two partial products
        return sc;
    }
};
int denoise_combined(mc_ctx* c, const float* x_t, int32_t step, const mc_step_coefs* k, void* stream, X0Parts* x0, const SeedArgs* seed = nullptr);
// the sampler update behind denoise_combined, its kernel picked by the step's mode (under capture: by the graph's table) -- sampler_update_k
// (modes 0 / 1; noise or rng) or sampler_multistep_k (mode 2; x0_hist must be allocated, the caller keeps the history-valid flag); with
// a seam table set (mc_ctx_set_seams) sampler_seam_k in every mode; in rows mode the row kernels, the edit kernels under an edit table,
// or sampler_seam_rows_k in every mode under a row seam table (mc_ctx_set_seam_rows), sampler_seam_edit_rows_k under both tables
// (mc_ctx_set_long_edits)
int sampler_update(mc_ctx* c, const float* x_t, const X0Parts& x0p, const mc_step_coefs* k, const float* noise, float* x_prev, float* x0,
                   hipStream_t s, const RngArgs* rng = nullptr, const PadOut* pad = nullptr);
#pragma GCC visibility pop
