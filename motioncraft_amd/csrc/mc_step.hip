// The per-step kernel schedule of the STMoGen denoiser: which kernel runs on which rows, on which stream and behind which event, from the
// pose encoder through the DecoderLayers to the CFG-combined decoder tail.  The entry points (mc_model.hip) call denoise_impl /
// denoise_combined; handles and workspace: mc_ctx.h; which helper answers which question of the schedule: DESIGN.md section 4, "The step schedule".
#include "mc_ctx.h"

// The fp16-MFMA kernels have no small-batch variants (128-row workgroups, no hidden / K split): up to this many residual
// rows (B=1 at 196 frames: 392) the fp32 small-batch kernels are faster and the reduced-precision modes run on them
// (B=1 50-step DDIM: 68.3 ms on the fp16 kernels, 57.3 ms on the fp32 ones; from B=2 the fp16 kernels win).
bool use_half(const mc_ctx* c) { return c->prec != MC_PREC_F32 && c->rows > c->opt.half_min_rows; }
// "does this launch run on the fp16 MFMA?": its weight's planes if use_half and they were built (the text MoE passes null), else null
static const HalfW* half_planes(const mc_ctx* c, const HalfW* hw) { return hw && hw->hi && use_half(c) ? hw : nullptr; }
static bool split3(const mc_ctx* c) { return c->prec == MC_PREC_F16X3; }      // the three-product hi / lo form

// twin layer: rows of the second CFG half whose routing equals their twin's are aliased, not recomputed ...
static bool twin_aliased(const mc_ctx* c, bool twin) { return twin && !c->no_alias; }
// ... and the kernels' argument for it, counted in tokens or in frames (the empty value when nothing is aliased)
static TwinAlias twin_alias(const mc_ctx* c, bool twin, bool tokens) {
    return twin_aliased(c, twin) ? TwinAlias{mc_route_split_flag_ptr(c->rb), (tokens ? c->N : c->rows) / 2} : TwinAlias();
}

// the routing tile map of slot group `group` (mc_route.hip) in an MlpArgs / GemmArgs; src_row / dst_row are not per group: the caller's
template <class Args>
static void set_tile_map(const mc_ctx* c, int group, Args& a) {
    const long to = (long)group * c->rb.max_tiles;
    a.tile_group = c->rb.tile_group + to; a.tile_row0 = c->rb.tile_row0 + to; a.tile_nrows = c->rb.tile_nrows + to;
    a.num_tiles = mc_route_num_tiles_ptr(c->rb, group);
}

// (tests) dbg_delay_us: hold stream `pos` (value > 0) or `neg` (< 0) for that many microseconds
static int dbg_hold(const mc_ctx* c, hipStream_t pos, hipStream_t neg) {
    const long us = c->opt.dbg_delay_us;
    return us == 0 ? MC_OK : mc_launch_spin((us > 0 ? us : -us) * 100, us > 0 ? pos : neg);
}

// c = nullptr: a context-free launch (mc_op_gemm) on the process options
int dense(const mc_ctx* c, const float* A, long lda, const float* W, long ldw, const float* bias, const float* R, long ldr,
          float* C, long ldc, long M, int N, int K, int act, hipStream_t s) {
    const McOptions* o = c ? &c->opt : mc_process_options();
    if (!o) return MC_ERR_ARG;
    GemmArgs g;
    mc_gemm_opts(*o, g);
    g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = bias; g.R = R; g.ldr = ldr;
    g.C = C; g.ldc = ldc; g.M = (int)M; g.N = N; g.K = K; g.act = act;
    if (M <= o->small_gemm_rows && act == ACT_NONE && K % 32 == 0 && lda % 4 == 0 && ldw % 4 == 0)
        return mc_launch_gemm_small(g, s);          // latency-bound sizes: 64 x 64 tiles (see gemm_small_k)
    return mc_launch_gemm(GM_PLAIN, g, 1, 0, s);
}

// C = A W^T + bias + R on the fp16 MFMA (reduced-precision mode); `hw` = the weight's fp16 planes
static int dense_h(const mc_ctx* c, const float* A, const HalfW& hw, const float* bias, const float* R, float* C, long M, int N, int K, hipStream_t s) {
    GemmHArgs g;
    g.A = A; g.lda = K; g.Wh = hw.hi; g.Wl = hw.lo; g.bias = bias; g.R = R; g.ldr = N; g.C = C; g.ldc = N; g.M = (int)M; g.N = N; g.K = K;
    return mc_launch_gemm_h(g, split3(c), s);
}

// Small batches: a [M x K] x [K x N] GEMM with fewer than ~128 output tiles leaves most of the 256 CUs idle while each
// tile walks the whole K serially.  Split K across workgroups (the grouped launch with column offsets as "group"
// strides), partial sums in `ws`, reduced in a fixed order: C = sum_s A[:, s] W[:, s]^T + bias + R.
static int dense_splitk(const mc_ctx* c, const float* A, const float* W, const float* bias, const float* R, float* C, long M, int N, int K,
                        float* ws, size_t ws_floats, hipStream_t s) {
    const int tiles = cdiv(M, 128) * cdiv(N, 128);
    int S = 1;
    // (up to two rounds of the 512 workgroup slots: measured better than stopping at one, B=4 -4.5 %)
    while (S < 8 && tiles * (S * 2) <= 1024 && K % (S * 2 * 32) == 0 && (size_t)(S * 2) * M * N <= ws_floats) S *= 2;
    if (S == 1) return dense(c, A, K, W, K, bias, R, N, C, N, M, N, K, ACT_NONE, s);
    GemmArgs g;
    mc_gemm_opts(c->opt, g);
    g.A = A; g.lda = K; g.a_gstride = K / S;          // split s reads columns [s K/S, (s+1) K/S) of A and of W
    g.W = W; g.ldw = K; g.w_gstride = K / S;
    g.C = ws; g.ldc = N; g.c_gstride = M * N;
    g.M = (int)M; g.N = N; g.K = K / S;
    int r = mc_launch_gemm(GM_PLAIN, g, S, 0, s);
    if (r != MC_OK) return r;
    return mc_launch_splitk_reduce(ws, S, M, N, bias, R, C, s);
}

// expert FFN over the slots of one slot group (mc_route.hip): y2[dst_row] = FC2(gelu(FC1(z[src_row]))); hw / hw2: the fp16 planes of
// FC1 / FC2 (null: the text MoE has none)
static int moe_experts(mc_ctx* c, const MoeW& w, const float* z, long Ntok, int group, hipStream_t s, const HalfW* hw, const HalfW* hw2) {
    const int E = c->m->cfg.num_experts, din = w.din, hid = 4 * w.din;
    const int max_tiles = cdiv(2 * Ntok, 128) + E;
    int r;
    if (chain_on(c, kChainMlp) && mc_mlp_supported(din, hid)) {
        // fused expert FFN: hidden activations stay on chip (mc_chain.hip)
        MlpArgs m;
        m.dma = chain_on(c, kChainMlpDma) ? 1 : 0;
        {   // top-2 slots of this slot group's source tokens (twins of base layer 0 have no slots of their own)
            const long nsrc = c->led_nsrc > 0 ? c->led_nsrc : Ntok, gs = c->led_gsplit;
            m.ledger_rows = 2 * ((gs <= 0 || gs >= nsrc) ? nsrc : (group == 0 ? gs : nsrc - gs));
        }
        m.X = z; m.ldx = din; m.W1 = w.fc1_w; m.b1 = w.fc1_b; m.W2t = w.fc2_wt; m.b2 = w.fc2_b;
        m.Y = c->y2; m.ldy = din; m.L = din; m.hidden = hid;
        set_tile_map(c, group, m);
        m.src_row = c->rb.src_row; m.dst_row = c->rb.dst_row;
        if (half_planes(c, hw) && half_planes(c, hw2))      // reduced-precision mode: the same fused MLP on the fp16 MFMA
            return mc_launch_mlp_h(MLP_EXPERT, m, *hw, *hw2, split3(c), 1, max_tiles, s);
        // small batches (a few dozen tiles, each walking all hidden chunks serially): split the hidden dimension 4 ways,
        // partial FC2 sums in hbuf, reduced in a fixed order (rows of dropped pairs stay unwritten garbage: never read)
        // how many ways: the launch is bound by the busiest CU (mc_cu_load) times the hidden chunks per workgroup; ~2 Ntok / 128
        // + E / 2 tiles are real.  4 ways except where 3 take a whole round off: B = 2 at 196 frames (620 -> 465 workgroups,
        // 3 -> 2 rounds: 80.5 -> 77.7 ms per 50-step DDIM; at B = 1 the tile count straddles 256 / 3 and 3 ways lose 2 %).
        int S = (int)c->opt.split_expert;          // (0: the model below)
        if (S <= 0) {
            const long tiles = 2 * Ntok / 128 + E / 2;
            auto load = [&](int ways) { return mc_cu_load(tiles * ways) * (double)cdiv(hid / 32, ways); };
            S = 4;
            if (hid / 32 >= 4 && load(3) < 0.92 * load(4) && tiles * 3 > 300) S = 3;     // (tiles * 3 <= 300: B = 1, see above)
        }
        if (z == c->z && c->rows <= c->opt.split_rows_expert && c->N <= c->opt.big_tokens && S > 1 && hid / 32 >= S &&      // (N <= big_tokens: the one-stream schedule, one user of hbuf)
            c->hbuf_floats >= (size_t)S * 2 * Ntok * din) {
            m.Y = c->hbuf; m.nsplit = S; m.y_sstride = 2 * Ntok * din;
            // B = 1 sizes (the estimated tile count straddles 256 / 3): 3 or 4 ways decided on the device from the real count
            const bool dyn = S == 4 && c->opt.split_expert == 0 && (2 * Ntok / 128 + E / 2) * 3 <= 300;
            m.dyn_split = dyn ? 1 : 0;
            if ((r = mc_launch_mlp(MLP_EXPERT, m, 1, max_tiles, s))) return r;
            return mc_launch_splitk_reduce(c->hbuf, S, 2 * Ntok, din, nullptr, nullptr, c->y2, s,
                                           dyn ? mc_route_num_tiles_ptr(c->rb, group) : nullptr);
        }
        return mc_launch_mlp(MLP_EXPERT, m, 1, max_tiles, s);
    }
    GemmArgs a;
    mc_gemm_opts(c->opt, a);
    a.A = z; a.lda = din; a.src_row = c->rb.src_row;
    a.W = w.fc1_w; a.ldw = din; a.w_gstride = (long)hid * din;
    a.bias = w.fc1_b; a.b_gstride = hid; a.act = ACT_GELU;
    a.C = c->hbuf; a.ldc = hid; a.N = hid; a.K = din;
    set_tile_map(c, group, a);
    if ((r = mc_launch_gemm(GM_EXP1, a, 1, max_tiles, s))) return r;
    GemmArgs b;
    mc_gemm_opts(c->opt, b);
    b.A = c->hbuf; b.lda = hid; b.W = w.fc2_wt; b.ldw = hid; b.w_gstride = (long)din * hid;
    b.bias = w.fc2_b; b.b_gstride = din; b.dst_row = c->rb.dst_row;
    b.C = c->y2; b.ldc = din; b.N = din; b.K = hid;
    set_tile_map(c, group, b);
    return mc_launch_gemm(GM_EXP2, b, 1, max_tiles, s);
}

// Post-score combine + GELU + MOE.proj of tokens [tok0, tok0 + ntok):  Y[tok][ldy] = gelu(sum_k comb_w[tok][k] y2[tok][k]) proj_w^T + proj_b.
// proj_chained: as a row-chain kernel (proj_chain_args: its arguments; layer_proj extends them to projqkv / pqbody), else the combine GEMM
static bool proj_chained(const mc_ctx* c, const MoeW& w) { return chain_on(c, kChainRowchain) && mc_mlp_supported(w.din, 32) && w.dout % 32 == 0; }
static RowChainArgs proj_chain_args(const mc_ctx* c, const MoeW& w, float* Y, long ldy, long tok0, long ntok, long twin_from, const TwinAlias& alias) {
    RowChainArgs p;
    p.split_tokens = c->opt.rowchain_split;
    p.X = c->y2; p.comb_w = c->rb.comb_w; p.W = w.proj_w; p.bias = w.proj_b;
    p.Y = Y; p.ldy = ldy; p.tok0 = tok0; p.N = tok0 + ntok; p.L = w.din; p.Nout = w.dout;
    p.twin_from = twin_from;
    p.alias = alias;
    return p;
}
static int moe_proj(const mc_ctx* c, const MoeW& w, float* Y, long ldy, long tok0, long ntok, long twin_from, const TwinAlias& alias, hipStream_t s) {
    if (proj_chained(c, w)) return mc_launch_rowchain(0, proj_chain_args(c, w, Y, ldy, tok0, ntok, twin_from, alias), s);
    GemmArgs p;
    mc_gemm_opts(c->opt, p);
    p.A = c->y2 + 2 * tok0 * w.din; p.lda = w.din; p.comb_w = c->rb.comb_w + 2 * tok0;
    p.W = w.proj_w; p.ldw = w.din; p.bias = w.proj_b;
    p.C = Y + tok0 * ldy; p.ldc = ldy; p.M = (int)ntok; p.N = w.dout; p.K = w.din;
    return mc_launch_gemm(GM_COMB, p, 1, 0, s);
}

// the ONE place a capacity is computed: tutel extract_critical with the context's factor (the model's unless mc_ctx_set_capacity_factor
// changed it); factor 0 = no pair is dropped, which the routing takes as "no selection at all" (MC_ROUTE_KEEP_ALL)
static int moe_capacity(const mc_ctx* c, long Ntok) {
    const mc_model_config& g = c->m->cfg;
    const int E = g.num_experts;
    if (c->keep_all) return MC_ROUTE_KEEP_ALL;
    return g.topk * (int)((double)c->cap_factor * (double)((Ntok + E - 1) / E));
}

// One tutel MoE layer + GELU + proj (class MOE, st_attention.py:49-56) over Ntok tokens whose
// gate/expert input `z` ([Ntok, din], embedding already added) is in HBM.
// `gated`: idx/gate/key/counts were already produced (fused gate_k); otherwise run projector + gate finish here.
// `gsplit` < Ntok: two slot groups; then only the routing runs here and the caller launches moe_experts per group.
int run_moe(mc_ctx* c, const MoeW& w, const float* z, long Ntok, float* out, long ldout, bool gated, bool twin, long gsplit,
            hipStream_t s, const HalfW* hw, const HalfW* hw2) {
    const mc_model_config& g = c->m->cfg;
    const int E = g.num_experts, din = w.din;
    int r;
    if (!gated) {
        // cosine projector (tutel/gates/cosine_top.py): proj = z Wp^T + bp
        if ((r = dense(c, z, din, w.gate_w, din, w.gate_b, nullptr, 0, c->proj, 256, Ntok, 256, din, ACT_NONE, s))) return r;
        if ((r = mc_launch_gate_finish(c->proj, w.sim_n, w.scale, Ntok, E, c->rb, s))) return r;
    }
    const int capacity = moe_capacity(c, Ntok);
    c->cnt_clean = false;
    c->early_clean = false;      // (the fill of this routing uses the cursors)
    c->led_nsrc = twin ? Ntok / 2 : Ntok;
    c->led_gsplit = gsplit;
    if ((r = mc_launch_route(Ntok, twin ? Ntok / 2 : Ntok, gsplit, E, capacity, c->rb, c->opt, s))) return r;
    c->cnt_clean = mc_route_cleans_counts(c->opt, Ntok);
    if (gsplit < Ntok) return MC_OK;
    if ((r = moe_experts(c, w, z, Ntok, 0, s, hw, hw2))) return r;
    if (!out) return MC_OK;                        // the caller launches the projection itself (row ranges)
    return moe_proj(c, w, out, ldout, 0, Ntok, twin ? Ntok / 2 : 0, TwinAlias(), s);
}

// ONE answer per context to "does `a` hold fp16 hi | lo planes instead of fp32 rows?" -- asked by film_block (which writes them) and by
// mc_ctx_get_buffer("a") (which must not hand planes out as fp32 rows): reduced-precision context, chain bit 17, the plane launcher's
// shape preconditions (N % 128, K % 64 via D % 128; 32-bit byte offsets into a plane).  Every per-step FiLM weight of a reduced-precision
// context has planes (mc_ctx_set_precision builds them for all layers or fails), so the weight is not part of the answer.
bool a_holds_planes(const mc_ctx* c) {
    const long D = (long)c->m->cfg.latent_dim * c->m->cfg.num_parts;
    return use_half(c) && chain_on(c, kChainFilmPlanes) && D % 128 == 0 && c->rows * D * 2 < (1L << 31);
}

// rows [row0, row0 + nrows) of:  a = silu(LN(y1 (+ y2)) * (1 + scale) + shift);  h += Linear(a)   (StylizationBlock)
static int film_block(mc_ctx* c, float* hs, const float* y1, const float* y2, const float* ln_g, const float* ln_b,
               const float* ss, const float* out_w, const float* out_b, long row0, long nrows, hipStream_t s,
               bool prologue_only = false, TwinAlias y1_alias = TwinAlias(), const HalfW* hw = nullptr, int y1_parts = 1,
               hipEvent_t ev_after_rows = nullptr) {
    // ev_after_rows: recorded on s behind the row kernel (the other sample group's FiLM block may be ordered behind it: run_layer)
    // y1_parts > 1: y1 = that many partial planes of [nrows][D] starting AT y1 (rows relative to row0), summed by the row kernel
    const int D = c->m->cfg.latent_dim * c->m->cfg.num_parts;
    const long o = row0 * D;
    int r;
    StepRef sref;
    if (c->graph_mode) { sref.ptr = c->gstep; sref.stride = 2L * D; }     // `ss` then is the table's row of step 0
    // reduced-precision contexts: `a` is consumed by the fp16-MFMA GEMM only -> written as fp16 planes (hi [rows][D] | lo) into the same
    // buffer: the rows of this range start at halves offset o, the lo plane sits rows * D halves behind the hi plane
    const bool half_gemm = !prologue_only && half_planes(c, hw);
    // (the plane path's launcher needs N % 128 == 0, K % 64 == 0 and 32-bit byte offsets into a plane: anything else stays on dense_h)
    const bool planes = half_gemm && a_holds_planes(c);      // (one answer per context: plane rows and fp32 rows never share `a`)
    const long pstride = c->rows * D;
    float* a_rows = prologue_only ? deferred_a(c) : c->a;
    float* a_out = planes ? reinterpret_cast<float*>(reinterpret_cast<mc_half*>(c->a) + o) : a_rows + o;
    // chain bit 29 (round 6): the planes of THIS launch's rows are written fragment-major and the GEMM reads its A fragments straight into registers
    // (gemm_hf_k); needs whole 32-row blocks (a sample group of B x 196 frames with B % 8 == 0 has them), else the row-major planes + gemm_hd_k
    const bool frag_major = planes && chain_on(c, kChainFragMajor) && row0 % 32 == 0 && nrows % 32 == 0 && D % 64 == 0 && D >= 192;
    if ((r = mc_launch_film_rows(y1_parts > 1 ? y1 : y1 + o, y2 ? y2 + o : nullptr, ln_g, ln_b, ss, a_out, nrows, D, s, y1_alias, row0, sref,
                                 y1_parts, nrows * D, planes ? ((split3(c) ? 2 : 1) | (frag_major ? 4 : 0)) : 0, pstride,
                                 c->rows_mode ? &c->rowtab : nullptr))) return r;      // (rows mode: `ss` is the table's row of index 0, every row adds its own)
    if (ev_after_rows) MC_HIP(hipEventRecord(ev_after_rows, s));
    if (prologue_only) return MC_OK;
    // h = h + Linear(a)          (st_attention.py:172 / stmogen.py:606)
    if (planes) {
        GemmHArgs g;
        g.Ah = reinterpret_cast<mc_half*>(c->a) + o; g.Al = g.Ah + pstride;
        g.Wh = hw->hi; g.Wl = hw->lo; g.bias = out_b; g.R = hs + o; g.ldr = D; g.C = hs + o; g.ldc = D;
        g.M = (int)nrows; g.N = D; g.K = D;
        g.a_fm = frag_major ? 1 : 0;
        g.pre = chain_on(c, kChainResidualPre);      // residual rows prefetched into registers (same bits)
        return mc_launch_gemm_h(g, split3(c), s);
    }
    if (half_gemm)
        return dense_h(c, c->a + o, *hw, out_b, hs + o, hs + o, nrows, D, D, s);
    if (nrows <= c->opt.small_gemm_rows && D % 64 == 0) {     // up to a few thousand rows: 64 x 64 tiles, short MFMA chains, no K split (B=8: -11 % per step)
        GemmArgs q;
        mc_gemm_opts(c->opt, q);
        q.A = c->a + o; q.lda = D; q.W = out_w; q.ldw = D; q.bias = out_b; q.R = hs + o; q.ldr = D; q.C = hs + o; q.ldc = D;
        q.M = (int)nrows; q.N = D; q.K = D;
        return mc_launch_gemm_small(q, s);
    }
    if (nrows <= 2048 && c->hbuf_floats)       // few output tiles: split K (hbuf is free scratch on the fused path)
        return dense_splitk(c, c->a + o, out_w, out_b, hs + o, hs + o, nrows, D, D, c->hbuf, c->hbuf_floats, s);
    if (!c->prof_on) return dense(c, c->a + o, D, out_w, D, out_b, hs + o, D, hs + o, D, nrows, D, D, ACT_NONE, s);
    // mc_ctx_profile: HIP events around this launch ON THE STREAM IT IS LAUNCHED ON (the sample group's stream)
    ProfRec pr;
    pr.rows = nrows;
    if (hipEventCreate(&pr.e0) != hipSuccess || hipEventCreate(&pr.e1) != hipSuccess) { mc_set_error("hipEventCreate failed"); return MC_ERR_HIP; }
    MC_HIP(hipEventRecord(pr.e0, s));
    r = dense(c, c->a + o, D, out_w, D, out_b, hs + o, D, hs + o, D, nrows, D, D, ACT_NONE, s);
    MC_HIP(hipEventRecord(pr.e1, s));
    c->prof.push_back(pr);
    return r;
}

// Everything of a DecoderLayer AFTER the expert MLP, restricted to residual-stream rows [row0, row0 + nrows) (whole samples), in four
// pieces: layer_proj, layer_body, layer_temporal and layer_rows_tail (proj_out FiLM block, SFFN, its FiLM block).  Every kernel here is
// row-independent, so disjoint row ranges can run on different streams.  layer_rows runs the first three for one range; the twin layer
// of the large-batch schedule calls them one by one (the front per sample sub-group, the temporal attention per CFG half: run_layer).
//
// large batches: proj + body LayerNorm + q/k/v as one kernel (small ones keep them apart: the temporal branch then starts on the side
// stream right after the projection) ...
static bool pq_fused(const mc_ctx* c) {
    const int L = c->m->cfg.latent_dim;
    return chain_on(c, kChainRowchain) && c->N > c->opt.big_tokens && mc_mlp_supported(L, 32) && (4 * L) % 32 == 0;
}
// ... and the body-topology attention too (pqbody_k: frame-aligned tiles, q/k/v never leave the chip): L = 128 / 64, 12 parts
static bool body_fused(const mc_ctx* c) {
    const mc_model_config& g = c->m->cfg;
    return pq_fused(c) && chain_on(c, kChainPqBody) && g.num_parts == 12 && g.dyn_heads == 8 && (g.latent_dim == 128 || g.latent_dim == 64);
}

// ---- post-score combine + GELU + MOE.proj -> mf [N][4L] (+ q/k/v when pq_fused, + ys when body_fused) ----
static int layer_proj(mc_ctx* c, int i, bool twin, long row0, long nrows, hipStream_t s) {
    const int L = c->m->cfg.latent_dim, H = c->m->cfg.num_parts;
    const LayerW& w = c->lw[i];
    const long tok0 = row0 * H, ntok = nrows * H, twin_from = twin ? c->N / 2 : 0;
    if (!pq_fused(c)) return moe_proj(c, w.mm, c->mf, 4 * L, tok0, ntok, twin_from, twin_alias(c, twin, true), s);
    // + the dynamic body topology's shared LayerNorm and q/k/v on the body_value columns   (pq_fused implies proj_chained)
    RowChainArgs p = proj_chain_args(c, w.mm, c->mf, 4 * L, tok0, ntok, twin_from, twin_alias(c, twin, true));
    p.gamma = w.dyn_g; p.beta = w.dyn_b; p.W2 = w.qkv_w; p.bias2 = w.qkv_b; p.Y2 = c->qkv; p.ldy2 = 3 * L;
    p.pad_row = c->N;      // mf / qkv carry 128 padding rows (mc_ctx_create): projqkv_k's stores are unconditional
    const HalfW *hp = half_planes(c, &w.h_proj), *hq = half_planes(c, &w.h_qkv);
    if (!body_fused(c)) return hp && hq ? mc_launch_projqkv_h(p, *hp, *hq, split3(c), s) : mc_launch_projqkv(p, s);
    p.wsm = w.wsm; p.ys = c->ys;
    return hp && hq ? mc_launch_pqbody_h(p, H, *hp, *hq, split3(c), s) : mc_launch_pqbody(p, H, s);
}

// ---- dynamic body topology: shared LayerNorm + q/k/v (unless layer_proj produced them), then the body attention (unless it did that too) ----
static int layer_body(mc_ctx* c, int i, bool twin, long row0, long nrows, hipStream_t sb) {
    const mc_model_config& g = c->m->cfg;
    const int L = g.latent_dim, H = g.num_parts, D = L * H;
    const LayerW& w = c->lw[i];
    const long tok0 = row0 * H, ntok = nrows * H;
    int r;
    if (pq_fused(c)) {
        // q/k/v were produced by projqkv_k
    } else if (chain_on(c, kChainRowchain) && mc_mlp_supported(L, 32)) {
        RowChainArgs q;
        q.split_tokens = c->opt.rowchain_split;
        q.X = c->mf; q.ldx = 4 * L; q.gamma = w.dyn_g; q.beta = w.dyn_b; q.W = w.qkv_w; q.bias = w.qkv_b;
        q.Y = c->qkv; q.ldy = 3 * L; q.tok0 = tok0; q.N = tok0 + ntok; q.L = L; q.Nout = 3 * L;
        q.alias = twin_alias(c, twin, true);
        if ((r = mc_launch_rowchain(1, q, sb))) return r;
    } else {
        if ((r = mc_launch_ln_rows(c->mf + tok0 * 4 * L, 4 * L, 0, w.dyn_g, w.dyn_b, nullptr, 1, c->z + tok0 * L, L, ntok, L, sb))) return r;
        if ((r = dense(c, c->z + tok0 * L, L, w.qkv_w, L, w.qkv_b, nullptr, 0, c->qkv + tok0 * 3 * L, 3 * L, ntok, 3 * L, L, ACT_NONE, sb))) return r;
    }
    if (body_fused(c)) return MC_OK;
    return mc_launch_body(c->mf + tok0 * 4 * L, 4 * L, c->qkv + tok0 * 3 * L, w.wsm, c->ys + row0 * D, nrows, H, L, g.dyn_heads, sb,
                          twin_alias(c, twin, false), row0);
}

// ---- temporal linear attention: needs only mf ----
static int layer_temporal(mc_ctx* c, int i, bool twin, long row0, long nrows, hipStream_t stt) {
    const mc_model_config& g = c->m->cfg;
    const int L = g.latent_dim, H = g.num_parts;
    const float* tfl = c->tf + (long)i * c->Ntxt * 2 * L;
    const int* twin_flag = twin_alias(c, twin, true).split_flag;
    const int tnb = (int)(nrows / c->T);
    if (use_half(c) && chain_on(c, kChainTemporalHalf) && (L == 128 || L == 64) && (long)tnb * H > c->opt.temporal_split)
        // reduced-precision mode: both contractions on the fp16 MFMA (whole-(sample, part) workgroups; the sliced small-batch form stays fp32)
        return mc_launch_temporal_h(c->mf, tfl, c->mask, c->yt, (int)(row0 / c->T), tnb, c->B, c->T, g.max_text_len, H, L,
                                    split3(c), stt, twin_flag, chain_on(c, kChainSkipText));
    return mc_launch_temporal(c->mf, tfl, c->mask, c->yt, (int)(row0 / c->T), tnb, c->B, c->T,
                              g.max_text_len, H, L, stt, twin_flag, c->opt.temporal_split, chain_on(c, kChainTemporalPair), chain_on(c, kChainSkipText));
}

// The three of them for one row range: the projection on `s`, then the body branch and the temporal branch -- beside each other when
// `st` is a second stream (small batches), else inline on `s`.
static int layer_rows(mc_ctx* c, int i, bool twin, long row0, long nrows, hipStream_t s, hipStream_t st) {
    int r;
    if ((r = layer_proj(c, i, twin, row0, nrows, s))) return r;
    // small batches: the longer branch (temporal) stays on `s`, LN + q/k/v + body go to the side stream -- the fork latency is
    // then paid by the short branch and the join event has fired long before `s` reaches it (B=1: -13 us per layer vs the
    // temporal branch on the side stream)
    hipStream_t sb = s, stt = s;         // streams of the body branch and of the temporal branch
    if (st != s) {
        MC_HIP(hipEventRecord(c->ev_fork, s));
        MC_HIP(hipStreamWaitEvent(st, c->ev_fork, 0));
        if (c->rows <= 1200) sb = st; else stt = st;      // (B <= 3 at 196 frames: -1.5 .. -3 %; B = 4: +1 %)
        if ((r = dbg_hold(c, st, s))) return r;        // (tests) hold the side stream (> 0) or the main stream (< 0) behind the fork
    }
    if ((r = layer_body(c, i, twin, row0, nrows, sb))) return r;
    if (sb != s) MC_HIP(hipEventRecord(c->ev_join, sb));
    if ((r = layer_temporal(c, i, twin, row0, nrows, stt))) return r;
    if (stt != s) MC_HIP(hipEventRecord(c->ev_join, stt));
    if (st != s) MC_HIP(hipStreamWaitEvent(s, c->ev_join, 0));
    return MC_OK;
}

static int layer_rows_tail(mc_ctx* c, int i, float* hs, int step, bool twin, long row0, long nrows, hipStream_t s, hipEvent_t ev_rows = nullptr,
                           hipEvent_t wait_first = nullptr) {
    // ev_rows: recorded behind the first FiLM block's row kernel; wait_first: this range's tail starts behind that event of the other group
    if (wait_first) MC_HIP(hipStreamWaitEvent(s, wait_first, 0));
    const mc_model_config& g = c->m->cfg;
    const int L = g.latent_dim, H = g.num_parts, D = L * H, F = g.ffn_dim;
    const LayerW& w = c->lw[i];
    int r;
    const float* ss0 = c->ss + ((long)(i * 2 + 0) * c->maxS + step) * 2 * D;
    if ((r = film_block(c, hs, c->ys, c->yt, w.ca_ln_g, w.ca_ln_b, ss0, w.ca_out_w, w.ca_out_b, row0, nrows, s, false, twin_alias(c, twin, false), &w.h_ca_out, 1,
                        ev_rows))) return r;
    // ---- SFFN (stmogen.py:596-607): 12 part-wise FFNs as grouped GEMMs ----
    const long o = row0 * D;
    int z2_parts = 1;
    if (chain_on(c, kChainMlp) && mc_mlp_supported(L, F)) {
        MlpArgs m;
        m.dma = chain_on(c, kChainMlpDma) ? 1 : 0;
        m.X = hs + o; m.ldx = D; m.x_gstride = L;
        m.W1 = w.ffn_w1; m.b1 = w.ffn_b1; m.W2t = w.ffn_w2; m.b2 = w.ffn_b2;
        m.Y = c->z2 + o; m.ldy = D; m.y_gstride = L; m.M = (int)nrows; m.L = L; m.hidden = F;
        // hidden split of the part-wise FFNs (partial sums folded into the FiLM row kernel): ways by the load of the busiest CU
        // (mc_cu_load) plus ~2 chunk times of fixed cost per workgroup -- 4 ways up to B = 5 (and at B = 8: 184.5 -> 178.0 ms
        // per 50-step DDIM), 2 at B = 6 and B = 16 (293.7 -> 287.5), none at B = 12 or beyond 8192 rows
        int S = (int)c->opt.split_sffn;            // (0: the model below)
        if (S <= 0) {
            S = 1;
            if (nrows <= c->opt.split_rows_sffn && nrows == c->rows) {      // (one launch over the whole batch: the partial planes live in the one hbuf -- not in the two-stream schedule)
                auto load = [&](int ways) { return mc_cu_load((long)cdiv(nrows, 128) * H * ways) * ((double)cdiv(F / 32, ways) + 2.0); };
                double best = load(1);
                for (int ways = 2; ways <= 4; ways *= 2)
                    if (F / 32 >= ways && load(ways) <= 1.03 * best) { S = ways; best = load(ways) < best ? load(ways) : best; }
            }
        }
        if (half_planes(c, &w.h_w1) && half_planes(c, &w.h_w2)) {
            if ((r = mc_launch_mlp_h(MLP_PARTS, m, w.h_w1, w.h_w2, split3(c), H, 0, s))) return r;
        } else if (nrows <= c->opt.split_rows_sffn && nrows == c->rows && S > 1 && F / 32 >= S && c->hbuf_floats >= (size_t)S * nrows * D) {     // small batches: see moe_experts
            m.Y = c->hbuf; m.nsplit = S; m.y_sstride = nrows * D;
            if ((r = mc_launch_mlp(MLP_PARTS, m, H, 0, s))) return r;
            z2_parts = S;          // the FiLM row kernel adds the partial planes up itself
        } else if ((r = mc_launch_mlp(MLP_PARTS, m, H, 0, s))) return r;
    } else {
        GemmArgs f1;
        mc_gemm_opts(c->opt, f1);
        f1.A = hs + o; f1.lda = D; f1.a_gstride = L;
        f1.W = w.ffn_w1; f1.ldw = L; f1.w_gstride = (long)F * L;
        f1.bias = w.ffn_b1; f1.b_gstride = F; f1.act = ACT_GELU;
        f1.C = c->fh + row0 * H * F; f1.ldc = (long)H * F; f1.c_gstride = F;
        f1.M = (int)nrows; f1.N = F; f1.K = L;
        if ((r = mc_launch_gemm(GM_PLAIN, f1, H, 0, s))) return r;
        GemmArgs f2;
        mc_gemm_opts(c->opt, f2);
        f2.A = c->fh + row0 * H * F; f2.lda = (long)H * F; f2.a_gstride = F;
        f2.W = w.ffn_w2; f2.ldw = F; f2.w_gstride = (long)L * F;
        f2.bias = w.ffn_b2; f2.b_gstride = L;
        f2.C = c->z2 + o; f2.ldc = D; f2.c_gstride = L;
        f2.M = (int)nrows; f2.N = L; f2.K = F;
        if ((r = mc_launch_gemm(GM_PLAIN, f2, H, 0, s))) return r;
    }
    const float* ss1 = c->ss + ((long)(i * 2 + 1) * c->maxS + step) * 2 * D;
    return film_block(c, hs, z2_parts > 1 ? c->hbuf : c->z2, nullptr, w.ffn_ln_g, w.ffn_ln_b, ss1, w.ffn_out_w, w.ffn_out_b, row0, nrows, s,
                      c->defer_last_gemm && i == g.num_layers - 1, TwinAlias(), &w.h_ffn_out, z2_parts);
}

// Pick the side stream that runs BESIDE the caller's stream `s` (see mc_ctx::side_cand): a 60 us spin kernel on `s` and one on the candidate, started
// together -- ~65 us when the two streams sit on different hardware queues, ~125 us when they share one.  Once per (context, caller stream); host-synchronous
// (~0.5 ms), so never inside a stream capture (a captured step keeps the stream picked by the eager calls before it).  MC_SIDE_PROBE=0 switches it off.
static int pick_side_stream(mc_ctx* c, hipStream_t s) {
    if (c->side_picked && c->side_for == s) return MC_OK;
    static const bool enabled = [] { const char* e = getenv("MC_SIDE_PROBE"); return !e || atoi(e) != 0; }();
    if (!enabled || c->graph_mode || c->graph_exec) return MC_OK;
    for (int k = 0; k < c->side_memo_n; ++k)
        if (c->side_memo_for[k] == s) {          // answered before for this caller stream: switch without a probe (the previous call joined its side work)
            c->side = c->side_cand[c->side_memo_pick[k]];
            c->side_for = s;
            return MC_OK;
        }
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess || st != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return MC_OK; }
    hipEvent_t e0 = nullptr, e1 = nullptr, eq = nullptr;
    MC_HIP(hipEventCreate(&e0));
    MC_HIP(hipEventCreate(&e1));
    MC_HIP(hipEventCreateWithFlags(&eq, hipEventDisableTiming));
    int best = 0, r = MC_OK;
    float best_ms = 1e30f;
    for (int rep = 0; rep < 2 && r == MC_OK; ++rep)           // (the first round also pays the candidates' first-use cost: the second one decides)
        for (int k = 0; k < mc_ctx::SIDE_CAND && r == MC_OK; ++k) {
            hipStream_t q = c->side_cand[k];
            bool ok = hipEventRecord(e0, s) == hipSuccess && hipStreamWaitEvent(q, e0, 0) == hipSuccess;
            ok = ok && mc_launch_spin(6000, s) == MC_OK && mc_launch_spin(6000, q) == MC_OK;
            ok = ok && hipEventRecord(eq, q) == hipSuccess && hipStreamWaitEvent(s, eq, 0) == hipSuccess && hipEventRecord(e1, s) == hipSuccess &&
                 hipEventSynchronize(e1) == hipSuccess;
            float ms = 0.f;
            ok = ok && hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
            if (!ok) { mc_set_error("side-stream probe failed: %s", hipGetErrorString(hipGetLastError())); r = MC_ERR_HIP; break; }
            if (rep == 1) {
                c->side_probe_ms[k] = ms;
                if (ms < best_ms - 0.02f) { best_ms = ms; best = k; }      // (20 us margin: near ties keep the earlier candidate)
            }
        }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipEventDestroy(eq);
    if (r != MC_OK) return r;
    c->side = c->side_cand[best];
    c->side_for = s;
    c->side_picked = true;
    {
        const int slot = c->side_memo_n < mc_ctx::SIDE_MEMO ? c->side_memo_n++ : 0;      // (more than SIDE_MEMO caller streams: the oldest answer is re-probed)
        c->side_memo_for[slot] = s;
        c->side_memo_pick[slot] = best;
    }
    if (getenv("MC_SIDE_PROBE_VERBOSE"))
        fprintf(stderr, "[motioncraft_amd] side stream for caller stream %p: candidate %d (spin pair %.0f %.0f %.0f %.0f us)\n", (void*)s, best,
                c->side_probe_ms[0] * 1e3f, c->side_probe_ms[1] * 1e3f, c->side_probe_ms[2] * 1e3f, c->side_probe_ms[3] * 1e3f);
    return MC_OK;
}

// The two sample groups of the large-batch schedule are the CFG halves: group 0 = rows [0, B T) on the caller's stream, group 1 =
// rows [B T, 2 B T) on the side stream.  side_fork / side_join: the side stream starts behind / the caller's stream waits for the other.
static int side_fork(mc_ctx* c, hipStream_t s) {
    MC_HIP(hipEventRecord(c->ev_fork, s));
    MC_HIP(hipStreamWaitEvent(c->side, c->ev_fork, 0));
    return MC_OK;
}
static int side_join(mc_ctx* c, hipStream_t s) {
    MC_HIP(hipEventRecord(c->ev_side, c->side));
    MC_HIP(hipStreamWaitEvent(s, c->ev_side, 0));
    return MC_OK;
}

// The schedule of one DecoderLayer has two shapes: one stream, or the two sample groups on two streams (`two_groups`, decided once per call
// by denoise_impl; the groups stay apart across layers and only meet where tokens of the whole batch are ranked against each other).
// Its decisions, taken once per layer and read by the phases of run_layer:
struct LayerPlan {
    bool two_groups, fused_gate, twin, twin_split, early, stagger;
    long half, sub_rows;   // rows of one CFG half (= one sample group); rows of the twin layer's first sub-group (whole samples)
    long nsrc, gsplit;     // routed source tokens; slot group 0 = tokens [0, gsplit), group 1 = [gsplit, nsrc)  (gsplit = N: one slot group)
};
static LayerPlan layer_plan(const mc_ctx* c, bool twin_ok, bool two_groups) {
    const int L = c->m->cfg.latent_dim, H = c->m->cfg.num_parts;
    LayerPlan p;
    p.two_groups = two_groups;
    // gate_k (two_groups implies it); else ln_rows and, inside run_moe, the projector GEMM + gate finish
    p.fused_gate = chain_on(c, kChainGate) && mc_mlp_supported(L, 32);
    // The two CFG halves enter base layer 0 with the same residual stream (the pose encoder output is written to both,
    // stmogen.py:736-740), so gate scores and expert outputs of token i + N/2 equal those of token i: gate and experts run on the
    // first half only, routing still ranks all N tokens ("twin" mode, mc_route.hip).
    p.twin = twin_ok && p.fused_gate && chain_on(c, kChainRowchain) && c->N % 2 == 0 &&
             c->rb.tie_xor == 0xFFFFFFFFu;   // (the dedupe relies on a twin ranking right behind its original: stable tie order)
    p.half = (long)c->B * c->T; p.sub_rows = ((long)c->B / 2) * c->T;
    // Twin layer of the two-group schedule: gate, experts and the front kernels exist for the FIRST CFG half only (the second one aliases
    // it), so the half is cut into two sample sub-groups that go down the two streams (otherwise one stream idles for the first ~1.75 ms
    // of every step at B=64); the streams cross-join behind the front (the temporal kernel of either CFG half reads mf rows of the whole
    // first half) and continue per CFG half as in every other layer.
    p.twin_split = p.twin && two_groups && chain_on(c, kChainTwinSplit) && !c->no_alias && p.sub_rows > 0;
    // option route_early: each group's experts start behind its own gate (moe_front, form c); the one-workgroup routing sizes stay joined
    p.early = p.fused_gate && two_groups && c->opt.route_early != 0 && !mc_route_is_small(c->opt, c->N);
    // the second group's first FiLM block starts behind the first group's FiLM row kernel (measured per shape, same-box A/B: helps the exact-fp32
    // L = 128 step; the fp16 modes lose 0.1 - 0.2 ms and the L = 64 models (M2D) 0.35 ms with it, batch 32 is neutral: applied where it helps)
    p.stagger = two_groups && chain_on(c, kChainStagger) && !use_half(c) && L == 128;
    p.nsrc = p.twin ? c->N / 2 : c->N;
    p.gsplit = p.twin_split ? p.sub_rows * H : two_groups ? p.half * H : c->N;
    return p;
}

// (tests) cap_idx: the routing's expert ids and combine weights of layer `i`, copied on `s` behind the routing
static int capture_routing(mc_ctx* c, int i, bool twin, hipStream_t s) {
    if (!c->cap_idx) return MC_OK;
    int* const ids = c->cap_idx + (long)i * 2 * c->N;      // (twin: expert ids exist for the first half only, the twins have the same ones)
    MC_HIP(hipMemcpyAsync(ids, c->rb.idx, sizeof(int) * (twin ? 1 : 2) * c->N, hipMemcpyDeviceToDevice, s));
    if (twin) MC_HIP(hipMemcpyAsync(ids + c->N, c->rb.idx, sizeof(int) * c->N, hipMemcpyDeviceToDevice, s));
    MC_HIP(hipMemcpyAsync(c->cap_w + (long)i * 2 * c->N, c->rb.comb_w, sizeof(float) * 2 * c->N, hipMemcpyDeviceToDevice, s));
    return MC_OK;
}

// Phase 1 of a layer, the MoE front: gate + routing + experts (the only part that couples tokens across the batch), up to "the expert rows
// are in flight".  ON RETURN every stream that will run row kernels is ordered behind the selection results (comb_w, the twin-split flag)
// and behind the expert rows its first row kernel reads; with two groups the side stream is forked.  Each form also leaves the next routing
// what it relies on (cnt_clean, early_clean, led_nsrc, led_gsplit): forms a and b through run_moe, form c in its own block.
static int moe_front(mc_ctx* c, int i, float* hs, const LayerPlan& p, hipStream_t s) {
    const mc_model_config& g = c->m->cfg;
    const int L = g.latent_dim, H = g.num_parts, E = g.num_experts;
    const LayerW& w = c->lw[i];
    int r;
    GateArgs ga;
    ga.X = hs; ga.ldx = L; ga.gamma = w.norm_g; ga.beta = w.norm_b; ga.emb = w.mm.emb; ga.emb_mod = c->T * H;
    ga.Z = c->z; ga.Wp = w.mm.gate_w; ga.bp = w.mm.gate_b; ga.sim_nT = w.mm.sim_nT; ga.logit_scale = w.mm.scale;
    ga.E = E; ga.L = L; ga.small_tokens = c->opt.gate_small;
    ga.idx = c->rb.idx; ga.gate = c->rb.gate; ga.key = c->rb.key; ga.cnt = c->rb.state;
    auto gate_whole = [&]() {      // one launch over all source tokens on `s`
        ga.N = p.nsrc;
        ga.zero_cnt = c->cnt_clean ? 0 : 1;      // small batches: the previous layer's routing kernel left the counts zeroed
        c->cnt_clean = false;
        return mc_launch_gate(ga, s);
    };
    auto gate_group = [&](int group, hipStream_t sk, int* cnt) {      // group 0 = tokens [0, gsplit), group 1 = [gsplit, nsrc); the counts were zeroed
        ga.zero_cnt = 0; ga.cnt = cnt;
        ga.tok0 = group ? p.gsplit : 0; ga.N = group ? p.nsrc : p.gsplit;
        return mc_launch_gate(ga, sk);
    };
    auto experts = [&](int group, hipStream_t sk) { return moe_experts(c, w.mm, c->z, c->N, group, sk, &w.h_fc1, &w.h_fc2); };
    // two groups: do both streams carry a gate and an expert launch?  (else: the twin layer without its sub-group split -- one gate launch and
    // one slot group on `s`; group 1 combines group 0's expert rows, so the side stream forks behind them)
    const bool both = !p.twin || p.twin_split;

    // ---- (a) one stream: gate (or ln_rows + the unfused gate inside run_moe), routing, experts ----
    if (!p.two_groups) {
        if (p.fused_gate) { if ((r = gate_whole())) return r; }
        else if ((r = mc_launch_ln_rows(hs, L, 0, w.norm_g, w.norm_b, w.mm.emb, c->T * H, c->z, L, c->N, L, s))) return r;
        if ((r = run_moe(c, w.mm, c->z, c->N, nullptr, 0, p.fused_gate, p.twin, p.gsplit, s, &w.h_fc1, &w.h_fc2))) return r;
        return capture_routing(c, i, p.twin, s);
    }

    // ---- (b) two groups, joined: gate per group, join, routing (it ranks the whole batch: both groups must have arrived), fork, experts per group ----
    if (!p.early) {
        if (both) {
            if (!c->cnt_clean) MC_HIP(hipMemsetAsync(ga.cnt, 0, sizeof(int) * 32, s));
            c->cnt_clean = false;
            if ((r = side_fork(c, s))) return r;
            if ((r = gate_group(0, s, ga.cnt))) return r;
            if ((r = gate_group(1, c->side, ga.cnt))) return r;
        } else if ((r = gate_whole())) return r;
        if ((r = side_join(c, s))) return r;
        if ((r = run_moe(c, w.mm, c->z, c->N, nullptr, 0, true, p.twin, p.gsplit, s, &w.h_fc1, &w.h_fc2))) return r;      // (gsplit < N: the routing alone)
        if ((r = capture_routing(c, i, p.twin, s))) return r;
        if (both && (r = side_fork(c, s))) return r;
        if ((r = experts(0, s))) return r;
        return both ? experts(1, c->side) : side_fork(c, s);      // (one gate: group 1 combines group 0's expert rows, so it forks behind them)
    }

    // ---- (c) two groups, early ----
    // What couples the tokens of the batch is the capacity cut alone, and its results are first read by the projection BEHIND the expert MLP,
    // whose rows are independent of their slots.  So each group's experts start behind its own gate, over a slot plan of ALL the group's pairs
    // (mc_launch_route_fill_group), and the whole-batch selection runs beside them:
    //   s:     gate 0 -> fill 0 -> experts 0 -> wait(ev_gate1) -> selection -> ev_sel -> projection of group 0 ...
    //   side:  gate 1 -> fill 1 -> ev_gate1 -> experts 1 -> wait(ev_sel) -> projection of group 1 ...
    // (ev_gate1 sits behind fill 1, not in front of it: the selection hands the counts and cursors back zeroed, which fill 1 must have
    // read by then; the few microseconds of fill 1 are long over when experts 0 end.)
    // (Measured, B=64 fp32: the selection on the side stream in front of experts 1 instead -- so that it never runs alone -- gains 0.17 ms
    // per step where this order gains 0.29: profiles/route_early_ab.txt.)
    if (!(c->cnt_clean && c->early_clean) && (r = mc_route_early_reset(c->rb, s))) return r;
    c->cnt_clean = c->early_clean = false;
    c->led_nsrc = p.nsrc; c->led_gsplit = p.gsplit;
    if (both && (r = side_fork(c, s))) return r;
    if ((r = gate_group(0, s, mc_route_group_counts(c->rb, 0)))) return r;
    if ((r = mc_launch_route_fill_group(0, 0, p.gsplit, E, c->rb, s))) return r;
    if ((r = experts(0, s))) return r;
    if (both) {
        if ((r = gate_group(1, c->side, mc_route_group_counts(c->rb, 1)))) return r;
        if ((r = mc_launch_route_fill_group(1, p.gsplit, p.nsrc - p.gsplit, E, c->rb, c->side))) return r;
        MC_HIP(hipEventRecord(c->ev_gate1, c->side));
        if ((r = experts(1, c->side))) return r;
        MC_HIP(hipStreamWaitEvent(s, c->ev_gate1, 0));     // the cut ranks the whole batch: both gates must have arrived
    } else if ((r = mc_launch_route_fill_group(1, p.gsplit, 0, E, c->rb, s))) return r;      // (an empty second group: no tiles)
    if ((r = mc_launch_route(c->N, p.nsrc, p.gsplit, E, moe_capacity(c, c->N), c->rb, c->opt, s, true))) return r;
    c->cnt_clean = c->early_clean = true;
    MC_HIP(hipEventRecord(c->ev_sel, s));
    if (both) MC_HIP(hipStreamWaitEvent(c->side, c->ev_sel, 0));      // group 1's projection reads comb_w and the twin-split flag
    if ((r = capture_routing(c, i, p.twin, s))) return r;
    return both ? MC_OK : side_fork(c, s);
}

// The one hazard early routing adds to the row phase of a twin layer: group 1's front reads the FIRST half's expert rows, which the next
// layer's experts on the caller's stream overwrite with no join in front of them.  kFrontRead: recorded on the side stream behind that
// front; kFrontWait: the caller's stream waits for it.  (The joined form meets in front of the next routing: nothing is enqueued.)
enum { kFrontRead = 1, kFrontWait = 2 };
static int expert_rows_guard(mc_ctx* c, const LayerPlan& p, int what, hipStream_t s) {
    if (!(p.early && p.twin)) return MC_OK;
    if (what & kFrontRead) MC_HIP(hipEventRecord(c->ev_front, c->side));
    if (what & kFrontWait) MC_HIP(hipStreamWaitEvent(s, c->ev_front, 0));
    return MC_OK;
}

// One DecoderLayer (STMA + SFFN, stmogen.py:610-623) in place on the residual stream `hs` [rows, D];
// `i` selects the layer slot (weights, text K/V, FiLM tables): base layers first, control copies after.
static int run_layer(mc_ctx* c, int i, float* hs, int step, bool twin_ok, bool two_groups, hipStream_t s) {
    const LayerPlan p = layer_plan(c, twin_ok, two_groups);
    const bool twin = p.twin;
    const long half = p.half;
    int r;
    if ((r = moe_front(c, i, hs, p, s))) return r;
    // ---- phase 2: the row-independent rest of the layer ----
    if (!two_groups) {
        // Small batches: the temporal branch runs on the side stream beside LN + qkv + body (measured +2.4 % at B=8).
        const bool side_temporal = c->side && c->N <= c->opt.big_tokens;
        if ((r = layer_rows(c, i, twin, 0, 2 * half, s, side_temporal ? c->side : s))) return r;
        return layer_rows_tail(c, i, hs, step, twin, 0, 2 * half, s);
    }
    // Large batches: the two CFG halves go down two streams.  Each kernel of the chain fills 4.59 "waves" of
    // workgroups at B=64, so ~8 % of every launch is a tail on a partly idle chip; with two independent chains in
    // flight the next kernel of one half starts inside the tail of the other (same effect as two batches in flight).
    if (p.twin_split) {
        auto front = [&](long row0, long nrows, hipStream_t sk) {       // projection + body branch of a row range on one stream
            const int e = layer_proj(c, i, twin, row0, nrows, sk);
            return e ? e : layer_body(c, i, twin, row0, nrows, sk);
        };
        if ((r = front(0, p.sub_rows, s))) return r;
        if ((r = front(p.sub_rows, half - p.sub_rows, c->side))) return r;
        // cross-join: each stream waits for the other's front
        MC_HIP(hipEventRecord(c->ev_join, s));
        MC_HIP(hipEventRecord(c->ev_side, c->side));
        MC_HIP(hipStreamWaitEvent(c->side, c->ev_join, 0));
        MC_HIP(hipStreamWaitEvent(s, c->ev_side, 0));
        // the second CFG half's own front: exits at once while no twin pair was split by a capacity cut (the usual case)
        if ((r = front(half, half, c->side))) return r;
        if ((r = expert_rows_guard(c, p, kFrontRead, s))) return r;
        if ((r = layer_temporal(c, i, twin, 0, half, s))) return r;
        if ((r = expert_rows_guard(c, p, kFrontWait, s))) return r;
        if ((r = layer_temporal(c, i, twin, half, half, c->side))) return r;
    } else {
        if ((r = layer_rows(c, i, twin, 0, half, s, s))) return r;
        if (twin_aliased(c, twin)) {
            // twin aliasing: group 1 reads group 0's mf / ys instead of producing its own
            MC_HIP(hipEventRecord(c->ev_join, s));
            MC_HIP(hipStreamWaitEvent(c->side, c->ev_join, 0));
        }
        if ((r = layer_rows(c, i, twin, half, half, c->side, c->side))) return r;
        if ((r = expert_rows_guard(c, p, kFrontRead | kFrontWait, s))) return r;
    }
    if ((r = dbg_hold(c, c->side, s))) return r;      // (tests) hold one sample group's stream in front of its tail: > 0 the second group, < 0 the first
    if ((r = layer_rows_tail(c, i, hs, step, twin, 0, half, s, p.stagger ? c->ev_stag : nullptr, nullptr))) return r;
    return layer_rows_tail(c, i, hs, step, twin, half, half, c->side, nullptr, p.stagger ? c->ev_stag : nullptr);
}

// `seed` != nullptr: x_t is overwritten in place on its first frames before the network reads it (mc_sample_step_seeded)
int denoise_impl(mc_ctx* c, const float* x_t, int32_t step, float* out2_dev, int32_t stop_after, void* stream, const SeedArgs* seed) {
    MC_REQUIRE(c && x_t, "null argument");
    MC_REQUIRE(c->have_cond, "mc_ctx_set_condition not called");
    MC_REQUIRE(step >= 0 && step < c->S, "step_index %d outside the %d-step schedule", step, c->S);
    if (c->graph_mode) step = 0;       // host-side table pointers address step 0; the kernels add *gstep rows
    if (c->rows_mode) step = 0;        // ... or every row its own index (mc_sample_rows / mc_denoise_rows checked them on the host)
    hipStream_t s = (hipStream_t)stream;
    const mc_model_config& g = c->m->cfg;
    const int L = g.latent_dim, H = g.num_parts, D = L * H, C = g.input_feats;
    const long BT = (long)c->B * c->T;
    int r;
    if ((r = pick_side_stream(c, s))) return r;        // once per caller stream: the side stream that really runs beside it (hardware queues)
    // PoseEncoder as one dense [C -> D] GEMM with the scattered weight, + sequence_embedding[:T],
    // written to both CFG halves (stmogen.py:336-353; diffusion_transformer.py:215-218; stmogen.py:740)
    {
        const bool padded = c->xpad_ready && !seed;        // mc_sample_loop: the previous step's sampler update wrote the rows already
        c->xpad_ready = false;
        if (seed) { if ((r = mc_launch_pad_rows_seeded(const_cast<float*>(x_t), c->xpad, BT, C, c->m->Cp, *seed, s))) return r; }
        else if (!padded && (r = mc_launch_pad_rows(x_t, c->xpad, BT, C, c->m->Cp, s))) return r;
        GemmArgs e;
        mc_gemm_opts(c->opt, e);
        e.A = c->xpad; e.lda = c->m->Cp;
        e.W = c->enc_w; e.ldw = c->m->Cp; e.bias = c->enc_b;
        e.add = c->seq_emb; e.add_mod = c->T; e.ld_add = D;
        e.C = c->h; e.ldc = D; e.dup_rows = BT;
        e.M = (int)BT; e.N = D; e.K = c->m->Cp;
        if (BT <= c->opt.small_gemm_rows && D % 64 == 0 && c->m->Cp % 32 == 0) { if ((r = mc_launch_gemm_small(e, s))) return r; }
        else if ((r = mc_launch_gemm(GM_ENC, e, 1, 0, s))) return r;
    }
    const int nl = stop_after >= 0 ? (stop_after < g.num_layers ? stop_after : g.num_layers) : g.num_layers;
    c->no_alias = stop_after >= 0 && stop_after < g.num_layers;
    const int NC = c->have_ctrl ? g.num_ctrl_layers : 0;
    // large batches: the CFG halves run on two streams (see run_layer) and stay there across the layers, the control branch's row-wise
    // ops between them included
    const bool fused = chain_on(c, kChainGate) && chain_on(c, kChainRowchain) && mc_mlp_supported(L, 32);
    const bool two_groups = c->side && chain_on(c, kChainTwoStreams) && c->N > c->opt.big_tokens && fused;
    // row-wise op between layers, on the stream of the sample group that owns the rows (one launch on one stream)
    auto by_group = [&](auto&& fn) -> int {
        if (!two_groups) return fn(0L, c->rows, s);
        if (int e = fn(0L, BT, s)) return e;
        return fn(BT, BT, c->side);
    };
    for (int i = 0; i < nl; ++i) {
        // ControlT2MHalf.forward_test (controlnet.py:372-413): base block 0, then for index 1..copy:
        //   c, c_skip = controlnet[index-1](x=h, c=c);  h = base[index](h + c_skip)
        if (i >= 1 && i <= NC) {
            const int j = i - 1, slot = g.num_layers + j;
            if (j == 0) {                                                                              // x + before_proj(c)
                if ((r = by_group([&](long r0, long n, hipStream_t sk) {
                         return mc_launch_add_rows(c->hc + r0 * D, c->h + r0 * D, c->cb + r0 * D, nullptr, n, D, sk); })))
                    return r;
            }
            if ((r = run_layer(c, slot, c->hc, step, false, two_groups, s))) return r;                       // copied_block
            const LayerW& cw = c->lw[slot];
            if ((r = by_group([&](long r0, long n, hipStream_t sk) {                                   // h += after_proj(c)
                     if (const HalfW* hp = half_planes(c, &cw.h_after))
                         return dense_h(c, c->hc + r0 * D, *hp, cw.after_b, c->h + r0 * D, c->h + r0 * D, n, D, D, sk);
                     return dense(c, c->hc + r0 * D, D, cw.after_w, D, cw.after_b, c->h + r0 * D, D, c->h + r0 * D, D, n, D, D, ACT_NONE, sk); })))
                return r;
        }
        if ((r = run_layer(c, i, c->h, step, i == 0, two_groups, s))) return r;
    }
    if (two_groups && (r = side_join(c, s))) return r;       // the groups meet again before the pose decoder
    if (stop_after >= 0) return MC_OK;
    // PoseDecoder as one dense [D -> C] GEMM (stmogen.py:505-544), /2 folded into the packed weight
    float* o = out2_dev ? out2_dev : c->out2;
    return dense(c, c->h, D, c->dec_w, D, c->dec_b, nullptr, 0, o, C, c->rows, C, D, ACT_NONE, s);
}

SamplerCoefs to_coefs(const mc_step_coefs* k) {
    SamplerCoefs c;
    c.mode = k->mode; c.text_coef = k->text_coef; c.none_coef = k->none_coef; c.c1 = k->c1; c.c2 = k->c2;
    c.log_var = k->log_var; c.sqrt_recip = k->sqrt_recip; c.sqrt_recipm1 = k->sqrt_recipm1; c.ab = k->ab;
    c.ab_prev = k->ab_prev; c.eta = k->eta; c.nonzero = k->nonzero;
    return c;
}

// The pose decoder is affine, so  w dec(h_text) + (1 - w) dec(h_none) = dec(w h_text + (1 - w) h_none):  the sampler
// entry points combine the two CFG halves of the residual stream first and decode B*T rows instead of 2*B*T
// (mc_denoise, which hands out both decoded halves, keeps the reference's order).
// -> *x0: the prediction, or the two partial products of the folded tail (summed by the sampler kernel)
int denoise_combined(mc_ctx* c, const float* x_t, int32_t step, const mc_step_coefs* k, void* stream, X0Parts* x0, const SeedArgs* seed) {
    const mc_model_config& g = c->m->cfg;
    // ... and so is the Linear of the very last StylizationBlock (h += a W^T + b): it, too, runs once on the combined
    // rows  h_c = comb(h) + comb(a) W^T + b  instead of on both halves (defer_last_gemm: the layers leave that GEMM out).
    c->defer_last_gemm = true;
    int r = denoise_impl(c, x_t, step, nullptr, g.num_layers, stream, seed);   // all layers (minus that GEMM), no decoder
    c->defer_last_gemm = false;
    if (r != MC_OK) return r;
    hipStream_t s = (hipStream_t)stream;
    const int D = g.latent_dim * g.num_parts, C = g.input_feats;
    const long BT = (long)c->B * c->T;
    const LayerW& w = c->lw[g.num_layers - 1];
    *x0 = X0Parts{c->out2, nullptr};       // (every form below leaves its one or first output in out2)
    // rows mode (mc_sample_rows): the same forms below, their CFG weights read per request row from the tick's table
    const RowTab* const rt = c->rows_mode ? &c->rowtab : nullptr;
    auto combine = [&](const float* x, const float* y, float* out) -> int {      // w x + (1 - w) y, w = this step's CFG weight
        if (rt) return mc_launch_axpby_rows(x, y, *rt, D, out, BT * D, s);
        if (c->graph_mode) return mc_launch_cfg_combine_tab(x, y, c->gcoefs, c->gstep, out, BT * D, s);
        return mc_launch_axpby(x, y, k->text_coef, k->none_coef, out, BT * D, s);
    };
    const bool folded = c->dec_cat_w != nullptr;      // the Linear composed with the decoder at pack time (a model with dec.wf / dec.bf bound)
    if (folded && chain_on(c, kChainTailOnePass) && BT > c->opt.small_gemm_rows && D % 32 == 0) {
        // large batches: CFG combination, both K groups and the biases in ONE GEMM pass (gemm_tail_k): no axpby_pair_k, no partial outputs
        TailArgs t;
        t.H = c->h; t.Af = deferred_a(c); t.half = BT * D; t.lda = D;
        t.W = c->dec_cat_w; t.ldw = D; t.w_gstride = (long)C * D; t.bias = c->dec_cat_b; t.b_gstride = C;
        t.C = c->out2; t.ldc = C; t.M = (int)BT; t.N = C; t.K = D;
        t.wc = k->text_coef; t.wu = k->none_coef;
        if (c->graph_mode) {
            static_assert(sizeof(SamplerCoefs) % sizeof(float) == 0 && offsetof(SamplerCoefs, none_coef) == offsetof(SamplerCoefs, text_coef) + sizeof(float), "SamplerCoefs layout");
            t.coef_table = reinterpret_cast<const float*>(c->gcoefs) + offsetof(SamplerCoefs, text_coef) / sizeof(float);
            t.coef_stride = sizeof(SamplerCoefs) / sizeof(float);
            t.step_ptr = c->gstep;
        }
        if (rt) {
            t.coef_table = reinterpret_cast<const float*>(rt->coefs) + offsetof(SamplerCoefs, text_coef) / sizeof(float);
            t.coef_stride = sizeof(SamplerCoefs) / sizeof(float);
            t.rows_T = rt->T; t.rows_B = rt->B;
        }
        t.tune = (int)c->opt.gemm_tune;
        t.C2 = c->out2 + BT * C;               // (out2 holds [2 B T][C]: room for one partial product per K group)
        if ((r = mc_launch_gemm_tail(t, s))) return r;
        if (mc_gemm_tail_two_outputs(t)) x0->b = t.C2;      // gemm_tail2_k: x0 = C + C2, added by the sampler-update kernel
        return MC_OK;
    }
    if (folded) {
        // h_c and a_c in one launch
        if (rt) { if ((r = mc_launch_axpby_pair_rows(c->h, c->h + BT * D, c->z2, deferred_a(c), deferred_a(c) + BT * D, c->z2 + BT * D, *rt, D, BT * D, s))) return r; }
        else if ((r = mc_launch_axpby_pair(c->h, c->h + BT * D, c->z2, deferred_a(c), deferred_a(c) + BT * D, c->z2 + BT * D, k->text_coef, k->none_coef,
                                      c->graph_mode ? c->gcoefs : nullptr, c->graph_mode ? c->gstep : nullptr, BT * D, s))) return r;
        // ... and that Linear composed with the decoder is one [C, D] matrix (folded at pack time):
        //   x0 = [dec(h_c) + Wd b] + [a_c (Wd W)^T]
        // the two skinny products (N = C = 322: 294 tiles each, half a chip) are the two groups of ONE grouped GEMM
        // over (h_c | a_c) x (Wd | Wd W); the sampler kernel adds the two partial outputs
        GemmArgs t;
        mc_gemm_opts(c->opt, t);
        t.A = c->z2; t.lda = D; t.a_gstride = BT * D; t.W = c->dec_cat_w; t.ldw = D; t.w_gstride = (long)C * D;
        t.bias = c->dec_cat_b; t.b_gstride = C; t.C = c->out2; t.ldc = C; t.c_gstride = BT * C;
        t.M = (int)BT; t.N = C; t.K = D;
        x0->b = c->out2 + BT * C;
        return D % 32 == 0 ? mc_launch_gemm_small(t, s, 2) : mc_launch_gemm(GM_PLAIN, t, 2, 0, s);
    }
    // no folded weight: both combinations, the Linear on the combined rows, then the decoder
    float* const ad = deferred_a(c);
    if ((r = combine(c->h, c->h + BT * D, c->z2))) return r;     // h_c
    if ((r = combine(ad, ad + BT * D, ad))) return r;            // a_c
    if ((r = dense(c, ad, D, w.ffn_out_w, D, w.ffn_out_b, c->z2, D, c->z2, D, BT, D, D, ACT_NONE, s))) return r;  // h_c += a_c W^T + b
    return dense(c, c->z2, D, c->dec_w, D, c->dec_b, nullptr, 0, c->out2, C, BT, C, D, ACT_NONE, s);
}

// The sampler update behind denoise_combined, for the per-step entry, the fused loop and the captured step: gathers what the context
// has set into ONE description of the form (mc_launch_sampler picks the kernel).  Under capture the coefficients (the mode among
// them) come from the device table at replay, so the mode is what mc_ctx_graph_capture found in the table (all mode 2 or none of it),
// not the step-0 entry `k`'s.  Per-row schedules (one mode per call, checked by mc_sample_rows) go with no graph and no whole-batch
// seam table, an edit table with no row seam table unless the context's long-edits switch is on (mc_ctx_set_long_edits).
int sampler_update(mc_ctx* c, const float* x_t, const X0Parts& x0p, const mc_step_coefs* k, const float* noise, float* x_prev, float* x0,
                   hipStream_t s, const RngArgs* rng, const PadOut* pad) {
    if (c->rows_mode && (c->graph_mode || c->seam_ov > 0)) { mc_set_error("per-row sampler update under graph capture or with a seam table set"); return MC_ERR_STATE; }
    if (c->rows_mode && c->seam_rows_ov > 0 && c->edit_set && !c->long_edits) { mc_set_error("per-row sampler update with a row seam table and an edit table set"); return MC_ERR_STATE; }
    if (c->seam_ov > 0 && c->graph_mode) { mc_set_error("sampler update under graph capture with a seam table set"); return MC_ERR_STATE; }
    const bool multistep = c->graph_mode ? c->graph_multistep : k->mode == MC_SAMPLER_MULTISTEP;
    const int C = c->m->cfg.input_feats;
    SamplerForm f;
    f.x_t = x_t; f.out_text = x0p.a; f.out_none = x0p.second(); f.x_prev = x_prev; f.x0_out = x0;
    f.n = (long)c->B * c->T * C;
    f.c = x0p.coefs(k);
    f.mode = c->graph_mode ? (multistep ? (int)MC_SAMPLER_MULTISTEP : (int)MC_SAMPLER_DDPM) : k->mode;      // (under capture only "2 or not" is read)
    f.pad = pad;
    MC_REQUIRE(!multistep || c->x0_hist, "multistep update without a history buffer");
    if (multistep) f.x0_hist = c->x0_hist;
    else f.noise = noise;
    // a seed table (mc_ctx_set_row_seeds): an in-kernel draw takes every row's own key; a noise tensor is read as it is
    const RowKeys rk{reinterpret_cast<const uint32_t*>(c->row_seeds), c->T * C};
    const bool drawn = !multistep && !noise;
    if (c->row_seeds_set && drawn && (rng || c->rows_mode)) f.keys = &rk;
    EditTab et;
    SeamTab st;
    SeamRowsTab sr;
    if (c->rows_mode) {
        MC_REQUIRE(!drawn || c->row_seeds_set, "per-row sampler update without a noise tensor needs a seed table (mc_ctx_set_row_seeds)");
        f.rt = &c->rowtab; f.TC = rk.TC;
        if (c->seam_rows_ov > 0) {       // windows of long requests among the rows (mc_ctx_set_seam_rows)
            sr.rows = c->seam_rows_tab; sr.w = reinterpret_cast<const float*>(c->seam_rows_tab + c->B);
            sr.T = c->T; sr.C = C; sr.ov = c->seam_rows_ov;
            f.seam_rows = &sr;
        }
        if (c->edit_set) {               // a kept region (mc_ctx_set_edit_rows); beside a row seam table under mc_ctx_set_long_edits
            MC_REQUIRE(multistep || !noise || k->mode == MC_SAMPLER_DDPM, "edited rows in mode 1 draw the kept region's noise from the seed table: no noise tensor");
            et.gt = c->edit_gt; et.keep = c->edit_keep;
            f.edit = &et;
        }
    } else {
        f.rng = rng;
        if (c->seam_ov > 0) {            // the batch as coupled windows (mc_ctx_set_seams)
            st.flags = c->seam_tab; st.w = reinterpret_cast<const float*>(c->seam_tab + c->B);
            st.T = c->T; st.C = C; st.ov = c->seam_ov;
            f.seam = &st;
        } else if (c->graph_mode) { f.table = c->gcoefs; f.step_ptr = c->gstep; }
    }
    return mc_launch_sampler(f, s);
}
