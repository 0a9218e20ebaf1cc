/* C-ABI of libmotioncraft_amd.so -- the MI355X (gfx950) STMoGen sampling hot path.
 *
 * This is the drop-in boundary for the per-step denoising path of cure-lab/MotionCraft
 * (SURVEY.md section 8b).  The reference is pure Python/PyTorch and has no FFI of its own; the
 * entry points below are what a binding for that path replaces, each citing the reference
 * interface (paths relative to the reference root):
 *
 *   mc_model_*            weights of  STMoGenTransformer               mogen/models/transformers/stmogen.py:626-653
 *                         (state dict as loaded by mmcv load_checkpoint, tools/test.py:99)
 *   mc_ctx_set_timesteps  timestep_map of SpacedDiffusion/_WrappedModel  mogen/models/utils/gaussian_diffusion.py:1416-1463
 *                         + time_embed / emb_layers hoists             diffusion_transformer.py:89-93,206-208; stylization_block.py:17-20
 *   mc_ctx_set_condition  model_kwargs {xf_out, motion_mask}           mogen/models/architectures/diffusion_architecture.py:166-174
 *                         + per-layer text_moe K/V hoist               mogen/models/attentions/st_attention.py:116-118
 *   mc_ctx_set_control    ControlT2MHalf.forward_c + before_proj           mogen/models/transformers/controlnet.py:66,186-199
 *   mc_denoise            model(x, ts, **model_kwargs)                 diffusion_transformer.py:186-238 -> stmogen.py:725-761
 *   mc_sample_step        GaussianDiffusion.p_sample / ddim_sample     gaussian_diffusion.py:634-696, 799-852
 *   mc_sample_step_inpaint  the same with y = {gt, outpainting_mask}   gaussian_diffusion.py:492-501, 855-877
 *   mc_sample_step_seeded   the same with pre_seq / transl_req         gaussian_diffusion.py:664-674, 816-820
 *   mc_ctx_set_seams      no reference counterpart: all windows of a long sequence as rows of ONE batch, the overlapping frames of
 *                         neighbouring windows blended after every denoiser call (the reference walks windows one by one, tools/m2d_test.py:139-232)
 *   mc_textenc_*          DiffusionTransformer.encode_text (CLIP text tower, text_pre_proj, textTransEncoder, text_ln)
 *                                                                      mogen/models/transformers/diffusion_transformer.py:109-172
 *   mc_evalenc_*          T2MContrastiveModel_SMPLX.encode_motion / encode_text (evaluation embeddings)
 *                                                                      mogen/models/rnns/t2m_bigru_smplx.py:66-437
 *   mc_t2meval_*          T2MContrastiveModel.encode_motion / encode_text (HumanML3D / KIT evaluation embeddings)
 *                                                                      mogen/models/rnns/t2m_bigru.py:72-299
 *   mc_wavenc_*           WavEncoder (audio condition pre-encoder)     mogen/models/utils/blocks.py:11-71; controlnet.py:90-105,187
 *   mc_postprocess_smplx  de-normalise + SMPL-X re-pack + temporal filter  tools/visualize.py:39-44,217-246; tools/s2g_test.py:289-297
 *   mc_postprocess_t2m_joints  HumanML3D / KIT features -> filtered joint positions (plot_t2m, recover_from_ric)
 *                                                                      tools/visualize.py:46-56; mogen/utils/plot_utils.py:40-104
 *   mc_smplx_*            the SMPL-X body model (55 joints, vertices) the tools run on the saved poses / expressions / trans
 *                                                                      tools/s2g_test.py:76-85,364-412; tools/visualize.py:71-86
 *   mc_smplx_vertex_errors  the face l2 / lvel sums over the vertices of sample and target   tools/s2g_test.py:377-412
 *   mc_beat_mask, mc_beat_align  alignment.load_pose / calculate_align (beat alignment score)
 *                                                                      mogen/datasets/EMAGE_2024/utils/metric.py:78-127,199-242
 *   mc_onset_strength, mc_onset_pick  alignment.load_audio (librosa's onset_detect)   metric.py:64-76
 *   mc_audio_condition    the S2G audio condition `onset+amplitude` [samples, 2]   mogen/datasets/EMAGE_2024/dataloaders/beat_motionx.py:398-412
 *   mc_pcm_decode, mc_resample_poly  librosa.load + librosa.resample in front of both (res_type='polyphase', not the default soxr_hq)
 *                                                                      dataloaders/beat_sep_lower.py:392-393; tools/s2g_test.py:416-417
 *   mc_render_*           the frames fast_render.generate_silent_videos* draws (orthographic rasteriser; own shading model)
 *                                                                      mogen/datasets/EMAGE_2024/utils/fast_render.py:13-81; other_tools.py:695-765
 *   mc_mjpeg_*            convert_img_to_mp4 / add_audio_to_video: frames -> one video file (baseline JPEG on the device, for a Motion-JPEG AVI)
 *                                                                      mogen/datasets/EMAGE_2024/utils/media.py:4-33
 *   mc_emb_frechet, mc_emb_statistics, mc_emb_zscore, mc_emb_retrieval, mc_emb_pair_distance  the metric functions over embedding tables
 *                         (Frechet distance, R precision, matching score, diversity, multimodality)   mogen/core/evaluation/utils.py:12-140
 *   mc_op_renoise         GaussianDiffusion._undo (resampling jumps)   gaussian_diffusion.py:429-435, 1113-1118
 *
 * Conventions: plain pointers and sizes only.  `*_dev` pointers are device (HBM) addresses owned
 * by the caller (e.g. torch allocations); `stream` is a hipStream_t passed as void*.  All tensors
 * are fp32, contiguous, row-major.  Every function returns 0 on success or an MC_ERR_* code;
 * mc_last_error() returns a thread-local description.  A handle is re-entrant across handles but
 * not thread-safe per handle.  No call synchronises the device except mc_model_set_param
 * (synchronous H2D upload), the *_create/_destroy functions and mc_emb_frechet (it waits for `stream` once per
 * Jacobi sweep to read the count of rotated pairs, so it cannot be captured into a graph).
 */
#ifndef MOTIONCRAFT_AMD_H
#define MOTIONCRAFT_AMD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MC_OK 0
#define MC_ERR_ARG 1
#define MC_ERR_HIP 2
#define MC_ERR_STATE 3
#define MC_ERR_NOCONV 4   /* an iteration reached its cap without converging (mc_emb_frechet) */

typedef struct mc_model mc_model;
typedef struct mc_ctx mc_ctx;

/* the configs under configs/stmogen: model=dict(type='STMoGenTransformer', ...) */
typedef struct mc_model_config {
    int32_t input_feats;      /* 322 (SMPL-X motionx layout)                       */
    int32_t max_seq_len;      /* 196                                               */
    int32_t latent_dim;       /* L: per-part latent (ca_block_cfg.latent_dim)      */
    int32_t num_parts;        /* H: 12 body parts (ca_block_cfg.num_heads)         */
    int32_t num_layers;       /* NL                                                */
    int32_t ffn_dim;          /* F: SFFN hidden (ffn_cfg.ffn_dim)                  */
    int32_t time_embed_dim;   /* Te                                                */
    int32_t text_latent_dim;  /* Dt                                                */
    int32_t max_text_len;     /* Nt = 77                                           */
    int32_t num_experts;      /* E = 16                                            */
    int32_t topk;             /* 2                                                 */
    int32_t dyn_heads;        /* 8 (st_attention.py:95)                            */
    float capacity_factor;    /* 1.5 (st_attention.py:33)                          */
    float cfg_scale;          /* scale_func_cfg.scale = 6.5                        */
    /* plug-and-play control branch ControlT2MHalf (mogen/models/transformers/controlnet.py:107-183); 0 = none */
    int32_t num_ctrl_layers;  /* copy_blocks_num                                   */
    int32_t ctrl_cond_feats;  /* width of the condition fed to control_cond_input  */
    int32_t ctrl_condition_cfg; /* condition_encode_cfg.condition_cfg: zero c in the uncond half */
} mc_model_config;

/* per-step scalars of the sampler, fp64 schedule tables cast to fp32 like _extract_into_tensor
 * (gaussian_diffusion.py:1330-1343) */
#define MC_SAMPLER_DDPM 0
#define MC_SAMPLER_DDIM 1
#define MC_SAMPLER_MULTISTEP 2
/* mode MC_SAMPLER_MULTISTEP (DPM-Solver++ 2M on the data prediction; the reference has no counterpart): the update is
 *   x_prev = c2 x + c1 x0 + eta x0_prev
 * c1 = coefficient of x0 and c2 = coefficient of x (their roles in mode 0), eta = k1, the coefficient of the x0 of the step taken
 * before this one (kept by the context, buffer "x0_hist"; never read when eta == 0).  text_coef / none_coef as in every mode; all
 * other fields are ignored, no noise is drawn.  The host computes the three scalars for a whole walk
 * (GaussianDiffusion.multistep_coefs). */
typedef struct mc_step_coefs {
    int32_t mode;             /* MC_SAMPLER_*: 0 = DDPM p_sample, 1 = DDIM ddim_sample, 2 = multistep (above) */
    float text_coef;          /* w = 1 + scale * t_orig / 1000 (stmogen.py:655-659) */
    float none_coef;          /* 1 - w                                             */
    float c1, c2;             /* posterior_mean_coef1/2[i]                          */
    float log_var;            /* log(append(posterior_variance[1], betas[1:]))[i]   */
    float sqrt_recip, sqrt_recipm1, ab, ab_prev, eta;   /* DDIM                     */
    float nonzero;            /* (t != 0)                                           */
} mc_step_coefs;

/* RePaint / outpainting operands of one step (long-sequence windows): model_kwargs['y'] of the reference */
typedef struct mc_inpaint {
    const float* gt_dev;          /* y['gt'] [B,T,C]                                                  */
    const uint8_t* keep_dev;      /* y['outpainting_mask'] [B,T,C], one byte per element (torch.bool)  */
    const float* gt_noise_dev;    /* 2nd randn_like of ddim_sample (:868) [B,T,C]; unused for DDPM     */
    const float* blend_w_dev;     /* linspace(0,1,overlap_len) (:873); may be NULL when blend_len == 0 */
    int32_t blend_len;            /* overlap_len if sqrt(1-alpha_bar_prev) < 0.2 and opt.addBlend, else 0 */
} mc_inpaint;

/* pre_seq / transl_req seeding of one step (p_sample :664-674, ddim_sample :816-820): before the network sees x_t,
 * x[:, :pre_len, :] = q_sample(pre_seq, t, randn_like(pre_seq)) and x[:, :2, channel_k] = q_sample(transl_k, t, randn(2)) */
#define MC_MAX_TRANSL 8
typedef struct mc_seed {
    const float* pre_seq_dev;     /* [B, pre_len, C]; may be NULL when pre_len == 0                                  */
    const float* pre_noise_dev;   /* [B, pre_len, C] the randn_like(pre_seq) of THIS step                            */
    int32_t pre_len;              /* pre_seq.shape[1]                                                                */
    float sqrt_ab, sqrt_1mab;     /* sqrt_alphas_cumprod[i], sqrt_one_minus_alphas_cumprod[i] cast to fp32           */
    int32_t num_transl;           /* len(transl_req) <= MC_MAX_TRANSL (DDPM only)                                     */
    int32_t transl_channel[MC_MAX_TRANSL];   /* item[0]                                                              */
    float transl_value[MC_MAX_TRANSL][2];    /* q_sample(item[1:], t, randn(2)): 2 scalars, evaluated by the host     */
} mc_seed;

const char* mc_last_error(void);
int mc_device_count(int* n);
int mc_set_device(int dev);

/* ---- model (weights) -------------------------------------------------------------- */
int mc_model_create(const mc_model_config* cfg, mc_model** out);
void mc_model_destroy(mc_model* m);
/* Upload one packed fp32 parameter from host memory.  Names and layouts: motioncraft_amd/weights.py */
int mc_model_set_param(mc_model* m, const char* name, const float* host, int64_t numel);
int mc_model_finalize(mc_model* m);

/* ---- context = workspace for one (batch, frames) shape ------------------------------ */
int mc_ctx_create(mc_model* m, int32_t batch, int32_t frames, int32_t max_steps, mc_ctx** out);
void mc_ctx_destroy(mc_ctx* c);
int64_t mc_ctx_workspace_bytes(const mc_ctx* c);
/* Synchronises `stream` and reports a sticky device-side error of the context (MC_ERR_STATE): today the one error a kernel can
 * raise is the grid-barrier time-out of the cooperative routing kernel (route_coop_k; its grid is reserved out of the device's
 * resident-workgroup capacity per context at mc_ctx_create, so only barrier kernels of ANOTHER process can starve it).  The
 * Python sampler loops call it once after the last step -- the reference has no counterpart (its routing is tutel's, on the
 * framework's stream: st_attention.py:28-45). */
int mc_ctx_check(mc_ctx* c, void* stream);
/* Measurement hook (bench.py `roofline.dominant_kernel`; no reference counterpart): while on, every FiLM out_layers GEMM launch
 * (h += Linear(a), stylization_block.py:39 -- the dominant kernel of a step) is bracketed by HIP events recorded on the stream it is
 * launched on.  mc_ctx_profile_read waits for them and returns the average duration (us), the number of launches and the
 * algorithmic GFLOP of one launch (2 rows D^2); rows_filter > 0 keeps only launches of that many rows. */
int mc_ctx_profile(mc_ctx* c, int32_t on);
int mc_ctx_profile_read(mc_ctx* c, int64_t rows_filter, double* avg_us, int32_t* count, double* gflop_per_launch);
/* the precision the per-step kernels of this context actually run in: MC_PREC_F32 also when a reduced-precision mode is set but
 * the batch is at most MC_HALF_MIN_ROWS (512) residual rows, where the fp32 small-batch kernels are the faster ones (B = 1) */
int mc_ctx_effective_precision(const mc_ctx* c);
/* 1 if this context routes its layers with the one-launch cooperative kernel (0: one-workgroup kernels or the launch sequence) */
int mc_ctx_uses_coop_routing(const mc_ctx* c);
/* tests: keep the routing decisions (expert ids, combine weights; 0 = dropped) of every layer of the
 * last mc_denoise call in buffers "cap_idx" / "cap_w" */
int mc_ctx_enable_capture(mc_ctx* c);
/* MFMA operand precision of the per-step GEMM-shaped kernels of this context (FiLM out_layers GEMMs, expert and SFFN MLPs,
 * control after_proj): the "fp16 MFMA" mode of BASELINE.json configs[4]; the reference hook is mmcv's wrap_fp16_model
 * (tools/test.py:95-97).  MC_PREC_F32 (default): exact fp32 MFMA.  MC_PREC_F16: operands rounded to fp16, fp32
 * accumulate (~2e-4 relative per GEMM stage).  MC_PREC_F16X3: operands split x = hi + lo in fp16, three products
 * hi*hi + hi*lo + lo*hi accumulated in fp32 -- fp32-class results at 3/16 of the fp32 MFMA time.  The gate, routing,
 * LayerNorm statistics, softmaxes and all elementwise work stay fp32 in every mode (tutel forces fp32_gate,
 * st_attention.py:31).  The fp16 weight planes are built once per model on the first call.
 * Tolerance: MC_PREC_F16X3 meets every bound of the fp32 path (tests/test_gpu_parity.py holds it to the same 2e-4 per call /
 * 1e-3 per trajectory).  MC_PREC_F16 is OUTSIDE the north-star tolerance on the x0 prediction (8e-3 observed at B = 16, t = 640: one
 * fp16 rounding per operand, amplified by the classifier-free-guidance weights); what it meets is 1e-3 on x_{t-1} of every sampler
 * step (1.1e-4 observed), since the update damps the x0 error -- the same class of result as the reference under
 * wrap_fp16_model, which is what configs[4] names. */
#define MC_PREC_F32 0
#define MC_PREC_F16 1
#define MC_PREC_F16X3 2
int mc_ctx_set_precision(mc_ctx* c, int32_t precision);
/* tutel boundary (parity unpinned): order of tokens with EXACTLY equal importance (max gate score) at an
 * expert's capacity cut.  tutel ranks by `importance_scores.argsort(dim=0)` -- not a stable sort, so the order of ties is
 * implementation-defined there.  MC_TIE_STABLE (default): lower token index first (what a stable sort / radix sort
 * gives; oracle/tutel_restated.py TIE_POLICY='stable'); MC_TIE_REVERSE: higher index first.  One switch in the kernel
 * and one in the oracle, so a golden from a real tutel install can be matched without kernel work.  Call before
 * mc_ctx_set_condition (the hoisted text K/V are routed too). */
#define MC_TIE_STABLE 0
#define MC_TIE_REVERSE 1
int mc_ctx_set_tie_policy(mc_ctx* c, int32_t policy);
/* Capacity factor of THIS context (no reference counterpart as a runtime switch: the reference fixes 1.5 in st_attention.py:33).  The
 * capacity cut is what makes a row of a batch depend on its batchmates: capacity = topk * int(cf * ceil(N / E)) is taken over all
 * tokens of the call and batch-prioritised routing drops the lowest-scoring tokens of a full expert.
 *   cf > 0   tutel's formula with this factor instead of the model's.  The default is the model's capacity_factor: nothing changes
 *            unless this is called.
 *   cf == 0  no (token, choice) pair is ever dropped, and no selection work runs (no histogram / radix pass, none of the cooperative
 *            kernel's selection barriers, no selection pass of the early schedule): comb_w == gate bit for bit, the twin-split flag
 *            is 0, counts / slot ranges / tile maps are those of a routing in which no expert overflowed.  A row's result then is a
 *            function of its own request at a fixed (batch, frames, options).
 *            [tutel-recall] tutel's own capacity_factor = 0 sizes the capacity to the largest expert load, i.e. drops nothing too.
 *   cf < 0   MC_ERR_ARG (tutel's negative form -- a cap on the adaptive capacity -- is not built).
 * Applies to the motion MoE of every layer slot (base and control) and to the hoisted text MoE, so the call clears the context's
 * condition and the multistep history flag: mc_ctx_set_condition must follow before the next denoiser call (which otherwise fails
 * as on a fresh context).  MC_ERR_STATE while a captured graph exists (mc_ctx_graph_release first).
 * Checkpoints were trained with drops at 1.5; sample quality at 0 is unmeasured. */
int mc_ctx_set_capacity_factor(mc_ctx* c, float cf);
float mc_ctx_capacity_factor(const mc_ctx* c);
/* Kernel-selection switches of ONE context (no reference counterpart: the reference has one code path; these exist for A/B
 * measurement and for the tests that pin alternative kernels to each other).  The MC_* environment variable of a key only seeds
 * the default of contexts created afterwards (and of context-free calls such as mc_op_gemm, read once per process); two contexts
 * of one process may differ.  Key (variable, default):
 *   "chain" (MC_CHAIN, 762806311: bit mask; the retired bits 3, 4, 6 - 14, 19, 23, 25, 28 and bits >= 30 are rejected),
 *   "small_gemm_rows" (MC_SMALL_GEMM_ROWS, 5600), "split_rows_expert" (MC_SPLIT_ROWS_EXPERT, 2048),
 *   "split_rows_sffn" (MC_SPLIT_ROWS_SFFN, 8192), "temporal_split" (MC_TEMPORAL_SPLIT, 96), "big_tokens" (MC_BIG_TOKENS, 65536),
 *   "rowchain_split" (MC_ROWCHAIN_SPLIT, 20480), "gemm_tune" (MC_GEMM_TUNE, 1841: bits 0, 4, 5, 6, 8, 9, 10 only),
 *   "small_tile_n" (MC_SMALL_TILE_N, 0: 0, 48, 64 or 96), "gemm_wp_grid" (MC_GEMM_WP_GRID, 512: <= 0 one workgroup per tile),
 *   "half_min_rows" (MC_HALF_MIN_ROWS, 512), "gate_small" (MC_GATE_SMALL, 12000), "split_expert" (MC_SPLIT_EXPERT, 0),
 *   "split_sffn" (MC_SPLIT_SFFN, 0), "route_reg" (MC_ROUTE_REG, 1), "route_coop" (MC_ROUTE_COOP, 1),
 *   "route_small" (MC_ROUTE_SMALL_CTX, else MC_ROUTE_SMALL, 20480: 0 .. 131072), "route_per" (none, 0: 0, 10 or 16),
 *   "route_early" (MC_ROUTE_EARLY, 1: 0 or 1; two-stream schedule: each sample group's experts start behind its own gate, 0 joins
 *   the groups in front of the routing; same bits either way; a context of a latent_dim = 64 model starts at 0 unless the variable
 *   is set: measured slower there),
 *   "dbg_delay_us" (none, 0: -100000 .. 100000; tests: holds one sample group's stream that long in front of every layer tail,
 *   so the two-stream schedule runs far out of phase; results must not change).
 * Results never depend on them beyond fp32 summation order where DESIGN.md says so.  An unknown key or a value outside the
 * stated range -> MC_ERR_ARG; an environment variable outside it fails mc_ctx_create (or the context-free call) with MC_ERR_ARG
 * naming the variable.  Not while a captured graph exists (mc_ctx_graph_release first). */
int mc_ctx_set_option(mc_ctx* c, const char* key, int64_t value);
int mc_ctx_set_timesteps(mc_ctx* c, const int32_t* t_orig_host, int32_t num_steps, void* stream);
int mc_ctx_set_condition(mc_ctx* c, const float* xf_out_dev, const float* mask_dev, void* stream);
/* control condition (ControlT2MHalf.forward_c + controlnet[0].before_proj, controlnet.py:186-199, 66):
 * c_feat_dev [B, Tc, ctrl_cond_feats] = output of the (step-invariant) condition_pre_encoder, Tc <= frames;
 * NULL disables the branch for this context (forward_test with c=None, controlnet.py:405-413). */
int mc_ctx_set_control(mc_ctx* c, const float* c_feat_dev, int32_t Tc, void* stream);

/* x_t_dev [B,T,C] at schedule index step_index -> out2_dev [2B,T,C] (text half, then uncond half);
 * out2_dev may be NULL (result stays in the context, buffer "out2").
 * stop_after_layers < 0: full model; >= 0: run only that many decoder layers and skip the pose
 * decoder (tests read intermediates through mc_ctx_get_buffer). */
int mc_denoise(mc_ctx* c, const float* x_t_dev, int32_t step_index, float* out2_dev,
               int32_t stop_after_layers, void* stream);
/* denoise + CFG combine + sampler update in one call; x0_dev may be NULL; x_prev_dev may alias x_t_dev.
 * Mode 2 (MC_SAMPLER_MULTISTEP) in mc_sample_step, mc_sample_loop, mc_ctx_graph_capture / _step: noise_dev may be NULL, seed and
 * noise_draw0 are ignored.  The context owns the history buffer "x0_hist" [B,T,C] (allocated on the first mode-2 call, or by
 * mc_ctx_graph_capture of a mode-2 table: contexts that never use the mode keep their workspace size) and a "history valid" flag:
 * a mode-2 step sets it; mc_ctx_set_condition, mc_ctx_set_control and mc_ctx_set_timesteps clear it; a mode-2 step with eta != 0
 * while it is clear is MC_ERR_STATE.  A graph is captured for one table: a table that mixes mode 2 with other modes is MC_ERR_ARG
 * (and a replay checks the flag on the host against the table entry of the step it is asked for).
 * mc_sample_step_inpaint and mc_sample_step_seeded return MC_ERR_ARG for mode 2. */
int mc_sample_step(mc_ctx* c, const float* x_t_dev, int32_t step_index, const mc_step_coefs* coefs,
                   const float* noise_dev, float* x_prev_dev, float* x0_dev, void* stream);

/* The sampler LOOP as one call -- GaussianDiffusion.p_sample_loop / ddim_sample_loop, gaussian_diffusion.py:698-797, 925-1049 (the
 * mode is in coefs[k].mode): runs schedule indices step_indices_host[0 .. num_steps) in order (the reference walks
 * num_timesteps-1 .. 0) with coefs_host[k], x_dev [B,T,C] updated IN PLACE, no return to the host language between steps.
 * The per-step th.randn_like(x) (gaussian_diffusion.py:684 / 847) is
 *   noise_dev != NULL: read from noise_dev [num_steps][B,T,C]  (parity runs on the reference's own seeds), or
 *   noise_dev == NULL: drawn inside the sampler-update kernel -- Philox4x32-10 keyed by `seed`, counter = (element / 4,
 *                      noise_draw0 + k), Box-Muller; mc_op_philox_normal writes the same draws to memory (bit for bit).
 * x0_last_dev (may be NULL) receives the last step's x0 prediction.  Asynchronous on `stream` like every other entry point. */
int mc_sample_loop(mc_ctx* c, float* x_dev, const int32_t* step_indices_host, const mc_step_coefs* coefs_host, int32_t num_steps,
                   const float* noise_dev, uint64_t seed, uint64_t noise_draw0, float* x0_last_dev, void* stream);
/* draw `draw` of the Philox stream keyed by `seed`: out_dev[n] = normals, bits_dev[n] = the raw 32-bit words (either may be NULL) */
int mc_op_philox_normal(float* out_dev, uint32_t* bits_dev, int64_t n, uint64_t seed, uint64_t draw, void* stream);
/* Row-keyed noise (no reference counterpart: the reference draws one randn over the batch).  While a seed table is set, the normal for
 * element r in [0, T*C) of row b in draw d is element r of mc_op_philox_normal(n = T*C, seed = seeds[b], draw = d): key seeds[b],
 * counter (r / 4, d), lane r % 4, the same Box-Muller.  A row gets exactly the noise a B = 1 call with that seed gets, whatever B is
 * and wherever the row sits.  It is read by
 *   mc_sample_loop with noise_dev == NULL: the `seed` argument is ignored, noise_draw0 + k stays the draw number (with a seam table
 *       too: a seam element takes the LEFT row's key and the left element's row-local counter);
 *   mc_ctx_draw_rows: out_dev [B,T,C] = draw `draw` of every row (MC_ERR_STATE without a table) -- every entry that takes noise_dev
 *       (mc_sample_step, graph replay, the inpaint and seeded steps) reaches row-keyed noise through it.
 * A noise_dev argument is read as it is, table or not; graph capture is unaffected.  seeds_host [B] is copied on `stream` (the call
 * synchronises it); NULL clears the table. */
int mc_ctx_set_row_seeds(mc_ctx* c, const uint64_t* seeds_host, void* stream);
int mc_ctx_draw_rows(mc_ctx* c, float* out_dev, uint64_t draw, void* stream);

/* Coupled windows of a long sequence (no reference counterpart; the window-parallel scheme of DoubleTake / MultiDiffusion): the B rows of
 * the context are windows of T frames, row b starting at global frame first_frame_host[b].  Rows b and b + 1 are NEIGHBOURS when
 * first_frame[b + 1] == first_frame[b] + T - overlap: the last `overlap` frames of b and the first of b + 1 are the same frames.  Rows
 * that are not neighbours must be disjoint (first_frame[b + 1] >= first_frame[b] + T: a new sequence); a partial overlap, a decreasing
 * list, a negative entry, or an overlap outside 0 < 2 overlap <= T is MC_ERR_ARG.  While a table is set, the sampler update of
 * mc_sample_step / mc_sample_loop (every mode) blends the two x0 predictions of a shared frame f,
 *     x0 = w[f] x0_right + (1 - w[f]) x0_left,     w = weight_host[overlap] in [0, 1], or NULL: w[f] = (f + 1) / (overlap + 1),
 * and gives both rows the SAME x_prev / x0 / history (computed once, with the LEFT row's noise element or Philox counter; the right
 * row's noise on its first `overlap` frames is not read).  Every other element gets the bits of the uncoupled update.
 * PRECONDITION (not checked): x_T is equal on shared frames; then x stays equal there bit for bit after every step.
 * The table is uploaded on `stream` (the call synchronises it); overlap == 0 clears it (the other arguments are ignored).  Setting or
 * clearing clears the multistep history flag.  While a table is set, mc_sample_step_inpaint, mc_sample_step_seeded and
 * mc_ctx_graph_capture return MC_ERR_STATE; with a captured graph in the context, setting a table is MC_ERR_STATE. */
int mc_ctx_set_seams(mc_ctx* c, int32_t overlap, const int32_t* first_frame_host, const float* weight_host, void* stream);

/* Per-row schedules: every request row b of the batch at its own schedule index and under its own coefficients,
 * the guidance weight (text_coef / none_coef) among them -- the reference's denoiser takes ts as a [B] tensor and its CFG weight is per
 * sample.  Row r of any [B T]- or [2 B T]-row operand belongs to request row (r / T) % B; sample b + B is the CFG twin of b.
 * mc_sample_rows: num_ticks ticks back to back, no return to the host between them; a tick is denoise, CFG combine, sampler update with
 *   row b at schedule index step_index_host[k][b] under coefs_host[k][b], x_dev [B,T,C] updated in place.  The noise of tick k is read
 *   from noise_dev + k B T C, or with noise_dev == NULL drawn in the kernel from the rows' keys (mc_ctx_set_row_seeds; MC_ERR_STATE
 *   without a table): row b takes draw draw_host[k][b], counter (row-local element / 4, draw).  x0_dev (may be NULL): x0 of the last tick.
 *   All entries of a call share one sampler mode (mixed: MC_ERR_ARG); an index outside the schedule is MC_ERR_ARG; num_ticks <=
 *   max_steps.  The kernels are the forms mc_sample_step picks at the same shape and options, so equal entries in every row give its bits.
 *   Mode 2: the "history valid" state is one flag per row -- a tick sets its rows' flags, eta != 0 on a row whose flag is clear is
 *   MC_ERR_STATE, a row with eta == 0 does not read the history.  Whatever sets or clears the context's flag (see mc_sample_step) sets
 *   or clears every row's.  The tables travel through context-owned pinned staging and device tables [max_steps][B], allocated by the
 *   first call of the mode; the call waits for the previous upload's event, never for the device.  Every argument is checked before
 *   the first launch: a call refused for its arguments or the context's state changes nothing.  A launch failure (MC_ERR_HIP) in
 *   tick k is not such a refusal: x_dev and the history have been advanced by ticks [0, k) and those ticks' row flags are kept.
 * mc_denoise_rows: mc_denoise (full model, both decoded halves in out2_dev [2B,T,C], no combine) with row b at step_index_host[b].
 * mc_ctx_set_condition_rows: mc_ctx_set_condition (the whole batch's text K/V are recomputed; at capacity factor 0 an unchanged row
 *   keeps its bits), but only rows with fresh_host[b] != 0 lose their history flag.
 * NOT in this mode: graph capture or replay (a context that holds a captured graph, or a capturing stream: MC_ERR_STATE), the
 * whole-batch seam table of mc_ctx_set_seams (MC_ERR_STATE), the inpaint and seeded steps (no rows entry).  The windows of a long
 * request ARE rows of this mode: mc_ctx_set_seam_rows below couples them per row. */
int mc_sample_rows(mc_ctx* c, float* x_dev, int32_t num_ticks, const int32_t* step_index_host, const mc_step_coefs* coefs_host,
                   const uint64_t* draw_host, const float* noise_dev, float* x0_dev, void* stream);
int mc_denoise_rows(mc_ctx* c, const float* x_t_dev, const int32_t* step_index_host, float* out2_dev, void* stream);
int mc_ctx_set_condition_rows(mc_ctx* c, const float* xf_out_dev, const float* mask_dev, const uint8_t* fresh_host, void* stream);

/* Edited rows: "these frames or channels are given, generate the rest" per request row -- keyframes,
 * in-betweening, continuing a motion, re-generating some body parts.  The reference's model_kwargs['y'] = {gt, outpainting_mask}
 * (gaussian_diffusion.py:492-501, 855-877) in the row form.  gt_dev [B,T,C] fp32 and keep_dev [B,T,C] bytes (non-zero: given), both in
 * model space (normalised), are COPIED into context-owned tables on `stream` (device to device, asynchronous): rows with
 * fresh_host[b] != 0, or every row with fresh_host == NULL; the other rows keep what they hold (nothing, before their first upload).
 * gt_dev == keep_dev == NULL clears the table: the flag is dropped and the keep bytes are zeroed on `stream` (the buffers stay allocated), so
 * after a clear no row holds a kept region until it is uploaded again; exactly one of them NULL is MC_ERR_ARG.
 * While a table is set, the sampler update of mc_sample_rows takes, for an element with keep != 0,
 *     x0 = gt                                             (a select: gt where keep == 0 is never read into a result, a NaN included)
 *     mode 0: x_prev = the DDPM update of (x, x0)         mode 2: x_prev = the multistep update of (x, x0), history <- x0
 *     mode 1: x_prev = sqrt(ab_prev) gt + sqrt(1 - ab_prev) z2
 * with z2 = draw number draw_host[k][b] ^ 2^63 of the row's seed, at the row-local counter of the step draw: a row's kept-region noise
 * depends on its seed alone.  x0_dev, the history and the next step's pose-encoder operand receive the edited values; every other
 * element, and every element of a row whose keep bytes are all zero, gets the bits it gets without a table.  At schedule index 0 all
 * three samplers leave the kept region of x equal to gt bit for bit.  No cross-fade, no resampling jumps: mc_sample_step_inpaint.
 * State: with a captured graph or a seam table in the context, setting a table is MC_ERR_STATE.  While a table is set,
 * mc_ctx_set_seams, mc_ctx_graph_capture, mc_ctx_graph_step, mc_sample_step, mc_sample_loop, mc_sample_step_inpaint and
 * mc_sample_step_seeded return MC_ERR_STATE, and mc_sample_rows in mode 1 with noise_dev != NULL returns MC_ERR_ARG (modes 0 and 2
 * take either noise source).  Every refusal leaves the context as it was.  The table does not touch the multistep history flags, and
 * mc_ctx_set_condition / mc_ctx_set_condition_rows do not touch the table. */
int mc_ctx_set_edit_rows(mc_ctx* c, const float* gt_dev, const uint8_t* keep_dev, const uint8_t* fresh_host, void* stream);

/* Long requests among the rows: the windows of a request longer than T frames are request rows of
 * mc_sample_rows, coupled on their shared frames like the windows of mc_ctx_set_seams -- but per row: any rows of the batch, each
 * request at its own step and guidance scale, beside short requests.  Row b shows global frames [first_frame_host[b],
 * first_frame_host[b] + T) of its request; right_host[b] is the row that holds the request's NEXT window (any row, lower or higher
 * than b), or -1.  Windows overlap by `overlap` frames, 0 < 2 overlap <= T: the last `overlap` frames of row b are the first of row
 * right_host[b].  MC_ERR_ARG, the context unchanged: right[b] outside [-1, B) or == b; a row named by two rows; first_frame < 0 or
 * first_frame[right[b]] != first_frame[b] + T - overlap; a chain that does not end; a weight outside [0, 1]; overlap outside the range.
 * While a table is set, the sampler update of mc_sample_rows blends the two x0 predictions of a shared frame f,
 *     x0 = w[f] x0_right + (1 - w[f]) x0_left,     w = weight_host[overlap], or NULL: w[f] = (f + 1) / (overlap + 1),
 * computes the update once under the LEFT row's table entry and gives both rows the same x_prev / x0 / history; every other element
 * gets the bits it gets without a table.  The two rows of a seam must carry, in every tick of a call, the same step index, the same
 * coefficient bytes, the same draw number and the same history flag, and (noise_dev == NULL) the same seed: mc_sample_rows checks this
 * before its first launch (MC_ERR_ARG).
 * Noise with noise_dev == NULL, the request-global counter rule: element r of row b in draw d is element first_frame[b] * C + r of
 * mc_op_philox_normal(n, seed = seeds[b], draw = d) -- key seeds[b], counter ((first_frame[b] * C + r) / 4, d), 64-bit.  The two copies
 * of a shared frame draw the same normal by construction; a row with first_frame 0 draws what it draws without a table.  x_T of a long
 * request is draw 0 of that field gathered into its windows (the caller's part, as in mc_ctx_set_seams).  With noise_dev the owner
 * reads its own (the left row's) element.
 * The table lives in the context, is uploaded on `stream` (the call synchronises it) and is replaced as a whole by every call;
 * overlap == 0 clears it (the other arguments are ignored).  Setting or clearing touches no multistep history flag.
 * State: with a captured graph, an edit table or a seam table (mc_ctx_set_seams) in the context, setting a table is MC_ERR_STATE.
 * While a table is set, mc_ctx_set_seams, mc_ctx_set_edit_rows, mc_ctx_graph_capture, mc_ctx_graph_step, mc_sample_step,
 * mc_sample_loop, mc_sample_step_inpaint and mc_sample_step_seeded return MC_ERR_STATE.  Every refusal leaves the context as it was.
 * B * T * C < 2^31 and T * C >= 4. */
int mc_ctx_set_seam_rows(mc_ctx* c, int32_t overlap, const int32_t* right_host, const int32_t* first_frame_host, const float* weight_host,
                         void* stream);

/* Kept regions on long requests: one switch per context under which the edit table and the row seam table may
 * be set side by side.  Off (the default), each setter refuses the other's table exactly as described above.  On:
 * mc_ctx_set_edit_rows beside a row seam table and mc_ctx_set_seam_rows beside an edit table are accepted, and mc_sample_rows runs
 * with both set.  For an element of a window row the order is 4q's blend, then 4p's select:
 *     x0m = the CFG-combined prediction;   the seam's owner (the left row's tail element): x0m = w x0_right + (1 - w) x0m
 *     x0 = keep ? gt : x0m;   the update of mc_ctx_set_edit_rows on that x0 (mode 1: x_prev = sqrt(ab_prev) gt + sqrt(1 - ab_prev) z2)
 * and the owner stores x_prev, x0, the history and the next step's operand to both copies of a shared element.  The owner reads ITS
 * OWN keep / gt entry; the entry of the head copy (the right row's first `overlap` frames, where it has a left neighbour) is never
 * read into a result.  The tables arrive as device pointers, so the library cannot check that the two copies agree: the caller
 * uploads equal keep / gt for both copies of a shared frame (serve.ContinuousBatcher cuts both from one request-global edit).
 * The step noise is the request-global field of mc_ctx_set_seam_rows; z2 is the same field at draw number draw ^ 2^63, so both copies
 * of a shared frame have one z2 and a row at first_frame 0 draws what it draws under mc_ctx_set_edit_rows alone.
 * Still MC_ERR_STATE / MC_ERR_ARG with the switch on, the context unchanged: either setter beside a captured graph or the whole-batch
 * seam table of mc_ctx_set_seams; every entry without a rows form while a table is set; mc_sample_rows in mode 1 with noise_dev !=
 * NULL beside an edit table; the seam-pair checks of mc_sample_rows.  Switching off while both tables are set is MC_ERR_STATE.  The
 * switch touches no table and no multistep history flag. */
int mc_ctx_set_long_edits(mc_ctx* c, int32_t on);

/* hipGraph replay of mc_sample_step (BASELINE.json configs[4] "hipGraph-captured 50-step DDIM"): ONE graph serves every step
 * of the schedule -- the step index is a device-side integer, the FiLM tables and the sampler coefficients are addressed
 * with it inside the kernels, no host sync or per-step H2D copy (SURVEY.md section 3.1 lists the reference's per-step
 * host syncs).  capture: coefs_host[num_steps] = the mc_step_coefs of every schedule index (num_steps must equal the
 * schedule of mc_ctx_set_timesteps); x_dev [B,T,C] is updated IN PLACE by every replay, noise_dev [B,T,C] is read by
 * every replay (the caller refills it between steps); both pointers are baked into the graph.  `stream` must be a
 * non-default stream.  step: runs schedule index step_index on `stream` (bit-identical to mc_sample_step). */
int mc_ctx_graph_capture(mc_ctx* c, float* x_dev, const float* noise_dev, const mc_step_coefs* coefs_host, int32_t num_steps,
                         void* stream);
int mc_ctx_graph_step(mc_ctx* c, int32_t step_index, void* stream);
int mc_ctx_graph_release(mc_ctx* c);

/* mc_sample_step with the seeding above; x_t_dev is MODIFIED IN PLACE on the seeded elements (the reference writes
 * into `img`) before the denoiser and the sampler update read it */
int mc_sample_step_seeded(mc_ctx* c, float* x_t_dev, int32_t step_index, const mc_step_coefs* coefs,
                          const float* noise_dev, const mc_seed* seed, float* x_prev_dev, float* x0_dev, void* stream);

/* mc_sample_step with the kept region of x0 / of the new sample taken from gt (RePaint) */
int mc_sample_step_inpaint(mc_ctx* c, const float* x_t_dev, int32_t step_index, const mc_step_coefs* coefs,
                           const float* noise_dev, const mc_inpaint* inpaint, float* x_prev_dev, float* x0_dev,
                           void* stream);

/* ---- introspection for tests --------------------------------------------------------- */
/* named context buffers: "h","z","proj","mf","qkv","ys","yt","a" (fp32 rows; refused while a reduced-precision context keeps fp16
 * planes there),"a_tail" (the deferred last FiLM block's fp32 rows),"z2","out2","emb","ss","tf",
 * "idx","gate","comb_w","key","cap_idx","cap_w" (layer selects tf / ss / cap slices),
 * "src_row","dst_row" (ints, [2N]: expert slot -> token / -> 2 token + choice), "tile_group","tile_row0","tile_nrows" (ints,
 * [2][max_tiles]: the 128-row tile map of either slot group), "num_tiles" (2 ints: tiles of either slot group) -- of the last routing,
 * "x0_hist" (the multistep sampler's previous x0 [B,T,C]; MC_ERR_STATE before the context's first mode-2 call),
 * "route_split" (one int: the last routing call's twin-split flag, nonzero if a capacity cut separated a token from its CFG twin) */
int mc_ctx_get_buffer(mc_ctx* c, const char* name, int32_t layer, void** dev_ptr, int64_t* numel);

/* FLOP ledger for the per-kernel roofline (tools/kernel_roofline.py; off by default): while enabled, every launcher books the useful
 * multiply-add work (x 2) of each launch under its kernel's name.  mc_debug_flop_ledger(1) clears and starts, (0) stops;
 * mc_debug_flop_ledger_dump writes "kernel<TAB>calls<TAB>flops" lines into buf (truncated at cap) and returns the size needed. */
int mc_debug_flop_ledger(int32_t enable);
int64_t mc_debug_flop_ledger_dump(char* buf, int64_t cap);

/* op-level entry points (kernel parity tests call these through the same ABI) */
/* the activation an `act` argument or field names; LRELU: nn.LeakyReLU() slope 0.01; QUICKGELU: x sigmoid(1.702 x) (CLIP) */
enum { MC_ACT_NONE = 0, MC_ACT_GELU = 1, MC_ACT_SILU = 2, MC_ACT_LRELU = 3, MC_ACT_QUICKGELU = 4 };
int mc_op_gemm(const float* a_dev, const float* w_dev, const float* bias_dev, const float* res_dev,
               float* c_dev, int32_t M, int32_t N, int32_t K, int32_t ldw, int32_t act, void* stream);
/* C = A W^T + bias + res on the fp16 MFMA (split != 0: hi/lo three-product form); N % 128 == 0, K % 32 == 0; synchronises */
int mc_op_gemm_f16(const float* a_dev, const float* w_dev, const float* bias_dev, const float* res_dev, float* c_dev,
                   int32_t M, int32_t N, int32_t K, int32_t split, void* stream);
/* the same product from caller-built fp16 planes of A (the kernels a reduced-precision context feeds from film_rows_k's planes; tests):
 * a_hi / a_lo [M][K] halves, or fragment-major (frag_major != 0: half (((r >> 5) (K >> 4) + s) 64 + (r & 31) + 32 h) 8 + e holds column
 * 16 s + 8 h + e of row r); a_lo is read only when split != 0; W fp32, split here; pre != 0: the row-major kernel prefetches res.
 * N % 128 == 0, K % 64 == 0 (fragment-major: M % 32 == 0, K >= 192); synchronises */
int mc_op_gemm_f16_planes(const void* a_hi_dev, const void* a_lo_dev, const float* w_dev, const float* bias_dev, const float* res_dev,
                          float* c_dev, int32_t M, int32_t N, int32_t K, int32_t split, int32_t pre, int32_t frag_major, void* stream);
/* the folded decoder tail as one op (stmogen.py:505-544 + 757-760 after the CFG combination, motioncraft_amd/csrc/mc_gemm.hip):
 *   C[r] = (wc h[r] + wu h[r + M]) W[0]^T + (wc a[r] + wu a[r + M]) W[1]^T + bias[0] + bias[1]
 * h, a [2 M][K] (conditional rows, then the unconditional ones), W [2][N][K], bias [2][N], C [M][N]; c2_dev: scratch [M][N] (the
 * block-range form writes one partial product per K group, added here by a second launch and by the sampler-update kernel in the step;
 * may be NULL for variant 1); variant 0 = the default kernel choice, 1 = the column-tile form (gemm_tail_k), 2 = the block-range form
 * (gemm_tail2_k; N <= 336) */
int mc_op_gemm_tail(const float* h_dev, const float* a_dev, const float* w_dev, const float* bias_dev, float* c_dev, float* c2_dev,
                    int32_t M, int32_t N, int32_t K, float wc, float wu, int32_t variant, void* stream);
int mc_op_ln_rows(const float* x_dev, int64_t ldx, const float* gamma_dev, const float* beta_dev,
                  const float* add_dev, int32_t add_mod, float* y_dev, int64_t rows, int32_t L, void* stream);
/* The two MC-Attn cores as context-free ops (st_attention.py:105-179; the launchers the step calls, no other work).  Layouts, as in the step:
 *   mf   [2 B * T * H][4 L] motion rows = [body_value | key | value | query], row (b T + t) H + h.  The body op takes the row stride
 *        ldmf >= L and reads the body_value columns only (the step passes 4 L); the temporal op reads rows of exactly 4 L
 *   qkv  [frames * H][3 L] = [q | k | v] of the dynamic body topology;  wsm [H][H] = softmax(body_weight, dim 1), as the step passes it
 *   tf   [2 B][Nt][2 L] text rows = [key | value];  mask [B][T] (sample b of the CFG-doubled batch reads row b % B; samples b >= B are
 *        the unconditioned half: their text keys carry -1e6 and their text values are 0)
 *   ys / yt [rows][H * L], row = frame (b T + t)
 * mc_op_body_attention: ys[f] for the `frames` frames behind the four pointers: static mix + body_value + dynamic linear attention over the H
 *   parts in 8 heads (H = 8 or 12; L = 32, 64, 128).  split_flag_dev != NULL and *split_flag_dev == 0: frames with frame0 + f >= twin_from
 *   are the aliased CFG twins and are not produced (their ys rows stay untouched); NULL: no aliasing.
 * mc_op_temporal_attention: yt rows of samples [b0, b0 + nb) of the 2 B.  twin_flag_dev != NULL and *twin_flag_dev == 0: a sample b >= B
 *   reads the motion rows of sample b - B (its own were not produced).  skip_text != 0: the unconditioned half skips whole leading blocks
 *   of its text rows (same bits).  `form` names the kernel; a form that does not exist for the shape is MC_ERR_ARG, never another form:
 *   LSPLIT needs L >= 64, PAIR L == 64 and even H, the fp16 forms L >= 64. */
enum { MC_TEMPORAL_STEP = 0,      /* what the fp32 step would launch for nb samples under the process options (temporal_split, chain);
                                     a reduced-precision context would pick temporal_h_k above temporal_split: ask for F16X3 / F16 */
       MC_TEMPORAL_WHOLE = 1,     /* temporal_k<L, false>: one workgroup per (sample, part) */
       MC_TEMPORAL_LSPLIT = 2,    /* temporal_k<L, true>: 32-column slices, query chunks dealt over 2 workgroups while the grid stays <= 256 */
       MC_TEMPORAL_PAIR = 3,      /* temporal_k<64, false, true>: two parts per workgroup */
       MC_TEMPORAL_F16X3 = 4,     /* temporal_h_k<L, true>: fp16 MFMA, hi/lo three-product form */
       MC_TEMPORAL_F16 = 5 };     /* temporal_h_k<L, false>: plain fp16 operands */
int mc_op_body_attention(const float* mf_dev, int64_t ldmf, const float* qkv_dev, const float* wsm_dev, float* ys_dev, int64_t frames,
                         int32_t H, int32_t L, int64_t twin_from, const int32_t* split_flag_dev, int64_t frame0, void* stream);
int mc_op_temporal_attention(const float* mf_dev, const float* tf_dev, const float* mask_dev, float* yt_dev, int32_t b0, int32_t nb,
                             int32_t B, int32_t T, int32_t Nt, int32_t H, int32_t L, int32_t form, int32_t skip_text,
                             const int32_t* twin_flag_dev, void* stream);
/* The kernels of the step-invariant encoders as context-free ops (text, evaluation, BiGRU and wav encoders): each calls the launcher
 * its encoder calls, no other work.
 * mc_op_enc_ln: y = LayerNorm_L(x) gamma + beta over `rows` rows of L floats (L % 4 == 0, L <= 4096), relu != 0: max(., 0) on the way
 *   out; y == x is allowed.
 * mc_op_enc_embed_tokens: x[r][:] = emb[clamp(ids[r], 0, vocab - 1)][:] + pos[r % S][:], d % 4 == 0.
 * mc_op_enc_attention: softmax((q / 8) k^T) v per (sample, head) over qkv [B*S][3 d] = [q | k | v], head_dim 64 (d = 64 heads) -> out
 *   [B*S][d].  valid: uint8 [B][S], 0 = the key is not attended (NULL: all are); causal != 0: key j > query i is not attended either.
 *   A query left with no key gives a zero row.  `form` names the kernel; a form that does not exist for the arguments is MC_ERR_ARG,
 *   never another form: SMALL needs valid == NULL and S <= 128. */
enum { MC_ENC_ATTN_LAYER = 0,     /* what an encoder layer launches: SMALL where it exists, else STREAM */
       MC_ENC_ATTN_SMALL = 1,     /* mha_small_k: one workgroup per (sample, head), all keys in LDS */
       MC_ENC_ATTN_STREAM = 2 };  /* mha_masked_k: 16-query blocks, keys streamed 64 at a time with the running-max softmax */
int mc_op_enc_ln(const float* x_dev, const float* gamma_dev, const float* beta_dev, float* y_dev, int64_t rows, int32_t L, float eps,
                 int32_t relu, void* stream);
int mc_op_enc_embed_tokens(const int32_t* ids_dev, const float* emb_dev, const float* pos_dev, float* x_dev, int64_t rows, int32_t S,
                           int32_t d, int32_t vocab, void* stream);
int mc_op_enc_attention(const float* qkv_dev, const uint8_t* valid_dev, float* out_dev, int32_t B, int32_t S, int32_t d, int32_t heads,
                        int32_t causal, int32_t form, void* stream);
/* The grouped / strided forms of the fp32 MFMA GEMM, mode MC_GM_PLAIN or MC_GM_ENC (encoder: rows of any alignment, table, duplicate rows):
 *   C[g c_gstride + r ldc + n] = act(sum_k A[g a_gstride + r lda + k] W[g w_gstride + n ldw + k] + bias[g b_gstride + n]) + add[(r % add_mod)
 *   ld_add + n] + R[g r_gstride + r ldr + n]   (act_after_res != 0: R inside the activation), r < M, n < N, k < K, g < groups;
 * dup_rows != 0: row r + dup_rows of C receives the same values.  W rows are zero padded from K to the next multiple of 4 (ldw % 4 == 0);
 * MC_GM_PLAIN needs K, lda % 4 == 0; add / dup_rows are MC_GM_ENC only and need 16-byte aligned output rows.  r_gstride < 0: c_gstride. */
enum { MC_GM_PLAIN = 0, MC_GM_ENC = 4 };
typedef struct mc_gemm_strided {
    const float* a_dev; int64_t lda, a_gstride;
    const float* w_dev; int64_t ldw, w_gstride;
    const float* bias_dev; int64_t b_gstride;
    float* c_dev; int64_t ldc, c_gstride;
    const float* res_dev; int64_t ldr, r_gstride;
    const float* add_dev; int64_t ld_add, dup_rows;
    int32_t add_mod, act, act_after_res, M, N, K;
} mc_gemm_strided;
int mc_op_gemm_strided(int32_t mode, int32_t groups, const mc_gemm_strided* args, void* stream);
/* recurrence steps [s0, s0 + steps) of a bidirectional GRU on h [B][2][H] in place (direction 1 visits t = len - 1 - s): gi [2][B*S][3H]
 * = input products + b_ih (gate order r | z | n), whh [2][3H][H], bhh [2][3H]; sample b is updated at steps s < min(lens[b] / len_div, S).
 * H % 4 == 0; scratch is allocated here; synchronises */
int mc_op_bigru_steps(const float* gi_dev, const float* whh_dev, const float* bhh_dev, float* h_dev, const int32_t* lens_dev,
                      int32_t len_div, int32_t B, int32_t S, int32_t H, int32_t s0, int32_t steps, void* stream);
/* Conv1d(kernel 4, stride 2, padding 1) + LeakyReLU(slope) over channels-last frames x [B*T] rows of ldx floats (C used):
 * w_tapmajor [O][4][Cp] (element (o, tap, c) = weight[o][c][tap], zero for c >= C; Cp % 4 == 0), y_padded [B][T1 + 2][O] with
 * T1 = (T - 2) / 2 + 1 and rows 0 and T1 + 1 of every sample zero (the padded input of a next convolution); synchronises */
int mc_op_conv1d_k4s2(const float* x_dev, int64_t ldx, const float* w_tapmajor_dev, const float* bias_dev, float* y_padded_dev, int32_t B,
                      int32_t T, int32_t C, int32_t Cp, int32_t O, float slope, void* stream);
int mc_op_sampler_update(const float* x_t_dev, const float* out_text_dev, const float* out_none_dev,
                         const float* noise_dev, float* x_prev_dev, float* x0_dev, int64_t n,
                         const mc_step_coefs* coefs, void* stream);
/* the mode-2 update without a context: x0 = text_coef out_text + none_coef out_none;  x_prev = c2 x_t + c1 x0 + eta x0_hist;
 * x0_hist <- x0 (IN-OUT [n]; read only when eta != 0, so it may be uninitialised on a first step).  x_prev_dev may alias x_t_dev,
 * x0_dev may be NULL.  coefs->mode must be MC_SAMPLER_MULTISTEP. */
int mc_op_sampler_multistep(const float* x_t_dev, const float* out_text_dev, const float* out_none_dev, float* x0_hist_dev,
                            float* x_prev_dev, float* x0_dev, int64_t n, const mc_step_coefs* coefs, void* stream);
/* The per-row kernel forms of mc_sample_rows without a context (both synchronise; coefs_host [B] is one entry per request row).
 * mc_op_gemm_tail_rows: mc_op_gemm_tail with (wc, wu) of row r = coefs_host[r / T].{text_coef, none_coef}; M % T == 0, B = M / T.
 *   variant 1 = gemm_tail_k, 2 = gemm_tail2_k, 3 = the small-batch form (axpby_pair_rows_k, then the grouped 64 x 64 GEMM); c2_dev
 *   [M][N] scratch for variants 2 and 3.
 * mc_op_sampler_rows: the update of [B][TC] with element e under coefs_host[e / TC] (one mode for all rows), x0 = out_text + out_none
 *   (the two partial products of the folded tail).  Modes 0 / 1 read noise_dev; mode 2 has x0_hist_dev in-out (read where the row's
 *   eta != 0).  Operands that are not all 16-byte aligned take the element form of the kernel. */
int mc_op_gemm_tail_rows(const float* h_dev, const float* a_dev, const float* w_dev, const float* bias_dev, float* c_dev, float* c2_dev,
                         int32_t M, int32_t N, int32_t K, const mc_step_coefs* coefs_host, int32_t T, int32_t variant, void* stream);
int mc_op_sampler_rows(const float* x_t_dev, const float* out_text_dev, const float* out_none_dev, const float* noise_dev,
                       float* x0_hist_dev, float* x_prev_dev, float* x0_dev, int32_t B, int32_t TC, const mc_step_coefs* coefs_host,
                       void* stream);
/* mc_op_sampler_rows with a kept region (see mc_ctx_set_edit_rows): gt_dev [B][TC] floats, keep_dev [B][TC] bytes.  Modes 0 / 1 take
 * either noise_dev (and, mode 1, gt_noise_dev [B][TC]: the kept region's second normal), or seeds_host [B] + draw_host [B]: both
 * noises are then drawn in the kernel, row b from key seeds_host[b] at draws draw_host[b] and draw_host[b] ^ 2^63; the two sources
 * exclude each other.  Mode 2: x0_hist_dev in-out, no noise of either kind.  Mixed modes are MC_ERR_ARG.  Synchronises. */
int mc_op_sampler_edit_rows(const float* x_t_dev, const float* out_text_dev, const float* out_none_dev, const float* noise_dev,
                            const float* gt_noise_dev, const float* gt_dev, const uint8_t* keep_dev, const uint64_t* seeds_host,
                            const uint64_t* draw_host, float* x0_hist_dev, float* x_prev_dev, float* x0_dev, int32_t B, int32_t TC,
                            const mc_step_coefs* coefs_host, void* stream);
/* the seam-coupled update without a context (see mc_ctx_set_seams for the plan rules and the blend): operands [B, T, C], any mode.
 * Modes 0 / 1: the noise is read from noise_dev, or with noise_dev == NULL drawn from the Philox stream (seed, draw) -- mutually
 * exclusive: seed and draw must be 0 beside a noise tensor.  Mode 2: x0_hist_dev in-out as in mc_op_sampler_multistep (unused, may
 * be NULL, in the other modes), no noise.  x_prev_dev may alias x_t_dev, x0_dev may be NULL.  Synchronises. */
int mc_op_sampler_seam(const float* x_t_dev, const float* out_text_dev, const float* out_none_dev, const float* noise_dev, uint64_t seed,
                       uint64_t draw, float* x0_hist_dev, float* x_prev_dev, float* x0_dev, int32_t B, int32_t T, int32_t C,
                       int32_t overlap, const int32_t* first_frame_host, const float* weight_host, const mc_step_coefs* coefs,
                       void* stream);

/* the seam-coupled rows update without a context (sampler_seam_rows_k; see mc_ctx_set_seam_rows for the table rules, the blend and the
 * noise): operands [B, T, C], coefs_host [B] one entry per row (one mode for all rows; the two rows of a seam carry equal entries:
 * MC_ERR_ARG otherwise), x0 = out_text + out_none as in mc_op_sampler_rows.  Modes 0 / 1 take noise_dev, or seeds_host [B] +
 * draw_host [B] (drawn in the kernel; the two sources exclude each other, and the rows of a seam share seed and draw number).  Mode 2:
 * x0_hist_dev in-out (read where the row's eta != 0), no noise.  x_prev_dev may alias x_t_dev, x0_dev may be NULL.  Operands that are
 * not all 16-byte aligned take the element form of the kernel.  Synchronises. */
int mc_op_sampler_seam_rows(const float* x_t_dev, const float* out_text_dev, const float* out_none_dev, const float* noise_dev,
                            const uint64_t* seeds_host, const uint64_t* draw_host, float* x0_hist_dev, float* x_prev_dev, float* x0_dev,
                            int32_t B, int32_t T, int32_t C, int32_t overlap, const int32_t* right_host, const int32_t* first_frame_host,
                            const float* weight_host, const mc_step_coefs* coefs_host, void* stream);
/* mc_op_sampler_seam_rows with a kept region (sampler_seam_edit_rows_k; see mc_ctx_set_long_edits): gt_dev [B,T,C] floats, keep_dev
 * [B,T,C] bytes, and the noise sources of mc_op_sampler_edit_rows -- noise_dev (mode 1: with gt_noise_dev), or seeds_host + draw_host,
 * both noises then drawn from the request-global field at draws draw_host[b] and draw_host[b] ^ 2^63.  The keep / gt / gt_noise
 * entries of the head copy of a shared element are never read into a result.  Synchronises. */
int mc_op_sampler_seam_edit_rows(const float* x_t_dev, const float* out_text_dev, const float* out_none_dev, const float* noise_dev,
                                 const float* gt_noise_dev, const float* gt_dev, const uint8_t* keep_dev, const uint64_t* seeds_host,
                                 const uint64_t* draw_host, float* x0_hist_dev, float* x_prev_dev, float* x0_dev, int32_t B, int32_t T,
                                 int32_t C, int32_t overlap, const int32_t* right_host, const int32_t* first_frame_host,
                                 const float* weight_host, const mc_step_coefs* coefs_host, void* stream);

/* Result post-processing of the 322-d motion.  pred_dev [B,T,322] normalised; lengths_dev [B]
 * int32 valid frames (NULL = T); mean/std_dev [322] fp64; taps_dev [4][MC_POST_MAXTAP] fp64 = normalised Gaussian
 * taps of the 4 channel groups (body+jaw, hands, trans, expressions) centred at radius[g]; radius[g] < 0 leaves the
 * group unfiltered.  stats_f32 != 0 de-normalises in fp32 like numpy does with float32 mean/std files.
 * Outputs fp64: poses [B,T,165], expressions [B,T,100], trans [B,T,3]; frames >= length are 0. */
#define MC_POST_MAXTAP 129
int mc_postprocess_smplx(const float* pred_dev, const int32_t* lengths_dev, const double* mean_dev,
                         const double* std_dev, const double* taps_dev, const int32_t radius[4], int32_t stats_f32,
                         int32_t B, int32_t T, int32_t C, double* poses_dev, double* expr_dev, double* trans_dev,
                         void* stream);
/* The same over the STITCHED sequence the tools save when several --text / --motion_length intervals are given
 * (tools/visualize.py:216-246: the intervals' valid frames are concatenated FIRST, the Gaussian filter then runs over
 * the whole sequence, so smoothing crosses the seams).  rows_dev int32 [n_frames]: row (b*T + t) of pred_dev [*,322]
 * that stitched frame i shows; filter support is clamped to [0, n_frames).  Outputs [n_frames, 165|100|3] fp64. */
int mc_postprocess_smplx_stitched(const float* pred_dev, const int32_t* rows_dev, int32_t n_frames,
                                  const double* mean_dev, const double* std_dev, const double* taps_dev,
                                  const int32_t radius[4], int32_t stats_f32, int32_t C, double* poses_dev,
                                  double* expr_dev, double* trans_dev, void* stream);

/* Joint positions from the HumanML3D (263-d, 22 joints) / KIT (251-d, 21 joints) feature vector: what the sampling
 * tool saves as --pose_npy (tools/visualize.py:46-56 -> recover_from_ric, mogen/utils/plot_utils.py:40-104).
 * data = float(pred * std + mean); yaw[t] = sum_{s<t} data[s,0]; root xz = running sum of the yaw-rotated velocities
 * data[t-1,1:3], root y = data[t,3]; joint j >= 1 = yaw-rotated data[t, 4+3(j-1) : 4+3j] + root xz; then every
 * (joint, axis) track is filtered over time with the normalised Gaussian taps_dev [MC_POST_MAXTAP] fp64 centred at
 * `radius` (edge frames replicated; radius < 0: unfiltered, taps_dev may be NULL).  Arithmetic after the fp32 rounding
 * of `data` is fp64.  pred_dev [B,T,C] normalised, lengths_dev [B] int32 valid frames (NULL = T): each sample is a
 * sequence of its own; mean/std_dev [C] fp64, stats_f32 as above.  C must equal 4 + 9 (J-1) + 3 J + 4 for
 * J = joints_num >= 2, and T <= 1024.  joints_out_dev fp32 [B,T,J,3]; frames >= length are 0. */
int mc_postprocess_t2m_joints(const float* pred_dev, const int32_t* lengths_dev, const double* mean_dev,
                              const double* std_dev, const double* taps_dev, int32_t radius, int32_t stats_f32,
                              int32_t B, int32_t T, int32_t C, int32_t joints_num, float* joints_out_dev, void* stream);
/* The same over the STITCHED sequence of several intervals (tools/visualize.py:217-232): rows_dev as in
 * mc_postprocess_smplx_stitched; the yaw and root sums AND the filter run over all n_frames (any number), so the
 * motion carries across the seams.  work_dev: caller-owned scratch of 4 * n_frames doubles (per-frame root state).
 * joints_out_dev fp32 [n_frames,J,3]. */
int mc_postprocess_t2m_joints_stitched(const float* pred_dev, const int32_t* rows_dev, int32_t n_frames,
                                       const double* mean_dev, const double* std_dev, const double* taps_dev,
                                       int32_t radius, int32_t stats_f32, int32_t C, int32_t joints_num,
                                       double* work_dev, float* joints_out_dev, void* stream);

/* ---- text condition encoder (encode_text, diffusion_transformer.py:142-172); run once per prompt batch -------- */
typedef struct mc_textenc mc_textenc;
typedef struct mc_textenc_config {
    int32_t clip_dim;         /* 512: width of the CLIP text features                          */
    int32_t text_latent_dim;  /* text_encoder.latent_dim (256)                                 */
    int32_t num_layers;       /* text_encoder.num_layers (2) of nn.TransformerEncoder          */
    int32_t ff_size;          /* text_encoder.ff_size (2048)                                   */
    int32_t num_heads;        /* text_encoder.num_heads (4); head_dim must be 64               */
    int32_t max_len;          /* 77 tokens                                                     */
    int32_t clip_layers;      /* 12 (0: the CLIP tower is not used, clip_feat is an input)     */
    int32_t clip_heads;       /* 8                                                             */
    int32_t clip_ff;          /* 2048                                                          */
    int32_t vocab;            /* 49408                                                         */
} mc_textenc_config;
int mc_textenc_create(const mc_textenc_config* cfg, mc_textenc** out);
void mc_textenc_destroy(mc_textenc* e);
/* fp32 parameters from host memory under the reference's own state-dict keys (relative to the denoiser):
 * "text_pre_proj.weight/bias", "textTransEncoder.layers.{i}.{self_attn.in_proj_weight,...}", "text_ln.weight/bias",
 * and optionally "clip.token_embedding.weight", "clip.positional_embedding", "clip.transformer.resblocks.{i}.*",
 * "clip.ln_final.*" */
int mc_textenc_set_param(mc_textenc* e, const char* name, const float* host, int64_t numel);
int mc_textenc_finalize(mc_textenc* e);
/* clip_feat_dev [B, max_len, clip_dim] -> xf_out_dev [B, max_len, text_latent_dim]  (encode_text with clip_feat given) */
int mc_textenc_forward_feat(mc_textenc* e, const float* clip_feat_dev, int32_t B, float* xf_out_dev, void* stream);
/* tokens_dev int32 [B, max_len] (clip.tokenize ids) -> xf_out_dev; clip_feat_out_dev may be NULL */
int mc_textenc_forward_tokens(mc_textenc* e, const int32_t* tokens_dev, int32_t B, float* clip_feat_out_dev,
                              float* xf_out_dev, void* stream);

/* ---- Evaluation embedding model (T2MContrastiveModel_SMPLX; mogen/models/rnns/t2m_bigru_smplx.py:396-437) --------
 * motion side: ActorAgnosticEncoder (:66-195); text side: DistilbertActorAgnosticEncoder after tokenisation (:198-394).
 * The embeddings feed FID / R-precision / matching score / diversity / multimodality (mogen/core/evaluation/). */
typedef struct mc_evalenc mc_evalenc;
typedef struct mc_evalenc_config {
    int32_t nfeats;           /* motion_encoder.nfeats (322)                                                  */
    int32_t latent_dim;       /* 256                                                                          */
    int32_t ff_size;          /* 1024                                                                         */
    int32_t num_layers;       /* 4 layers of nn.TransformerEncoder (post-LN, GELU)                            */
    int32_t num_heads;        /* 4; head_dim must be 64                                                       */
    int32_t pe_len;           /* rows of sequence_pos_encoding.pe (5000)                                      */
    int32_t bert_dim;         /* DistilBERT hidden size (768); 0 = motion side only                           */
    int32_t bert_layers;      /* 6                                                                            */
    int32_t bert_heads;       /* 12; head_dim must be 64                                                      */
    int32_t bert_ff;          /* 3072                                                                         */
    int32_t bert_vocab;       /* 30522                                                                        */
    int32_t bert_max_pos;     /* 512                                                                          */
} mc_evalenc_config;
int mc_evalenc_create(const mc_evalenc_config* cfg, mc_evalenc** out);
void mc_evalenc_destroy(mc_evalenc* e);
/* fp32 parameters from host memory under the evaluator checkpoint's own keys ("motionencoder.skel_embedding.weight",
 * "motionencoder.mu_token", "motionencoder.sequence_pos_encoding.pe", "motionencoder.seqTransEncoder.layers.{i}.*",
 * "textencoder.text_model.embeddings.*", "textencoder.text_model.transformer.layer.{i}.*", "textencoder.projection.1.*",
 * "textencoder.mu_token", ... as split by load_pretrained, t2m_bigru_smplx.py:417-435) */
int mc_evalenc_set_param(mc_evalenc* e, const char* name, const float* host, int64_t numel);
int mc_evalenc_finalize(mc_evalenc* e);
/* encode_motion(motion, motion_length).loc: motion_dev [B, T, nfeats], lengths_dev int32 [B] -> mu_out_dev [B, latent_dim] */
int mc_evalenc_encode_motion(mc_evalenc* e, const float* motion_dev, const int32_t* lengths_dev, int32_t B, int32_t T,
                             float* mu_out_dev, void* stream);
/* encode_text(...).loc after the tokenizer: ids_dev int32 [B, S], mask_dev uint8 [B, S] (attention_mask) -> mu_out_dev */
int mc_evalenc_encode_text(mc_evalenc* e, const int32_t* ids_dev, const uint8_t* mask_dev, int32_t B, int32_t S,
                           float* mu_out_dev, void* stream);

/* ---- HumanML3D / KIT evaluation embedding model (T2MContrastiveModel; mogen/models/rnns/t2m_bigru.py:284-299) --------
 * motion side: T2MMotionEncoder = MovementConvEncoder + MotionEncoderBiGRUCo (:72-110, :226-282); text side:
 * TextEncoderBiGRUCo on word vectors + part-of-speech one-hots (:186-223; the GloVe lookup stays with the dataset). */
typedef struct mc_t2meval mc_t2meval;
typedef struct mc_t2meval_config {
    int32_t input_size;       /* motion_encoder.input_size (263 / 251); the last 4 channels are dropped            */
    int32_t movement_hidden;  /* 512                                                                               */
    int32_t movement_latent;  /* 512                                                                               */
    int32_t motion_hidden;    /* 1024                                                                              */
    int32_t motion_latent;    /* 512                                                                               */
    int32_t word_size;        /* 300; 0 = motion side only                                                         */
    int32_t pos_size;         /* 15                                                                                */
    int32_t text_hidden;      /* 512                                                                               */
    int32_t text_out;         /* 512                                                                               */
} mc_t2meval_config;
int mc_t2meval_create(const mc_t2meval_config* cfg, mc_t2meval** out);
void mc_t2meval_destroy(mc_t2meval* e);
/* fp32 parameters from host memory: the checkpoint's three state dicts flattened with their names as prefixes
 * ("movement_encoder.main.0.weight" [O, C, 4] as stored, "motion_encoder.gru.weight_ih_l0_reverse", "text_encoder.hidden", ...) */
int mc_t2meval_set_param(mc_t2meval* e, const char* name, const float* host, int64_t numel);
int mc_t2meval_finalize(mc_t2meval* e);
/* motion_dev [B, T, input_size], lengths_dev int32 [B] (frames, >= 4) -> out_dev [B, motion_latent] */
int mc_t2meval_encode_motion(mc_t2meval* e, const float* motion_dev, const int32_t* lengths_dev, int32_t B, int32_t T,
                             float* out_dev, void* stream);
/* word_emb_dev [B, S, word_size], pos_onehot_dev [B, S, pos_size], sent_len_dev int32 [B] (>= 1) -> out_dev [B, text_out] */
int mc_t2meval_encode_text(mc_t2meval* e, const float* word_emb_dev, const float* pos_onehot_dev, const int32_t* sent_len_dev,
                           int32_t B, int32_t S, float* out_dev, void* stream);

/* ---- WavEncoder: step-invariant audio condition encoder of the speech-to-gesture configs ------------------ */
typedef struct mc_wavenc mc_wavenc;
int mc_wavenc_create(int32_t audio_in, int32_t out_dim, mc_wavenc** out);
void mc_wavenc_destroy(mc_wavenc* e);
/* BatchNorm-folded, tap-major conv weights from host memory: "b{i}.conv1.w" [planes][ceil4(15*cin)], "b{i}.conv1.b",
 * "b{i}.conv2.w" [planes][15*planes], "b{i}.conv2.b", "b{i}.down.w", "b{i}.down.b" (blocks 0,1,3,5), i = 0..5 */
int mc_wavenc_set_param(mc_wavenc* e, const char* name, const float* host, int64_t numel);
int mc_wavenc_finalize(mc_wavenc* e);
int mc_wavenc_out_len(const mc_wavenc* e, int32_t samples, int32_t* frames);
/* wav_dev [B, samples, audio_in] -> out_dev [B, frames, out_dim] (channels-last, like WavEncoder.forward's return) */
int mc_wavenc_forward(mc_wavenc* e, const float* wav_dev, int32_t B, int32_t samples, float* out_dev, void* stream);

/* ---- SMPL-X body model: linear blend skinning of the published model (what smplx.lbs.lbs computes), fed from what
 * mc_postprocess_smplx leaves on the device (tools/s2g_test.py:76-85,364-412; tools/visualize.py:71-86).  Per frame:
 * R_j = rodrigues(theta_j) with the angle taken as |theta_j + 1e-8|; v_shaped = v_template + shapedirs [beta; psi];
 * J = J_regressor v_shaped; v_posed = v_shaped + posedirs^T vec(R_1..54 - I); G_0 = [R_0 | J_0], G_j = G_parent
 * [R_j | J_j - J_parent], A_j = G_j [I | -J_j]; joints_j = G_j[:3,3] + transl; verts_v = (sum_j W[v,j] A_j) [v_posed_v; 1]
 * + transl.  Only the 55 kinematic joints are produced (tools/s2g_test.py:406 keeps [:55*3]).  This is lbs() itself: the
 * package's forward adds the model file's mean hand pose to theta first unless flat_hand_mean is set (the reference
 * leaves it unset); a caller who wants that adds it to poses_dev (body_model.SMPLXBodyModel does, from hands_meanl/r). */
typedef struct mc_smplx mc_smplx;
typedef struct mc_smplx_config {
    int32_t num_vertices;     /* 10475 for the published model                                                     */
    int32_t num_joints;       /* 55                                                                                */
    int32_t num_betas;        /* 1..300 shape coefficients in use                                                  */
    int32_t num_expr;         /* 1..100 expression coefficients in use                                             */
    int32_t num_pose_feats;   /* 486 = 9 * 54                                                                      */
} mc_smplx_config;
int mc_smplx_create(const mc_smplx_config* cfg, mc_smplx** out);
void mc_smplx_destroy(mc_smplx* m);
/* fp32 parameters from host memory, as the model file stores them: "v_template" [V,3], "shapedirs" [V,3,num_betas],
 * "expr_dirs" [V,3,num_expr], "posedirs" [V,3,486], "J_regressor" [55,V], "weights" [V,55], "parents" [55]
 * (kintree_table[0] as floats; entry 0 is ignored) */
int mc_smplx_set_param(mc_smplx* m, const char* name, const float* host, int64_t numel);
/* MC_ERR_ARG for a tree with parents[j] >= j (j > 0).  Folds the
 * regressor into J0 = J_regressor v_template and Jdirs = J_regressor [shapedirs | expr_dirs] in fp64, compacts the skin
 * weights to their nonzeros, builds the level table of the tree and the K-contiguous blend-shape weight of the GEMM. */
int mc_smplx_finalize(mc_smplx* m);
/* poses_dev fp64 [n,165] (global 0:3, body 3:66, jaw 66:69, leye 69:72, reye 72:75, left hand 75:120, right hand
 * 120:165), expr_dev fp64 [n,num_expr] or NULL (zeros), trans_dev fp64 [n,3] or NULL (zeros), betas_dev fp64 [num_betas]
 * (betas_per_frame = 0) or [n,num_betas] -> joints_out_dev fp32 [n,55,3].  One kernel, fp64 arithmetic with one
 * rounding at the fp32 store. */
int mc_smplx_joints(mc_smplx* m, const double* poses_dev, const double* expr_dev, const double* trans_dev,
                    const double* betas_dev, int32_t betas_per_frame, int32_t n, float* joints_out_dev, void* stream);
/* bytes of workspace with which mc_smplx_vertices runs n_frames frames as one chunk (-1: bad argument) */
int64_t mc_smplx_work_bytes(const mc_smplx* m, int32_t n_frames, int32_t betas_per_frame);
/* The same inputs -> verts_out_dev fp32 [n,V,3] (16-byte aligned) and, if not NULL, joints_out_dev fp32 [n,55,3] (bit for
 * bit what mc_smplx_joints writes: the same kernel also produces the skinning transforms).  fp32 like the package: blend
 * shapes on the fp32 MFMA GEMM, then the skinning kernel.  Frames run in chunks of as many as work_dev (16-byte aligned,
 * work_bytes >= mc_smplx_work_bytes(m, 1, .)) holds; the result does not depend on the chunk size. */
int mc_smplx_vertices(mc_smplx* m, const double* poses_dev, const double* expr_dev, const double* trans_dev,
                      const double* betas_dev, int32_t betas_per_frame, int32_t n, void* work_dev, int64_t work_bytes,
                      float* verts_out_dev, float* joints_out_dev, void* stream);
/* The two sums behind the face errors of tools/s2g_test.py:407-412 (reclatent_loss = MSELoss, vel_loss = L1Loss, :99-100) with
 * the vertices never leaving the device: the vertex path above runs for pose set a (the sample) and pose set b (the target),
 * both with betas_dev, chunk by chunk, and sums_out_dev fp64 [2] receives
 *   [0] sum over n V 3 of (a - b)^2          [1] sum over (n - 1) V 3 of |(a[t+1] - b[t]) - (b[t+1] - b[t])|
 * with fp32 element operations (the reference's tensors) and fp64 sums: one partial per frame, then one fixed-order pass over
 * the frames, so the sums do not depend on work_bytes and two runs give the same bits.  The caller divides ([1] is 0 for n < 2).
 * work_dev: 16-byte aligned, work_bytes >= mc_smplx_vertex_errors_work_bytes(m, 1, n, .); that function gives the bytes with
 * which the n frames run in chunks of chunk_frames (-1: bad argument). */
int64_t mc_smplx_vertex_errors_work_bytes(const mc_smplx* m, int32_t chunk_frames, int32_t n_frames, int32_t betas_per_frame);
int mc_smplx_vertex_errors(mc_smplx* m, const double* poses_a_dev, const double* expr_a_dev, const double* trans_a_dev,
                           const double* poses_b_dev, const double* expr_b_dev, const double* trans_b_dev, const double* betas_dev,
                           int32_t betas_per_frame, int32_t n, void* work_dev, int64_t work_bytes, double* sums_out_dev, void* stream);

/* ---- Beat alignment of the speech-to-gesture test (alignment.load_pose + alignment.calculate_align,
 * mogen/datasets/EMAGE_2024/utils/metric.py:78-127,199-242; called at tools/s2g_test.py:418-422 on the 55 joints of
 * mc_smplx_joints).  The onset times are an input; mc_onset_strength / mc_onset_pick below produce them from the waveform.
 * mc_beat_mask: joints_dev fp32 [n_frames, num_joints, 3] (n_frames >= 2), mean_vel_dev fp64 [num_joints] ->
 * mask_out_dev uint8 [num_joints, t_end - t_start].  speed = |velocity| / mean_vel with forward / central / backward
 * differences in fp32 (dt = 1 / pose_fps rounded to fp32, sqrt((x x + y y) + z z), no fused multiply-add: numpy on fp32 joints),
 * the division in fp32 when mean_vel_fp32 is set (the values are then fp32 numbers held as doubles) and in fp64 otherwise.
 * Over s = speed[t_start:t_end, j], index i is a beat iff s[i] < s[clip(i +- k, 0, n - 1)] for every k = 1..order (1..MC_BEAT_MAX_ORDER;
 * scipy.signal.argrelextrema(np.less, mode='clip')) and speed[i, j] > threshold, where i is slice-relative but looked up in the
 * unsliced array, like metric.py:113-123. */
#define MC_BEAT_MAX_ORDER 64
#define MC_BEAT_MAX_UPPER 64
int mc_beat_mask(const float* joints_dev, int32_t n_frames, int32_t num_joints, const double* mean_vel_dev, int32_t mean_vel_fp32,
                 int32_t t_start, int32_t t_end, double pose_fps, int32_t order, double threshold, uint8_t* mask_out_dev, void* stream);
/* bytes of workspace of mc_beat_align (-1: bad argument) */
int64_t mc_beat_align_work_bytes(int32_t n_slice, int32_t n_upper);
/* mask_dev [num_joints, n_slice] as written by mc_beat_mask, upper_body_host: n_upper (1..MC_BEAT_MAX_UPPER) joint indices in HOST memory,
 * onsets_dev fp64 [n_onsets] seconds (n_onsets >= 1) -> score_out_dev fp64 [1]: the mean over the upper-body joints of the mean
 * over onsets of exp(-d^2 / (2 sigma^2)), d = |onset - nearest beat time i / pose_fps| (GAHR, metric.py:204-216); a joint
 * without beats contributes 0.  Fixed-order fp64 sums, no atomics: two runs give the same bits.  work_dev 8-byte aligned. */
int mc_beat_align(const uint8_t* mask_dev, int32_t num_joints, int32_t n_slice, const int32_t* upper_body_host, int32_t n_upper,
                  const double* onsets_dev, int32_t n_onsets, double pose_fps, double sigma, void* work_dev, int64_t work_bytes,
                  double* score_out_dev, void* stream);

/* ---- Audio onset detection (alignment.load_audio, metric.py:64-76: librosa 0.10.1's onset.onset_detect with its defaults,
 * restated in tests/onset_ref.py).  n_fft is MC_ONSET_N_FFT; hop a multiple of 4 in 4..MC_ONSET_MAX_HOP; n_mels 1..MC_ONSET_MAX_MELS; at most
 * 2^20 frames.
 * mc_onset_strength: wave_dev fp32 [n_samples] (finite) -> env_out_dev fp32 [F], F = 1 + n_samples / hop, the UN-normalised
 * onset envelope: frames centred on f hop with zeros outside the clip, power spectrum, mel projection, 10 log10(max(1e-10, .)),
 * the clamp at (maximum over the whole spectrogram) - 80, then env[j] = mean over the mel rows of max(0, S[j-lag+1] - S[j-lag]),
 * lag = 1 + n_fft / (2 hop), and env[j] = 0 for j < lag.
 *   dft_dev fp32 [n_fft, 2 (n_fft/2 + 1)]: column 2b = w[k] cos(2 pi k b / n_fft), column 2b + 1 = -w[k] sin(2 pi k b / n_fft),
 *           w the analysis window (periodic Hann for librosa's default);
 *   mel_dev fp32 [n_mels, n_fft/2 + 1]: the mel filter bank, row-major as librosa stores it.
 * work_dev: 16-byte aligned, work_bytes >= mc_onset_work_bytes(...) (-1: bad argument).  No atomics: two runs give the same bits.
 * mc_onset_pick: env_dev fp32 [n_frames] -> mask_out_dev uint8 [n_frames] (1 = onset), count_out_dev int32 [1].  With
 * `normalize` the envelope is first taken to (env - min) / (max - min + DBL_MIN) in fp64, and an all-zero one has no onsets.
 * Frame n is an onset iff env[n] >= every value of [n - pre_max, n + post_max), env[n] >= the mean of [n - pre_avg, n + post_avg)
 * + delta, env[n] > 0 and n > the last accepted onset + wait, left to right; the windows are truncated at both ends of the array
 * (librosa.util.peak_pick; post_max and post_avg count the frame itself, so they are >= 1). */
#define MC_ONSET_N_FFT 2048
#define MC_ONSET_MAX_HOP 512
#define MC_ONSET_MAX_MELS 128
int64_t mc_onset_work_bytes(int64_t n_samples, int32_t n_fft, int32_t hop, int32_t n_mels);
int mc_onset_strength(const float* wave_dev, int64_t n_samples, const float* dft_dev, const float* mel_dev, int32_t n_fft, int32_t hop,
                      int32_t n_mels, void* work_dev, int64_t work_bytes, float* env_out_dev, void* stream);
int mc_onset_pick(const float* env_dev, int32_t n_frames, int32_t pre_max, int32_t post_max, int32_t pre_avg, int32_t post_avg, double delta,
                  int32_t wait, int32_t normalize, uint8_t* mask_out_dev, int32_t* count_out_dev, void* stream);

/* ---- The audio condition of the speech-to-gesture configs (audio_rep `onset+amplitude`, beat_motionx.py:398-412; restated in
 * tests/audio_cond_ref.py): wave_dev fp32 [n_samples] -> out_dev fp32 [n_samples, 2], what mc_wavenc_forward reads with audio_in = 2.
 *   out[i][0] = max |wave[s .. s + window - 1]|, s = min(i, n_samples - window): the rolling maximum over the full windows; the last
 *               window's value is repeated over the final window - 1 samples (the reference pads with it), the window never shrinks
 *   out[i][1] = 1 if i < n_frames and onset_mask_dev[i], else 0: onset_mask_dev uint8 [n_frames] is the mask mc_onset_pick writes, one
 *               byte per onset FRAME, and the reference writes those frame indices into this sample-indexed column as they are
 *               (onset_array[audio_onset_f] = 1.0) -- kept.  onset_mask_dev may be NULL: a column of zeros.
 * window 1..MC_AUDIO_COND_MAX_WINDOW (the reference: 1024) and <= n_samples; n_frames <= n_samples.  One launch, a workgroup per
 * MC_AUDIO_COND_TILE output samples, no workspace, no atomics; a maximum of magnitudes has no rounding, so the result is exact and two runs
 * give the same bits. */
#define MC_AUDIO_COND_MAX_WINDOW 1024
#define MC_AUDIO_COND_TILE 4096
int mc_audio_condition(const float* wave_dev, int64_t n_samples, int32_t window, const uint8_t* onset_mask_dev, int32_t n_frames,
                       float* out_dev, void* stream);

/* ---- From a PCM wav file's bytes to the waveform the two blocks above read: what the reference does on the host with librosa.load
 * (libsndfile decode, librosa.to_mono, resample to 22 050 Hz) + librosa.resample(target_sr = 16000), beat_sep_lower.py:392-393 and
 * s2g_test.py:416-417.  The resampler is librosa's res_type = 'polyphase', which is scipy.signal.resample_poly(y, up, down) with zero
 * padding, restated in tests/resample_ref.py and pinned to scipy itself.  It is NOT librosa's default soxr_hq, whose parity stays
 * unpinned: a condition built this way differs from the reference's above roughly 0.9 of the Nyquist rate.
 * mc_pcm_decode: pcm_dev = the file's data chunk as uploaded, n_frames * channels * sample_bytes bytes of interleaved little-endian
 * PCM; sample_bytes 1 (unsigned, offset 128), 2, 3 or 4 (signed).  out_dev fp32 [n_frames]:
 *   mono != 0  out[i] = fp32((sum over the channels of the integer value, in fp64) / channels / 2^(8 sample_bytes - 1)): the sum and
 *              the power of two are exact, so the quotient and the conversion are the only roundings, and for 1, 2 and 4 channels
 *              the conversion alone.  For 16-bit input this equals libsndfile's float32 read followed by librosa.to_mono; for the
 *              other widths it is this project's definition (libsndfile scales them the same way but was not compared);
 *   mono == 0  out[i] = fp32(value of channel 0 / 2^(8 sample_bytes - 1)), for 16 bits what speech.read_wav returns.
 * channels 1..1024; out_dev 4-byte aligned.
 * mc_resample_out_len: ceil(n_in * up / down), the length scipy and librosa give; -1 for n_in < 0, up < 1, down < 1 or a length
 * whose indices would leave int64.
 * mc_resample_poly: x_dev fp32 [n_in] -> y_dev fp32 [n_out], n_out = mc_resample_out_len(n_in, up, down), gcd(up, down) = 1:
 *   y[m] = fp32(sum over k of x[k] * taps[half + m*down - k*up]),  0 <= k < n_in,  0 <= half + m*down - k*up < n_taps,
 * taps the fp64 filter ALREADY multiplied by `up`, n_taps odd, half = (n_taps - 1) / 2.  taps_dev holds them phase-major and reversed:
 * fp64 [up][L], L = ceil(n_taps / up), taps_dev[p * L + i] = taps[p + (L - 1 - i) * up], and 0 where that index is >= n_taps
 * (audio.phase_major builds it), so that an output walks its inputs and its taps in ascending order.  Products and the sum are fp64,
 * added in ascending k whatever the tiling, and rounded to fp32 once.  One launch, no workspace, no atomics: two runs give the same
 * bits.  All sample indices are 64-bit.  A tile of MC_RESAMPLE_TILE outputs must read at most 16384 inputs ((511 down + n_taps - 1) / up + 2): with
 * the default filter of 20 max(up, down) + 1 taps that holds for down / up <= 30; resample in two steps beyond. */
#define MC_RESAMPLE_TILE 512
int mc_pcm_decode(const uint8_t* pcm_dev, int64_t n_frames, int32_t channels, int32_t sample_bytes, int32_t mono, float* out_dev, void* stream);
int64_t mc_resample_out_len(int64_t n_in, int32_t up, int32_t down);
int mc_resample_poly(const float* x_dev, int64_t n_in, int32_t up, int32_t down, const double* taps_dev, int32_t n_taps, float* y_dev,
                     int64_t n_out, void* stream);

/* ---- Orthographic rasteriser: the vertices mc_smplx_vertices writes -> frames, the last step of the reference's tools
 * (mogen/datasets/EMAGE_2024/utils/fast_render.py:13-81 builds the scene -- a grey mesh, OrthographicCamera(xmag = ymag = 1), one
 * DirectionalLight -- and other_tools.py:695-765 feeds it; there pyrender + osmesa draw it in eight host processes).  The geometry below
 * is restated exactly in tests/raster_ref.py.  The colours are THIS project's shading model: pyrender's were not available to pin.
 *   project   screen_x = S[0] . (p, 1), screen_y = S[1] . (p, 1) in pixels (row 0 on top), zcam = S[2] . (p, 1), the distance along
 *             the view direction, S the fp32 3x4 world-to-screen affine, all fp32 fma; snapped to 8 sub-pixel bits,
 *             X = floor(256 screen_x + 0.5) as int32 (INT32_MIN when that is not finite or beyond the guard band).
 *             n_v = normalise(sum over the vertex's adjacency list, in list order, of cross(p1 - p0, p2 - p0)): area weighted,
 *             fp32, no atomics; a vertex without faces has the normal 0.
 *   raster    per triangle, with P = (256 x + 128, 256 y + 128) the centre of pixel (x, y) and E_ab(P) = (bx - ax)(Py - ay) -
 *             (by - ay)(Px - ax) in int64: w0 = E_12, w1 = E_20, w2 = E_01, area = w0 + w1 + w2.  area < 0 is counter-clockwise
 *             with y up = front; area == 0, and area > 0 under cull_backfaces, are dropped, and so is a triangle with a vertex whose
 *             zcam is not finite or whose snapped coordinate lies outside +-MC_RENDER_MAX_SIZE px (every product then fits int64).  A sample is
 *             covered when the three w have the sign of area or are 0 on a top or left edge (top-left fill rule), over the bounding
 *             box clamped to the viewport.  b1 = float(w1) / float(area), b2 = float(w2) / float(area),
 *             z = fmaf(b2, z2 - z0, fmaf(b1, z1 - z0, z0)); a sample with z outside [znear, zfar] is discarded.  The visible face of
 *             a pixel is the minimum of (bits of z) << 32 | face over its samples, by a 64-bit integer atomic minimum: the nearest
 *             sample, the lower face id at equal depth, whatever the order of arrival.  A triangle whose clamped box holds more than
 *             large_threshold pixels is walked by large_slices waves instead of one thread; the result is the same.
 *   shade     per pixel: background, or b0 = 1 - b1 - b2 and n = normalise(b0 n_0 + b1 n_1 + b2 n_2) (0 when the sum is 0),
 *             c = min(1, base (ambient + gain max(0, n . light))) per channel, u8 = (int)(255 c + 0.5).  A back face drawn with
 *             culling off keeps its outward normal.  depth is z of the winning sample (+inf on the background), face its id (-1).
 * Frames run in chunks of as many as work_dev holds; the result does not depend on the chunk size and two runs give the same bits.
 * work_dev: 16-byte aligned, at least the bytes mc_render_work_bytes gives for one frame (-1: bad argument).  Its head (a list
 * counter and the visibility keys of every frame it holds) must be 0 / all-ones when the kernels start; every call leaves it so.  With
 * work_clean = 0 the call fills it first; a caller that hands back the buffer of an earlier, successful call of the same width and
 * height, untouched since, may pass work_clean = 1 and skip the fill. */
#define MC_RENDER_MAX_SIZE 16384
#define MC_RENDER_MAX_SLICES 1024
typedef struct mc_render mc_render;
typedef struct mc_render_params {
    float screen[12];         /* S, row-major 3x4 (render.OrthographicCamera.screen_affine)                                 */
    float light[3];           /* unit vector towards the light, world space                                                 */
    float base[3];            /* mesh colour, 0..1                                                                          */
    float ambient, gain;      /* gain = intensity / pi: a unit-albedo Lambert surface                                       */
    float znear, zfar;        /* 0 < znear <= zfar                                                                          */
    int32_t background[3];    /* 0..255                                                                                     */
    int32_t width, height;    /* 1..MC_RENDER_MAX_SIZE                                                                      */
    int32_t cull_backfaces;
    int32_t large_threshold;  /* 0 = the default (1024); 1 sends every multi-pixel box to the wave path, INT32_MAX none      */
    int32_t large_slices;     /* waves that share one triangle of the wave path: 0 = the default (32), at most MC_RENDER_MAX_SLICES */
} mc_render_params;
/* faces_host int32 [num_faces,3]; the vertex-to-face adjacency in CSR form, adj_start_host int32 [num_vertices + 1] and
 * adj_faces_host int32 [adj_start[num_vertices]], the faces of each vertex in ascending order (all three checked here) */
int mc_render_create(const int32_t* faces_host, int32_t num_faces, int32_t num_vertices, const int32_t* adj_start_host,
                     const int32_t* adj_faces_host, mc_render** out);
void mc_render_destroy(mc_render* r);
int64_t mc_render_work_bytes(const mc_render* r, int32_t n_frames, int32_t width, int32_t height);
/* verts_dev fp32 [n,V,3] -> rgb_out_dev uint8 [n,H,W,3] (4-byte aligned) and, where not NULL, face_out_dev int32 [n,H,W],
 * depth_out_dev fp32 [n,H,W], screen_out_dev int32 [n,V,2], zcam_out_dev fp32 [n,V] */
int mc_render_frames(mc_render* r, const float* verts_dev, int32_t n, const mc_render_params* p, void* work_dev, int64_t work_bytes,
                     int32_t work_clean, uint8_t* rgb_out_dev, int32_t* face_out_dev, float* depth_out_dev, int32_t* screen_out_dev,
                     float* zcam_out_dev, void* stream);

/* ---- Capsule rasteriser: the joints mc_postprocess_t2m_joints* writes -> the skeleton animation the reference's text-to-motion tool
 * ends with (plot_3d_motion, mogen/utils/plot_utils.py:107-204: matplotlib's mplot3d on the host).  The scene (ground quad, root
 * trail, kinematic chains; a pixel's layer is the maximum layer that covers it, there is no depth test), the projection (fp32 fma,
 * correctly rounded division, 4 sub-pixel bits, a guard band of 8192 px), the exact int64 capsule rule and the triangle rule are
 * defined in the header comment of csrc/mc_skeleton.hip and restated in tests/skeleton_ref.py.  Not drawn: the title, anti-aliasing
 * and mplot3d's projecting caps; pixel parity with matplotlib's Agg output is not claimed.
 * Layers: 0 background, 1 plane, 2 trail, 3 + c chain c.  Frames run in chunks of as many as work_dev holds; the result does not depend
 * on the chunk size, two runs give the same bits, and there are no atomics. */
#define MC_SKELETON_MAX_LAYERS 64
#define MC_SKELETON_MAX_SIZE 4096
#define MC_SKELETON_MIN_RADIUS 12
#define MC_SKELETON_MAX_RADIUS 512
typedef struct mc_skeleton mc_skeleton;
typedef struct mc_skeleton_params {
    float screen[16];         /* S, row-major 4x4: world -> (X_num, Y_num, depth, W), pixel = (X_num / W, Y_num / W), row 0 on top
                                 (skeleton.Mplot3dCamera.screen_projective); row 2 is not read                                */
    int32_t width, height;    /* 1..MC_SKELETON_MAX_SIZE                                                                      */
} mc_skeleton_params;
/* Chain c is the polyline through chain_joints_host[chain_start_host[c] .. chain_start_host[c + 1]) (int32, at least 2 joints each,
 * all < num_joints; 1..61 chains) drawn chain_width_px_host[c] pixels wide; the trail is trail_width_px wide.  A width w gives the
 * radius max(MC_SKELETON_MIN_RADIUS, floor(8 w + 0.5)) sixteenths of a pixel, at most MC_SKELETON_MAX_RADIUS: w must be positive and at most 64.  palette_host uint8 [3 + num_chains][3]:
 * background, plane (already composited over the background), trail, then the chains. */
int mc_skeleton_create(const int32_t* chain_joints_host, const int32_t* chain_start_host, int32_t num_chains, int32_t num_joints,
                       const float* chain_width_px_host, float trail_width_px, const uint8_t* palette_host, mc_skeleton** out);
void mc_skeleton_destroy(mc_skeleton* h);
/* bytes that hold n_frames frames of sequences of at most max_trail frames each; -1: bad argument */
int64_t mc_skeleton_work_bytes(const mc_skeleton* h, int32_t n_frames, int32_t max_trail, int32_t width, int32_t height);
/* joints_dev fp32 [n,J,3], n = seq_start_host[num_seqs]; sequence s is the rows seq_start_host[s] .. seq_start_host[s + 1] (int32
 * [num_seqs + 1], ascending from 0, on the host).  work_dev: 16-byte aligned, at least mc_skeleton_work_bytes(h, 1, L, ...) with L the
 * longest sequence; its contents need not be kept.  -> rgb_out_dev uint8 [n,H,W,3] (4-byte aligned) and, where not NULL,
 * layer_out_dev uint8 [n,H,W] (4-byte aligned), screen_out_dev int32 [n,J + 4,2] (joints, then the plane's corners; INT32_MIN twice
 * for an invalid point), trail_screen_out_dev int32 [n,L,2] (frame i of a sequence: its trail points j < i when i >= 2, invalid
 * elsewhere), stats_out_dev fp32 [num_seqs,6] (MINS, MAXS; an empty sequence's row is not written), traj_out_dev fp32 [n,2]. */
int mc_skeleton_frames(mc_skeleton* h, const float* joints_dev, const int32_t* seq_start_host, int32_t num_seqs, const mc_skeleton_params* p,
                       void* work_dev, int64_t work_bytes, uint8_t* rgb_out_dev, uint8_t* layer_out_dev, int32_t* screen_out_dev,
                       int32_t* trail_screen_out_dev, float* stats_out_dev, float* traj_out_dev, void* stream);

/* ---- Baseline JPEG encoder: the uint8 RGB frames the two rasterisers write -> one complete JFIF file per frame, back to back in a
 * device byte buffer, for a Motion-JPEG AVI (video.AviWriter) in place of the reference's ffmpeg child processes
 * (mogen/datasets/EMAGE_2024/utils/media.py:4-33).  SOF0, 8 bit, Y / Cb / Cr, 4:2:0 or 4:4:4, the Annex K quantisation tables under the
 * IJG quality rule, the Annex K Huffman tables in every frame, one restart interval per MCU row (DRI; RST(row mod 8) between rows), edges
 * replicated up to the MCU.  The arithmetic is integer only and defined in the header comment of csrc/mc_mjpeg.hip (fixed-point JFIF
 * colour matrix, 2x2 chroma mean, a two-pass integer DCT, round-half-away quantisation), restated in tests/jpeg_ref.py: the byte stream
 * is a definition.  Frames run in chunks of as many as work_dev holds; the result does not depend on the chunk size. */
#define MC_MJPEG_420 0
#define MC_MJPEG_444 1
#define MC_MJPEG_MAX_SIZE 16384
typedef struct mc_mjpeg mc_mjpeg;
/* width, height 1..MC_MJPEG_MAX_SIZE; quality 1..100 */
int mc_mjpeg_create(int32_t width, int32_t height, int32_t quality, int32_t subsampling, mc_mjpeg** out);
void mc_mjpeg_destroy(mc_mjpeg* h);
/* scratch that holds `frames` frames at once; -1: bad argument */
int64_t mc_mjpeg_work_bytes(const mc_mjpeg* h, int32_t frames);
/* a true upper bound of the bytes `frames` frames encode to, whatever their content: per frame the header and, per restart interval,
 * 2 * 208 bytes per block (1660 bits at most, every byte stuffed) and its 2-byte marker; -1: bad argument */
int64_t mc_mjpeg_max_bytes(const mc_mjpeg* h, int32_t frames);
/* rgb_dev uint8 [n,H,W,3] -> out_dev: frame i is the bytes offsets_dev[i] .. offsets_dev[i + 1] (int64 [n + 1], offsets_dev[0] = 0).
 * work_dev: 256-byte aligned, at least mc_mjpeg_work_bytes(h, 1); its contents need not be kept.  Returns an error and launches nothing
 * when work_bytes is below that, or when out_capacity is below mc_mjpeg_max_bytes(h, n): nothing is sized by a typical ratio. */
int mc_mjpeg_encode(mc_mjpeg* h, const uint8_t* rgb_dev, int32_t n, void* work_dev, int64_t work_bytes, uint8_t* out_dev, int64_t out_capacity,
                    int64_t* offsets_dev, void* stream);

/* ---- The quality metrics over embedding tables (mogen/core/evaluation/utils.py:12-140), reduced on the device in fp64.
 * A table is [rows, d] row-major in DEVICE memory, fp32 or (table_fp64 != 0) fp64; 2..MC_EMB_MAX_ROWS rows (1.. where stated),
 * d in 1..MC_EMB_MAX_DIM.  Every `_dev` pointer is checked to be a device address: a host pointer is MC_ERR_ARG.  Results are fp64; every
 * sum runs in a fixed order (strided per-thread sums, then a fixed tree; the one atomic is an integer counter), so two runs give the
 * same bits.  Error codes: MC_ERR_ARG (null, ill-sized or host argument; workspace too small or not 8-byte aligned), MC_ERR_HIP,
 * and from mc_emb_frechet MC_ERR_NOCONV when a decomposition still rotated column pairs in its last allowed sweep.
 *
 * mc_emb_frechet: gt_dev [n, d], pred_dev [m, d] -> fid_out_dev fp64 [1] = |mu1 - mu2|^2 + Tr C1 + Tr C2 - 2 Tr sqrt(C1 C2) of the tables
 * times emb_scale, with Tr sqrt(C1 C2) = (sum of the singular values of A_c B_c^T) / sqrt((n - 1)(m - 1)) over the column-centred tables:
 * no covariance and no matrix root is formed, and the value is the exact one for positive semi-definite covariances, also when
 * n - 1 < d.  Three one-sided Jacobi decompositions (each table over min(rows, d) columns, then the small product), one launch per
 * round of disjoint column pairs.  After each sweep the call synchronises `stream` to read the count of rotated pairs; a
 * decomposition takes at most max_sweeps sweeps (0: MC_EMB_MAX_SWEEPS; 1..MC_EMB_MAX_SWEEPS).  work_dev: 8-byte aligned,
 * mc_emb_frechet_work_bytes(n, m, d) bytes (-1: bad argument), contents need not be kept.  info_host (HOST memory, may be NULL):
 * int32 [6] = sweeps and round launches of the decompositions of gt, pred and the product.
 * mc_emb_statistics: -> mean_out_dev fp64 [d], cov_out_dev fp64 [d, d]: np.mean / np.cov(rowvar=False) of table * emb_scale
 * (calculate_activation_statistics); work_dev as above with mc_emb_statistics_work_bytes(n, d).
 * mc_emb_zscore: table [n >= 1, d] -> out_dev fp64 [n, d] = (x - column mean) / population standard deviation, a deviation of
 * exactly zero replaced by 1e-8 (evaluation._zscore).
 * mc_emb_retrieval: text_dev, motion_dev [n >= 1, d] cut into batches of `batch` (1..MC_EMB_MAX_BATCH) rows, the last one ragged; within a
 * batch dist(t_i, m_j) = sqrt(sum (t_i - m_j)^2) from direct differences and rank_i = #{j : dist(t_i, m_j) < dist(t_i, m_i)} +
 * #{j < i : dist(t_i, m_j) = dist(t_i, m_i)} -> counts_out_dev int32 [ceil(n / batch), top_k]: per batch the rows with rank_i < k for
 * k = 1..top_k (1..MC_EMB_MAX_TOPK), and (may be NULL) match_sum_out_dev fp64 [ceil(n / batch)]: the sum over the batch of dist(t_i, m_i).
 * mc_emb_pair_distance: table [groups, rows, d] (groups * rows <= MC_EMB_MAX_ROWS), first_dev / second_dev int32 [n_pairs] row indices
 * in 0..rows - 1 (an index outside is clamped into the table) -> mean_out_dev fp64 [1]: the mean over groups and pairs of
 * |(a[g, first] * emb_scale - a[g, second] * emb_scale) * norm_scale| (calculate_diversity with groups = 1, calculate_multimodality). */
#define MC_EMB_MAX_DIM 512
#define MC_EMB_MAX_ROWS 1048576
#define MC_EMB_MAX_BATCH 64
#define MC_EMB_MAX_TOPK 64
#define MC_EMB_MAX_SWEEPS 30
int64_t mc_emb_frechet_work_bytes(int32_t n, int32_t m, int32_t d);
int mc_emb_frechet(const void* gt_dev, int32_t n, const void* pred_dev, int32_t m, int32_t d, int32_t table_fp64, double emb_scale, int32_t max_sweeps,
                   void* work_dev, int64_t work_bytes, double* fid_out_dev, int32_t* info_host, void* stream);
int64_t mc_emb_statistics_work_bytes(int32_t n, int32_t d);
int mc_emb_statistics(const void* table_dev, int32_t n, int32_t d, int32_t table_fp64, double emb_scale, void* work_dev, int64_t work_bytes,
                      double* mean_out_dev, double* cov_out_dev, void* stream);
int mc_emb_zscore(const void* table_dev, int32_t n, int32_t d, int32_t table_fp64, double* out_dev, void* stream);
int mc_emb_retrieval(const void* text_dev, const void* motion_dev, int32_t n, int32_t d, int32_t table_fp64, int32_t batch, int32_t top_k,
                     int32_t* counts_out_dev, double* match_sum_out_dev, void* stream);
int mc_emb_pair_distance(const void* table_dev, int32_t groups, int32_t rows, int32_t d, int32_t table_fp64, const int32_t* first_dev,
                         const int32_t* second_dev, int32_t n_pairs, double emb_scale, double norm_scale, double* mean_out_dev, void* stream);

/* out = a * x + b * noise over n elements (out may alias x) */
int mc_op_renoise(const float* x_dev, const float* noise_dev, float a, float b, float* out_dev, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MOTIONCRAFT_AMD_H */
