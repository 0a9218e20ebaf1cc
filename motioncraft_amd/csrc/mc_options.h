// Per-context runtime options (mc_ctx_set_option keys, seeded from MC_* environment variables) and the named bits of the chain
// mask.  One table in mc_model.hip (kOptions) gives each option its key, variable, built-in default and validity check.
#pragma once

// bits of McOptions::chain: schedule and kernel selection (DESIGN.md section 5 has the history and the measurements)
enum ChainBit {
    kChainMlp = 0,               // fused expert / SFFN MLP (mlp2_k)
    kChainGate = 1,              // fused gate (gate_k)
    kChainRowchain = 2,          // chained proj / q/k/v (rowchain_k)
    kChainTwoStreams = 5,        // large batches: the two sample groups (the CFG halves) on two streams
    kChainPqBody = 15,           // pqbody_k: projqkv_k's work plus the body-topology attention
    kChainTwinSplit = 16,        // the twin layer's gate / experts / front kernels as two sample sub-groups on the two streams
    kChainFilmPlanes = 17,       // reduced precision: film_rows_k writes the FiLM GEMM's A operand as fp16 planes (gemm_hd_k)
    kChainMlpDma = 18,           // the fused MLPs stage their weight chunks by LDS-DMA (mlp2d_k / mlp2hd_k)
    kChainTemporalHalf = 20,     // reduced precision: temporal linear attention on the fp16 MFMA (temporal_h_k)
    kChainTailOnePass = 21,      // large batches: folded decoder tail with the CFG combination in its A staging (gemm_tail_k)
    kChainTemporalPair = 22,     // L = 64: temporal_k takes two adjacent parts per workgroup
    kChainSkipText = 24,         // temporal_k: the unconditional half skips whole leading blocks of its masked text rows
    kChainStagger = 26,          // fp32, L = 128: the second group's first FiLM block starts behind the first group's FiLM row kernel
    kChainResidualPre = 27,      // reduced precision: the plane GEMM prefetches its epilogue's residual rows (gemm_hd_k<., true>)
    kChainFragMajor = 29,        // reduced precision: fragment-major FiLM planes, A fragments straight into registers (gemm_hf_k)
    kChainBits = 30,             // bits from here up are not defined
};
// Retired bits: the numbers stay reserved and a mask that sets one is rejected.  3, 23, 25 and 28 lost their A/B; the others were on by
// default with an off-arm that no test used as a reference, so the arm went and what the bit switched on is now unconditional:
//    3  the temporal branch on the side stream at every batch size
//    4  CFG twin dedupe in base layer 0
//    6  one expert-MLP launch per sample group (the two-stream schedule with one whole-batch expert launch went)
//    7  last FiLM Linear + pose decoder on the CFG-combined rows (the sampler entry points always defer it)
//    8  twin aliasing of the mf / qkv / ys rows in base layer 0
//    9  the sample groups stay on their streams across the control-branch ops (the per-layer re-join went)
//   10  large batches: proj + body LN + q/k/v in one kernel (projqkv_k)
//   11  folded decoder tail as one grouped GEMM + sum in the sampler kernel (the two-dense form went)
//   12  small batches: the FiLM row kernel adds up the SFFN's split-hidden partial sums (the reduce launch went)
//   13  B = 1 sizes: the expert MLP picks 3 or 4 hidden slices on the device
//   14  small batches: temporal branch on the main stream, LN + q/k/v + body on the side stream
//   19  mc_sample_loop: the sampler update also writes x_{t-1} padded for the next pose-encoder GEMM
//   23  the last group's gate launch cut at whole workgroup rounds
//   25  the twin layer's front covering its sub-group's twins in the same launch
//   28  plain f16: the plane GEMM's accumulators start as R + bias
constexpr long kChainRetired = 1L << 3 | 1L << 4 | 1L << 6 | 1L << 7 | 1L << 8 | 1L << 9 | 1L << 10 | 1L << 11 | 1L << 12 | 1L << 13 | 1L << 14 |
                               1L << 19 | 1L << 23 | 1L << 25 | 1L << 28;
constexpr long kChainDefault = ((1L << kChainBits) - 1) & ~kChainRetired;
static_assert(kChainDefault == 762806311, "the default chain mask is public ABI");

// Resolved values, one field per row of kOptions (mc_model.hip: key = field name, variable, default, meaning, check)
struct McOptions {
    long chain, small_gemm_rows, split_rows_expert, split_rows_sffn, temporal_split, big_tokens, rowchain_split;
    long gemm_tune, small_tile_n, gemm_wp_grid, half_min_rows, gate_small, split_expert, split_sffn;
    long route_reg, route_coop, route_small, route_early, route_per, dbg_delay_us;
};

// The options of context-free launches (mc_op_*, the text / eval / wav encoders): one snapshot of the environment through the same
// table, taken at first use.  nullptr (the last error names the variable) if a variable holds an invalid value: return MC_ERR_ARG.
const McOptions* mc_process_options();
