// fp32 MFMA GEMM family for the STMoGen denoiser (gfx950).
//
//   C[M,N] = epilogue( prologue(A)[M,K] * W[N,K]^T + bias[N] )
//
// All matrices fp32 row-major, K contiguous in both operands (nn.Linear weight layout).
// One 256-thread workgroup (4 waves, 2x2) computes a 128x128 tile with
// v_mfma_f32_32x32x2_f32 (exact fp32, 157 TF chip peak); each wave owns 64x64 = 2x2 MFMA
// tiles (64 accumulator VGPRs).  Operands are staged through LDS in [rows][32+4] tiles,
// double buffered, read back as one ds_read_b128 per 4 MFMA k-steps: inside an 8-wide k-group
// lanes 0-31 take k = 8j..8j+3 and lanes 32-63 take k = 8j+4..8j+7, which is a permutation of the
// k order applied identically to A and W (the dot product is order-independent up to rounding).
// The +4 pad makes both the b128 reads and the b128 staging writes bank-conflict free.
//
// The W tile is fed as the MFMA "A" operand and the activation tile as "B", i.e. each wave
// computes C^T fragments: lane l then owns output row m = l & 31 and, per accumulator quad,
// FOUR CONSECUTIVE output columns -> the epilogue is 16 float4 stores per lane (bias / residual
// loaded as float4 too) instead of 64 scalar ones.
//
// Modes (one kernel instantiation each):
//   GM_PLAIN  dense / part-grouped (blockIdx.y = group) with optional activation and residual
//   GM_EXP1   expert FC1 over device-built slot tiles: A row = src_row[slot], C row = slot
//   GM_EXP2   expert FC2: A row = slot, C row = dst_row[slot]  (= 2*token + choice)
//   GM_COMB   A[r][k] = gelu(w0[r]*Y[2r][k] + w1[r]*Y[2r+1][k]) (post-score combine of the two
//             expert outputs of a token, dropped choices have w = 0), then dense GEMM
//   GM_ENC    pose encoder / first conv layer: rows may be unaligned (scalar loads on the guarded path), + row-periodic add table
//             (positional embedding) and duplicate-row write (the two CFG halves share h0)
#include "mc_common.h"
#include "mc_gemm.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 32, LD = BK + 4;

struct Stage {
    long aoff[4], woff[4];
    bool aok[4], wok[4];
    float cw0[4], cw1[4];
};

template <int MODE, bool GUARD>
__device__ __forceinline__ void load_tile(const GemmArgs& g, const float* __restrict__ Ab, const float* __restrict__ Wb,
                                          const Stage& st, int k, f32x4 (&ra)[4], f32x4 (&rb)[4]) {
    const bool kin = !GUARD || k < g.K;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if ((!GUARD || st.aok[i]) && kin) {
            if constexpr (MODE == GM_COMB) {
                f32x4 y0 = {0.f, 0.f, 0.f, 0.f}, y1 = {0.f, 0.f, 0.f, 0.f};
                if (st.cw0[i] != 0.f) y0 = *reinterpret_cast<const f32x4*>(Ab + st.aoff[i] + k);
                if (st.cw1[i] != 0.f) y1 = *reinterpret_cast<const f32x4*>(Ab + st.aoff[i] + g.lda + k);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = gelu_exact(st.cw0[i] * y0[j] + st.cw1[i] * y1[j]);
            } else if constexpr (MODE == GM_ENC && GUARD) {      // unaligned rows (K or lda not a multiple of 4): scalar loads
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (k + j < g.K) v[j] = Ab[st.aoff[i] + k + j];
            } else {
                v = *reinterpret_cast<const f32x4*>(Ab + st.aoff[i] + k);
            }
        }
        ra[i] = v;
        f32x4 w = {0.f, 0.f, 0.f, 0.f};
        if ((!GUARD || st.wok[i]) && kin) w = *reinterpret_cast<const f32x4*>(Wb + st.woff[i] + k);
        rb[i] = w;
    }
}

template <int MODE, bool GUARD, bool EARLY>
__device__ __forceinline__ void mainloop(const GemmArgs& g, const float* __restrict__ Ab, const float* __restrict__ Wb,
                                         const Stage& st, float* As, float* Bs, int sr, int sk, int wm, int wn, int lane,
                                         f32x16 (&acc)[2][2]) {
    f32x4 ra[4], rb[4];
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<f32x4*>(As + buf * BM * LD + (sr + 32 * i) * LD + sk) = ra[i];
            *reinterpret_cast<f32x4*>(Bs + buf * BN * LD + (sr + 32 * i) * LD + sk) = rb[i];
        }
    };
    const int nk = (g.K + BK - 1) / BK;
    const int frow = lane & 31;
    const int fk = (lane >> 5) * 4;
    // fragments of k-group j+1 are read while the 16 MFMAs of group j execute (explicit software pipeline)
    struct Frag { f32x4 a0, a1, b0, b1; };
    auto ld_frag = [&](const float* Ap, const float* Bp, int j) {
        Frag f;
        f.a0 = *reinterpret_cast<const f32x4*>(Ap + j * 8);
        f.a1 = *reinterpret_cast<const f32x4*>(Ap + 32 * LD + j * 8);
        f.b0 = *reinterpret_cast<const f32x4*>(Bp + j * 8);
        f.b1 = *reinterpret_cast<const f32x4*>(Bp + 32 * LD + j * 8);
        return f;
    };
    auto mma = [&](const Frag& f) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            // D[n][m] += W[n][k] * A[m][k]   (W is the MFMA "A" operand)
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.b0[i], f.a0[i], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.b1[i], f.a0[i], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.b0[i], f.a1[i], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.b1[i], f.a1[i], acc[1][1], 0, 0, 0);
        }
    };
    if constexpr (!EARLY) {
        load_tile<MODE, GUARD>(g, Ab, Wb, st, sk, ra, rb);
        store_tile(0);
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const int buf = kt & 1;
            if (kt + 1 < nk) load_tile<MODE, GUARD>(g, Ab, Wb, st, (kt + 1) * BK + sk, ra, rb);
            const float* Ap = As + buf * BM * LD + (wm * 64 + frow) * LD + fk;
            const float* Bp = Bs + buf * BN * LD + (wn * 64 + frow) * LD + fk;
            Frag f0 = ld_frag(Ap, Bp, 0);
            Frag f1 = ld_frag(Ap, Bp, 1);
            mma(f0);
            f0 = ld_frag(Ap, Bp, 2);
            mma(f1);
            f1 = ld_frag(Ap, Bp, 3);
            mma(f0);
            mma(f1);
            if (kt + 1 < nk) store_tile(buf ^ 1);
            __syncthreads();
        }
    } else {
        // Staging in the MIDDLE of the MFMA stream with ONE register set: after the first 16 MFMAs of
        // k-tile kt the registers holding tile kt+1 (requested during iteration kt-1, ~48 MFMAs = 1.4 us
        // earlier, so the vmcnt wait in front of the LDS writes is already satisfied) are written to the
        // other LDS buffer, then tile kt+2 is requested into the same registers.  Neither the global
        // latency nor the staging writes sit between the last MFMA and the barrier.
        load_tile<MODE, GUARD>(g, Ab, Wb, st, sk, ra, rb);
        store_tile(0);
        if (nk > 1) load_tile<MODE, GUARD>(g, Ab, Wb, st, BK + sk, ra, rb);
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {
            const int buf = kt & 1;
            const float* Ap = As + buf * BM * LD + (wm * 64 + frow) * LD + fk;
            const float* Bp = Bs + buf * BN * LD + (wn * 64 + frow) * LD + fk;
            Frag f0 = ld_frag(Ap, Bp, 0);
            Frag f1 = ld_frag(Ap, Bp, 1);
            mma(f0);
            f0 = ld_frag(Ap, Bp, 2);
            if (kt + 1 < nk) store_tile(buf ^ 1);
            if (kt + 2 < nk) load_tile<MODE, GUARD>(g, Ab, Wb, st, (kt + 2) * BK + sk, ra, rb);
            mma(f1);
            f1 = ld_frag(Ap, Bp, 3);
            mma(f0);
            mma(f1);
            __syncthreads();
        }
    }
}

// vector epilogue: lane owns row m = (lane & 31) of each 32-row block and 4 consecutive columns per quad
template <int MODE, bool GUARD, int ACT>
__device__ __forceinline__ void epilogue_vec(const GemmArgs& g, int grp, int row0, int nrows, int tn, int wm, int wn,
                                             int lane, f32x16 (&acc)[2][2]) {
    const float* __restrict__ bias = g.bias ? g.bias + (long)grp * g.b_gstride : nullptr;
    float* __restrict__ Cb = g.C + (long)grp * g.c_gstride + g.c_col;
    const float* __restrict__ Rb = g.R ? g.R + (long)grp * (g.r_gstride >= 0 ? g.r_gstride : g.c_gstride) + g.c_col : nullptr;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
        const int m = wm * 64 + mi * 32 + (lane & 31);
        if (GUARD && m >= nrows) continue;
        long drow = row0 + m;
        if constexpr (MODE == GM_EXP2) drow = g.dst_row[row0 + m];
        float* crow = Cb + drow * g.ldc;
        const float* rrow = Rb ? Rb + drow * g.ldr : nullptr;
        const float* arow = nullptr;
        if constexpr (MODE == GM_ENC) arow = g.add ? g.add + (long)((row0 + m) % g.add_mod) * g.ld_add : nullptr;
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = tn * BN + wn * 64 + ni * 32 + 8 * q + 4 * (lane >> 5);
                if (GUARD && n >= g.N) continue;
                f32x4 v = {acc[mi][ni][4 * q], acc[mi][ni][4 * q + 1], acc[mi][ni][4 * q + 2], acc[mi][ni][4 * q + 3]};
                if (bias) v += *reinterpret_cast<const f32x4*>(bias + n);
                if (g.act_after_res && rrow) v += *reinterpret_cast<const f32x4*>(rrow + n);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = apply_act(v[j], ACT);
                if constexpr (MODE == GM_ENC) {
                    if (arow) v += *reinterpret_cast<const f32x4*>(arow + n);
                }
                if (!g.act_after_res && rrow) v += *reinterpret_cast<const f32x4*>(rrow + n);
                *reinterpret_cast<f32x4*>(crow + n) = v;
                if constexpr (MODE == GM_ENC) {
                    if (g.dup_rows) *reinterpret_cast<f32x4*>(crow + g.dup_rows * g.ldc + n) = v;
                }
            }
        }
    }
}

// scalar epilogue for outputs whose rows are not 16-byte aligned (pose decoder: N = 322)
template <int MODE>
__device__ __forceinline__ void epilogue_scalar(const GemmArgs& g, int grp, int row0, int nrows, int tn, int wm, int wn,
                                                int lane, f32x16 (&acc)[2][2]) {
    const float* __restrict__ bias = g.bias ? g.bias + (long)grp * g.b_gstride : nullptr;
    float* __restrict__ Cb = g.C + (long)grp * g.c_gstride + g.c_col;
    const float* __restrict__ Rb = g.R ? g.R + (long)grp * (g.r_gstride >= 0 ? g.r_gstride : g.c_gstride) + g.c_col : nullptr;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
        const int m = wm * 64 + mi * 32 + (lane & 31);
        if (m >= nrows) continue;
        long drow = row0 + m;
        if constexpr (MODE == GM_EXP2) drow = g.dst_row[row0 + m];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int n = tn * BN + wn * 64 + ni * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
                if (n >= g.N) continue;
                float v = acc[mi][ni][reg];
                if (bias) v += bias[n];
                if (g.act_after_res && Rb) v += Rb[drow * g.ldr + n];
                v = apply_act(v, g.act);
                if (!g.act_after_res && Rb) v += Rb[drow * g.ldr + n];
                Cb[drow * g.ldc + n] = v;
            }
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(256, 2) void gemm_k(GemmArgs g) {
    __shared__ __attribute__((aligned(16))) float smem[2 * (BM + BN) * LD];
    float* As = smem;                  // [2][BM*LD]
    float* Bs = smem + 2 * BM * LD;    // [2][BN*LD]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    const int ntn = (g.N + BN - 1) / BN;
    int bid, grp = blockIdx.y;
    if constexpr (MODE == GM_EXP1 || MODE == GM_EXP2) {
        // the launch covers the worst-case tile count; remap over the tiles that exist
        const int real = *g.num_tiles * ntn;
        if ((int)blockIdx.x >= real) return;
        bid = xcd_remap(blockIdx.x, real);
    } else {
        bid = xcd_remap(blockIdx.x, gridDim.x);
    }
    const int tm = bid / ntn, tn = bid % ntn;
    int row0, nrows;
    if constexpr (MODE == GM_EXP1 || MODE == GM_EXP2) {
        grp = g.tile_group[tm];
        row0 = g.tile_row0[tm];
        nrows = g.tile_nrows[tm];
    } else {
        row0 = tm * BM;
        nrows = min(BM, g.M - row0);
        if (nrows <= 0) return;
    }
    const float* __restrict__ Ab = g.A + (long)grp * g.a_gstride + g.a_col;
    const float* __restrict__ Wb = g.W + (long)grp * g.w_gstride;

    // staging assignment: thread -> rows (tid>>3) + 32*i, k-column (tid&7)*4
    const int sr = tid >> 3;
    const int sk = (tid & 7) * 4;
    Stage st;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = sr + 32 * i;
        st.aok[i] = r < nrows;
        long srow = row0 + r;
        if constexpr (MODE == GM_EXP1) srow = st.aok[i] ? g.src_row[row0 + r] : 0;
        if constexpr (MODE == GM_COMB) {
            st.aoff[i] = 2 * srow * g.lda;
            st.cw0[i] = st.aok[i] ? g.comb_w[2 * srow] : 0.f;
            st.cw1[i] = st.aok[i] ? g.comb_w[2 * srow + 1] : 0.f;
        } else {
            st.aoff[i] = srow * g.lda;
        }
        const int n = tn * BN + r;
        st.wok[i] = n < g.N;
        st.woff[i] = (long)n * g.ldw;
    }

    f32x16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    const bool full = nrows == BM && (tn + 1) * BN <= g.N && (g.K % BK) == 0 &&
                      (MODE != GM_ENC || (g.lda % 4 == 0 && g.a_gstride % 4 == 0));
    if (full) {
        if (g.tune & kTuneStaging) mainloop<MODE, false, true>(g, Ab, Wb, st, As, Bs, sr, sk, wm, wn, lane, acc);
        else mainloop<MODE, false, false>(g, Ab, Wb, st, As, Bs, sr, sk, wm, wn, lane, acc);
    } else {
        mainloop<MODE, true, false>(g, Ab, Wb, st, As, Bs, sr, sk, wm, wn, lane, acc);
    }

    const bool vec = (g.N % 4 == 0) && (g.ldc % 4 == 0) && (g.c_col % 4 == 0) && (g.c_gstride % 4 == 0) &&
                     (!g.R || (g.ldr % 4 == 0 && (g.r_gstride < 0 || g.r_gstride % 4 == 0)));
    if (!vec) {
        epilogue_scalar<MODE>(g, grp, row0, nrows, tn, wm, wn, lane, acc);
    } else if (full) {
        if (g.act == ACT_GELU) epilogue_vec<MODE, false, ACT_GELU>(g, grp, row0, nrows, tn, wm, wn, lane, acc);
        else if (g.act == ACT_SILU) epilogue_vec<MODE, false, ACT_SILU>(g, grp, row0, nrows, tn, wm, wn, lane, acc);
        else if (g.act == ACT_LRELU) epilogue_vec<MODE, false, ACT_LRELU>(g, grp, row0, nrows, tn, wm, wn, lane, acc);
        else if (g.act == ACT_QUICKGELU) epilogue_vec<MODE, false, ACT_QUICKGELU>(g, grp, row0, nrows, tn, wm, wn, lane, acc);
        else epilogue_vec<MODE, false, ACT_NONE>(g, grp, row0, nrows, tn, wm, wn, lane, acc);
    } else {
        if (g.act == ACT_GELU) epilogue_vec<MODE, true, ACT_GELU>(g, grp, row0, nrows, tn, wm, wn, lane, acc);
        else if (g.act == ACT_SILU) epilogue_vec<MODE, true, ACT_SILU>(g, grp, row0, nrows, tn, wm, wn, lane, acc);
        else if (g.act == ACT_LRELU) epilogue_vec<MODE, true, ACT_LRELU>(g, grp, row0, nrows, tn, wm, wn, lane, acc);
        else if (g.act == ACT_QUICKGELU) epilogue_vec<MODE, true, ACT_QUICKGELU>(g, grp, row0, nrows, tn, wm, wn, lane, acc);
        else epilogue_vec<MODE, true, ACT_NONE>(g, grp, row0, nrows, tn, wm, wn, lane, acc);
    }
}

// ---------------------------------------------------------------------------------------
// LDS-DMA variant of the plain GEMM for launches made of full tiles only (M % 128 == N % 128 == K % 32 == 0):
// `global_load_lds_dwordx4` writes each lane's 16 bytes straight into LDS (lane-linear, 1 KiB per wave-instruction),
// so there is no register staging and no ds_write in the k-loop.  The LDS image is the unpadded [128][32] tile; the
// 16-byte chunk a lane fetches is XOR-swizzled with its row (chunk c of row r sits at position c ^ (r & 7)) so the
// b128 fragment reads of 8 consecutive rows hit 8 different bank groups (rows r and r+8 still share one: 2-way).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void gemm_dma_k(GemmArgs g) {
    __shared__ __attribute__((aligned(16))) float smem[2 * (BM + BN) * BK];
    float* As = smem;                  // [2][BM][BK]
    float* Bs = smem + 2 * BM * BK;    // [2][BN][BK]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int ntn = g.N / BN;
    const int bid = (g.tune & kTuneNoXcd) ? (int)blockIdx.x : xcd_remap(blockIdx.x, gridDim.x);
    const int tm = bid / ntn, tn = bid % ntn;
    const int row0 = tm * BM;
    const float* __restrict__ Ab = g.A + g.a_col;
    const float* __restrict__ Wb = g.W;
    // DMA assignment: wave w moves rows [32w, 32w+32) of both tiles, 8 rows per instruction;
    // lane l -> row 8q + (l >> 3), LDS position l & 7, global chunk (l & 7) ^ (l >> 3)
    const int dr = lane >> 3, dc = ((lane & 7) ^ dr) * 4;
    const float* ga = Ab + (long)(row0 + 32 * wave + dr) * g.lda + dc;
    const float* gw = Wb + (long)(tn * BN + 32 * wave + dr) * g.ldw + dc;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);    // the LDS destination goes to M0: must be provably uniform
    auto issue = [&](int kt, int buf) {
        float* la = As + buf * BM * BK + 32 * wave_u * BK;
        float* lw = Bs + buf * BN * BK + 32 * wave_u * BK;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            __builtin_amdgcn_global_load_lds(ga + (long)8 * q * g.lda + kt * BK, la + 8 * q * BK, 16, 0, 0);
            __builtin_amdgcn_global_load_lds(gw + (long)8 * q * g.ldw + kt * BK, lw + 8 * q * BK, 16, 0, 0);
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
    const int frow = lane & 31, hf = lane >> 5, sw = frow & 7;
    struct Frag { f32x4 a0, a1, b0, b1; };
    auto ld_frag = [&](const float* At, const float* Bt, int j) {
        const int pos = ((2 * j + hf) ^ sw) * 4;          // rows frow and frow + 32 share frow & 7
        Frag f;
        f.a0 = *reinterpret_cast<const f32x4*>(At + pos);
        f.a1 = *reinterpret_cast<const f32x4*>(At + 32 * BK + pos);
        f.b0 = *reinterpret_cast<const f32x4*>(Bt + pos);
        f.b1 = *reinterpret_cast<const f32x4*>(Bt + 32 * BK + pos);
        return f;
    };
    auto mma = [&](const Frag& f) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.b0[i], f.a0[i], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.b1[i], f.a0[i], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.b0[i], f.a1[i], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.b1[i], f.a1[i], acc[1][1], 0, 0, 0);
        }
    };
    const int nk = g.K / BK;
    issue(0, 0);
    __syncthreads();                                      // (its fence waits vmcnt(0): the DMA has landed)
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) issue(kt + 1, buf ^ 1);          // in flight during the 64 MFMAs below
        const float* At = As + buf * BM * BK + (wm * 64 + frow) * BK;
        const float* Bt = Bs + buf * BN * BK + (wn * 64 + frow) * BK;
        // fragments of k-group j+1 are requested BEFORE the 16 MFMAs of group j (sched_barrier: the scheduler otherwise
        // sinks the reads to their use and exposes the LDS latency four times per k-tile)
        Frag f0 = ld_frag(At, Bt, 0);
        Frag f1 = ld_frag(At, Bt, 1);
        __builtin_amdgcn_sched_barrier(0);
        mma(f0);
        f0 = ld_frag(At, Bt, 2);
        __builtin_amdgcn_sched_barrier(0);
        mma(f1);
        f1 = ld_frag(At, Bt, 3);
        __builtin_amdgcn_sched_barrier(0);
        mma(f0);
        mma(f1);
        __syncthreads();
    }
    if (g.act == ACT_GELU) epilogue_vec<GM_PLAIN, false, ACT_GELU>(g, 0, row0, BM, tn, wm, wn, lane, acc);
    else if (g.act == ACT_SILU) epilogue_vec<GM_PLAIN, false, ACT_SILU>(g, 0, row0, BM, tn, wm, wn, lane, acc);
    else if (g.act == ACT_NONE) epilogue_vec<GM_PLAIN, false, ACT_NONE>(g, 0, row0, BM, tn, wm, wn, lane, acc);
    else epilogue_vec<GM_PLAIN, false, ACT_LRELU>(g, 0, row0, BM, tn, wm, wn, lane, acc);
}

// ---------------------------------------------------------------------------------------
// Wave-private pipeline variant of the plain full-tile GEMM: NO workgroup barrier in the k-loop.
// The 128 x 128 block tile is still four 64 x 64 wave tiles, but every wave streams its OWN operand rows (64 rows of A and
// 64 rows of W, 16 k-columns per stage) into a private LDS ring with LDS-DMA and orders itself with its own counted
// `s_waitcnt vmcnt` -- the DMA instructions are inline asm, so the compiler neither counts them nor drains them in front
// of LDS reads (guide section 5.7).  Cost: every operand row is fetched by two waves of the workgroup (L1/L2 hits);
// gain: a wave never waits for another wave, the two waves that share a SIMD (one of each co-resident workgroup) drift
// freely and fill each other's issue gaps, and the per-k-tile barrier + its vmcnt(0) drain are gone.
// LDS image of a stage: [A rows 0..63 | W rows 0..63][16 floats], 16-byte chunk c of row r at position c ^ ((r >> 2) & 3)
// (conflict-free ds_read_b128 of any aligned 16-lane group: 4 rows share a 256-byte bank row, rows 4 apart differ in the XOR).
// ---------------------------------------------------------------------------------------
constexpr int WBK = 16, WSTAGE = 128 * WBK;     // floats per stage of one wave: (64 + 64) rows x 16 (dma16: mc_common.h)

// Persistent form: gridDim.x <= 2 workgroups per CU walk the tile list (tile = blockIdx.x, += gridDim.x); a wave goes from the
// stores of one tile straight into the first DMAs of the next, and the residual / bias rows of a tile are requested two
// k-tiles before its k-loop ends, so neither the operand prologue nor the epilogue reads sit exposed between two k-loops
// and the waves of the chip drift out of the launch-synchronised rounds in which every tile's epilogue traffic bursts at once.
__global__ __launch_bounds__(256, 2) void gemm_wp_k(GemmArgs g) {
    __shared__ __attribute__((aligned(16))) float smem[4 * 2 * WSTAGE];      // 4 waves x 2 stages x 8 KB = 64 KB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int ntn = g.N / BN, ntiles = (g.M / BM) * ntn;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    float* wbase = smem + wave_u * 2 * WSTAGE;
    const unsigned lds0 = (unsigned)(size_t)wbase;                            // LDS byte offset of this wave's ring
    // DMA piece q (16 rows x 64 bytes per wave-instruction): lane -> row 16 q + (lane >> 2), LDS position lane & 3,
    // global chunk (lane & 3) ^ ((row >> 2) & 3)   (16 q is a multiple of 4: the XOR term does not depend on q)
    const int dr = lane >> 2, dc = ((lane & 3) ^ ((dr >> 2) & 3)) * 4;
    const int frow = lane & 31, hf = lane >> 5, sw = (frow >> 2) & 3;
    const float* Ab = g.A + g.a_col;
    const float* Wb = g.W;
    const float* __restrict__ Rb = g.R ? g.R + g.c_col : nullptr;
    float* __restrict__ Cb = g.C + g.c_col;
    const int nk = g.K / WBK;
    struct Frag { f32x4 a0, a1, b0, b1; };
    auto ld_frag = [&](int st, int j) {          // k-group j (8 columns) of the stage: rows frow and frow + 32 share the XOR term
        const float* S = wbase + st * WSTAGE + frow * WBK + ((2 * j + hf) ^ sw) * 4;
        Frag f;
        f.a0 = *reinterpret_cast<const f32x4*>(S);
        f.a1 = *reinterpret_cast<const f32x4*>(S + 32 * WBK);
        f.b0 = *reinterpret_cast<const f32x4*>(S + 64 * WBK);
        f.b1 = *reinterpret_cast<const f32x4*>(S + 96 * WBK);
        return f;
    };
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int bid = (g.tune & kTuneNoXcd) ? t : xcd_remap(t, ntiles);
        const int tm = bid / ntn, tn = bid % ntn;
        const int row0 = tm * BM;
        unsigned voa[4], vow[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            voa[q] = (unsigned)(((long)(row0 + wm * 64 + 16 * q + dr) * g.lda + dc) * 4);
            vow[q] = (unsigned)(((long)(tn * BN + wn * 64 + 16 * q + dr) * g.ldw + dc) * 4);
        }
        auto issue_q = [&](int kt, int st, int q) {
            const unsigned l = lds0 + st * WSTAGE * 4;
            dma16(voa[q], Ab + kt * WBK, l + q * 1024);
            dma16(vow[q], Wb + kt * WBK, l + 4096 + q * 1024);
        };
        f32x16 acc[2][2];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;
        auto mma2 = [&](const Frag& f, int i0) {     // two of the four k-steps of a fragment: 8 MFMAs
#pragma unroll
            for (int i = i0; i < i0 + 2; ++i) {
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.b0[i], f.a0[i], acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.b1[i], f.a0[i], acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.b0[i], f.a1[i], acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.b1[i], f.a1[i], acc[1][1], 0, 0, 0);
            }
        };
        // (the stage buffers were last read by MFMAs of the previous tile that have issued: free)
#pragma unroll
        for (int q = 0; q < 4; ++q) issue_q(0, 0, q);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (also drains the previous tile's stores)
        Frag f0 = ld_frag(0, 0);
        auto ktile = [&](int kt) {
            const int st = kt & 1;
            const bool more = kt + 1 < nk;
            Frag f1 = ld_frag(st, 1);
            __builtin_amdgcn_sched_barrier(0);
            mma2(f0, 0);
            // the next k-tile's 8 DMAs are spread over the first two MFMA groups (one issue slot each behind an MFMA)
            if (more) { issue_q(kt + 1, st ^ 1, 0); issue_q(kt + 1, st ^ 1, 1); }
            __builtin_amdgcn_sched_barrier(0);
            mma2(f0, 2);
            if (more) { issue_q(kt + 1, st ^ 1, 2); issue_q(kt + 1, st ^ 1, 3); }
            __builtin_amdgcn_sched_barrier(0);
            mma2(f1, 0);
            if (more) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                f0 = ld_frag(st ^ 1, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            mma2(f1, 2);
        };
        const int npre = nk > 2 ? nk - 2 : 0;
        for (int kt = 0; kt < npre; ++kt) ktile(kt);
        // epilogue operands requested under the last two k-tiles: residual rows + bias (C^T fragment layout: lane = row)
        f32x4 rv[2][2][4], bv[2][4];
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = tn * BN + wn * 64 + ni * 32 + 8 * q + 4 * hf;
                bv[ni][q] = g.bias ? *reinterpret_cast<const f32x4*>(g.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) {
                    const long m = row0 + wm * 64 + mi * 32 + frow;
                    rv[mi][ni][q] = Rb ? *reinterpret_cast<const f32x4*>(Rb + m * g.ldr + n) : f32x4{0.f, 0.f, 0.f, 0.f};
                    // row-periodic table (pose encoder: + sequence_embedding[t]); a launch has R or the table, not both
                    if (g.add) rv[mi][ni][q] = *reinterpret_cast<const f32x4*>(g.add + (m % g.add_mod) * g.ld_add + n);
                }
            }
        for (int kt = npre; kt < nk; ++kt) ktile(kt);
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
            float* crow = Cb + (long)(row0 + wm * 64 + mi * 32 + frow) * g.ldc;
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int n = tn * BN + wn * 64 + ni * 32 + 8 * q + 4 * hf;
                    f32x4 v = {acc[mi][ni][4 * q], acc[mi][ni][4 * q + 1], acc[mi][ni][4 * q + 2], acc[mi][ni][4 * q + 3]};
                    v += bv[ni][q];
                    if (g.act != ACT_NONE) {
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj) v[jj] = apply_act(v[jj], g.act);
                    }
                    v += rv[mi][ni][q];
                    *reinterpret_cast<f32x4*>(crow + n) = v;
                    if (g.dup_rows) *reinterpret_cast<f32x4*>(crow + g.dup_rows * g.ldc + n) = v;      // the two CFG halves share the encoder output
                }
        }
    }
}

// ---------------------------------------------------------------------------------------
// Small-M variant (latency-bound launches of a few hundred rows): 64 x 64 tiles, each wave one 32 x 32 MFMA tile, so
// the serial MFMA chain per k-tile is 16 instead of 64 instructions and a K = 1536 product takes ~30 us instead of
// ~105 us per tile; 4x more workgroups fill the chip without splitting K (no partial sums, no reduction pass).
// C = A W^T + bias (+ add[(r % add_mod)]) + R (also written dup_rows below), fp32, lda / ldw % 4 == 0, K % 32 == 0; any M, N
// (float4 epilogue when N % 64 == 0 and the output rows are 16-byte aligned, guarded scalar stores otherwise).
// ---------------------------------------------------------------------------------------
constexpr int SM = 64, SN = 64, SRING = 4;
// Operand staging: LDS-DMA into a ring of SRING stages, issued THREE k-tiles ahead (no staging registers, no ds_write in
// the loop).  The DMAs are inline asm with hand-counted s_waitcnt (the compiler's own insertion drains every outstanding
// load in front of an LDS access of the loop).  LDS image of a stage: unpadded [64][32] A rows then [64][32] W rows, 16-byte
// chunk c of row r at position c ^ (r & 7) (gemm_dma_k's layout); accumulation order over k is unchanged: results are
// bit-identical to the register double buffer this kernel used first.  Measured: the SAME speed as that version (and
// fragment double buffering across the barrier or DMA issue / LDS reads dealt out behind single MFMAs are 1-2 us SLOWER):
// the bare 768-MFMA chain of a K = 1536 tile is 22.9 us (tools/clock_probe.hip), the loop sits within ~2 us of it, the
// rest of a 34 us launch is the first operand round trip and the epilogue.  What does help: the epilogue operands
// requested before the loop (-1.2 us) and, per launch, a tile width that evens out the work per CU (gemm_small16_k).
template <bool VEC>     // VEC: N % 64 == 0 and 16-byte aligned output rows (float4 epilogue); else guarded scalar stores
__global__ __launch_bounds__(256) void gemm_small_k(GemmArgs g) {
    __shared__ __attribute__((aligned(16))) float smem[SRING * 2 * SM * BK];      // 4 x (8 + 8) KB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int ntn = (g.N + SN - 1) / SN;
    // XCD-aware tile order (tune bit 8): consecutive tile ids -- the ntn column tiles of one row block -- run on ONE XCD, so the row
    // block's A rows are fetched into that XCD's L2 once instead of once per column tile (the folded decoder tail, N = 322 in six
    // 64-wide tiles, fetched its 154 MB of A six times: 980 MB per launch, profiles/r03_pmc_hbm_traffic.txt).  Same arithmetic per tile.
    const int bid = (g.tune & kTuneSmallXcd) ? xcd_remap((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
    const int tm = bid / ntn, tn = bid % ntn, grp = blockIdx.y;
    const int row0 = tm * SM;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    // DMA piece q of a wave: rows 16 wave + 8 q + (lane >> 3) of the A slab and of the W slab, LDS position lane & 7,
    // global chunk (lane & 7) ^ (row & 7); rows past M / N re-read the last row (never stored)
    const int dr = lane >> 3, dc = ((lane & 7) ^ dr) * 4;
    const float* Ab = g.A + (long)grp * g.a_gstride + g.a_col;       // uniform bases (SGPR pair of the DMA)
    const float* Wb = g.W + (long)grp * g.w_gstride;
    unsigned voa[2], vow[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int ar = min(row0 + 16 * wave + 8 * q + dr, g.M - 1), wr = min(tn * SN + 16 * wave + 8 * q + dr, g.N - 1);
        voa[q] = (unsigned)(((long)ar * g.lda + dc) * 4);
        vow[q] = (unsigned)(((long)wr * g.ldw + dc) * 4);
    }
    const unsigned lds0 = (unsigned)(size_t)smem + (unsigned)(16 * wave_u) * BK * 4;
    auto issue = [&](int kt) {
        const unsigned l = lds0 + (unsigned)(kt & (SRING - 1)) * (2 * SM * BK * 4);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            dma16(voa[q], Ab + kt * BK, l + q * 8 * BK * 4);
            dma16(vow[q], Wb + kt * BK, l + SM * BK * 4 + q * 8 * BK * 4);
        }
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int nk = g.K / BK;
    const int frow = lane & 31, hf = lane >> 5, sw = frow & 7;
    // epilogue operands (bias, row-periodic table, residual) are requested before anything else: by the end of the k-loop
    // they sit in registers instead of costing a memory round trip between the last MFMA and the stores.  (Older than
    // every DMA, so they never stand between a counted wait and the stage it waits for.)
    const int me = min(row0 + wm * 32 + frow, g.M - 1);
    const long rgs = g.r_gstride >= 0 ? g.r_gstride : g.c_gstride;
    f32x4 pb[4], pa[4], pr[4];
    if constexpr (VEC) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = tn * SN + wn * 32 + 8 * q + 4 * hf;
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            pb[q] = g.bias ? *reinterpret_cast<const f32x4*>(g.bias + (long)grp * g.b_gstride + n) : z;
            pa[q] = g.add ? *reinterpret_cast<const f32x4*>(g.add + (long)(me % g.add_mod) * g.ld_add + n) : z;
            pr[q] = g.R ? *reinterpret_cast<const f32x4*>(g.R + (long)grp * rgs + (long)me * g.ldr + g.c_col + n) : z;
        }
    }
    for (int kt = 0; kt < SRING - 1 && kt < nk; ++kt) issue(kt);
    for (int kt = 0; kt < nk; ++kt) {
        // this wave's DMAs of stage kt have landed when at most the 4 * (stages issued beyond kt) later ones are in flight
        const int ahead = min(nk - 1 - kt, SRING - 2);
        if (ahead == 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else if (ahead == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                          // every wave's part of stage kt is in LDS; every wave is done reading stage kt-1
        if (kt + SRING - 1 < nk) issue(kt + SRING - 1);      // into the buffer of stage kt-1
        const float* St = smem + (kt & (SRING - 1)) * (2 * SM * BK);
        const float* At = St + (wm * 32 + frow) * BK;
        const float* Bt = St + SM * BK + (wn * 32 + frow) * BK;
        // all 8 fragment reads of the k-tile are requested up front (the scheduler otherwise sinks each pair to its use
        // and exposes the LDS latency four times per k-tile)
        f32x4 fa[4], fb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int pos = ((2 * j + hf) ^ sw) * 4;
            fa[j] = *reinterpret_cast<const f32x4*>(At + pos);
            fb[j] = *reinterpret_cast<const f32x4*>(Bt + pos);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fb[j][i], fa[j][i], acc, 0, 0, 0);
    }
    const int m = row0 + wm * 32 + frow;
    if (m >= g.M) return;
    float* crow = g.C + (long)grp * g.c_gstride + (long)m * g.ldc + g.c_col;
    const float* rrow = g.R ? g.R + (long)grp * rgs + (long)m * g.ldr + g.c_col : nullptr;
    const float* arow = g.add ? g.add + (long)(m % g.add_mod) * g.ld_add : nullptr;      // row-periodic table (pose encoder)
    const float* bias = g.bias ? g.bias + (long)grp * g.b_gstride : nullptr;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int n = tn * SN + wn * 32 + 8 * q + 4 * hf;
        f32x4 v = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
        if constexpr (VEC) {
            v += pb[q];
            v += pa[q];
            v += pr[q];
            *reinterpret_cast<f32x4*>(crow + n) = v;
            if (g.dup_rows) *reinterpret_cast<f32x4*>(crow + g.dup_rows * g.ldc + n) = v;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (n + i >= g.N) continue;
                float x = v[i];
                if (bias) x += bias[n + i];
                if (arow) x += arow[n + i];
                if (rrow) x += rrow[n + i];
                crow[n + i] = x;
                if (g.dup_rows) crow[g.dup_rows * g.ldc + n + i] = x;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// gemm_small_k on 64 x (16 NBLK) tiles (NBLK = 3: 64 x 48, NBLK = 6: 64 x 96) with v_mfma_f32_16x16x4_f32: wave w owns rows
// [16 w, 16 w + 16) of the tile and all NBLK 16-column blocks (one A fragment feeds NBLK MFMAs).  Small-M launches are
// bound by the MFMA pipe of the CUs that HAVE a tile -- at M = 392, N = 1536 the 64 x 64 grid is 168 workgroups on 256
// CUs -- so the tile width is chosen per launch to even out the work per CU (mc_launch_gemm_small): 224 tiles of 64 x 48
// there, 3/4 of the MFMA chain per CU.  Same DMA ring as gemm_small_k.  Fragments: lane -> row (lane & 15), k-group
// lane >> 4; C^T block: lane holds row (lane & 15), columns 16 blk + 4 (lane >> 4) + 0..3.
// (the k accumulation order differs from gemm_small_k's: results agree to fp32 round-off, not bit for bit)
// ---------------------------------------------------------------------------------------
template <int NBLK, bool VEC>
__global__ __launch_bounds__(256) void gemm_small16_k(GemmArgs g) {
    constexpr int NB = 16 * NBLK, NWP = NB / 8;               // W slab rows, 8-row DMA pieces of the W slab
    constexpr int STAGE = (SM + NB) * BK;                     // floats per stage
    __shared__ __attribute__((aligned(16))) float smem[SRING * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ntn = (g.N + NB - 1) / NB;
    const int bid = (g.tune & kTuneSmallXcd) ? xcd_remap((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;      // (XCD-aware tile order: see gemm_small_k)
    const int tm = bid / ntn, tn = bid % ntn, grp = blockIdx.y;
    const int row0 = tm * SM;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int dr = lane >> 3, dc = ((lane & 7) ^ dr) * 4;
    const float* Ab = g.A + (long)grp * g.a_gstride + g.a_col;
    const float* Wb = g.W + (long)grp * g.w_gstride;
    // A slab: pieces 2 wave, 2 wave + 1; W slab: pieces wave, wave + 4, wave + 8 (< NWP)
    constexpr int MAXW = (NWP + 3) / 4;
    unsigned voa[2], vow[MAXW];
#pragma unroll
    for (int q = 0; q < 2; ++q) voa[q] = (unsigned)(((long)min(row0 + 16 * wave + 8 * q + dr, g.M - 1) * g.lda + dc) * 4);
#pragma unroll
    for (int q = 0; q < MAXW; ++q) vow[q] = (unsigned)(((long)min(tn * NB + 8 * (wave + 4 * q) + dr, g.N - 1) * g.ldw + dc) * 4);
    const int nw = (NWP - wave_u + 3) / 4;                    // W pieces of this wave (uniform)
    const unsigned lds_base = (unsigned)(size_t)smem;
    auto issue = [&](int kt) {
        const unsigned l = lds_base + (unsigned)(kt & (SRING - 1)) * (STAGE * 4);
#pragma unroll
        for (int q = 0; q < 2; ++q) dma16(voa[q], Ab + kt * BK, l + (unsigned)(16 * wave_u + 8 * q) * BK * 4);
#pragma unroll
        for (int q = 0; q < MAXW; ++q)
            if (q < nw) dma16(vow[q], Wb + kt * BK, l + SM * BK * 4 + (unsigned)(8 * (wave_u + 4 * q)) * BK * 4);
    };
    f32x4 acc[NBLK];
#pragma unroll
    for (int b = 0; b < NBLK; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nk = g.K / BK;
    const int frow = lane & 15, kg = lane >> 4;
    const int per = 2 + nw;                                   // DMAs of this wave per stage
    const int sw = frow & 7;                                  // (16 wave and 16 blk are multiples of 8)
    // epilogue operands first (see gemm_small_k)
    const int me = min(row0 + 16 * wave + frow, g.M - 1);
    const long rgs = g.r_gstride >= 0 ? g.r_gstride : g.c_gstride;
    f32x4 pb[NBLK], pa[NBLK], pr[NBLK];
    if constexpr (VEC) {
#pragma unroll
        for (int b = 0; b < NBLK; ++b) {
            const int n = tn * NB + 16 * b + 4 * kg;
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            pb[b] = g.bias ? *reinterpret_cast<const f32x4*>(g.bias + (long)grp * g.b_gstride + n) : z;
            pa[b] = g.add ? *reinterpret_cast<const f32x4*>(g.add + (long)(me % g.add_mod) * g.ld_add + n) : z;
            pr[b] = g.R ? *reinterpret_cast<const f32x4*>(g.R + (long)grp * rgs + (long)me * g.ldr + g.c_col + n) : z;
        }
    }
    for (int kt = 0; kt < SRING - 1 && kt < nk; ++kt) issue(kt);
    for (int kt = 0; kt < nk; ++kt) {
        switch (min(nk - 1 - kt, SRING - 2) * per) {          // this wave's DMAs issued after those of stage kt
            case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
            case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
            case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
            case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
            case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
            case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
            default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        }
        __syncthreads();
        if (kt + SRING - 1 < nk) issue(kt + SRING - 1);
        const float* St = smem + (kt & (SRING - 1)) * STAGE;
        const float* At = St + (16 * wave + frow) * BK;
        const float* Bt = St + SM * BK + frow * BK;
        f32x4 fa[2], fb[NBLK][2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int pos = ((4 * j + kg) ^ sw) * 4;
            fa[j] = *reinterpret_cast<const f32x4*>(At + pos);
#pragma unroll
            for (int b = 0; b < NBLK; ++b) fb[b][j] = *reinterpret_cast<const f32x4*>(Bt + b * 16 * BK + pos);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int b = 0; b < NBLK; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fb[b][j][i], fa[j][i], acc[b], 0, 0, 0);
    }
    const int m = row0 + 16 * wave + frow;
    if (m >= g.M) return;
    float* crow = g.C + (long)grp * g.c_gstride + (long)m * g.ldc + g.c_col;
    const float* rrow = g.R ? g.R + (long)grp * rgs + (long)m * g.ldr + g.c_col : nullptr;
    const float* arow = g.add ? g.add + (long)(m % g.add_mod) * g.ld_add : nullptr;
    const float* bias = g.bias ? g.bias + (long)grp * g.b_gstride : nullptr;
#pragma unroll
    for (int b = 0; b < NBLK; ++b) {
        const int n = tn * NB + 16 * b + 4 * kg;
        f32x4 v = acc[b];
        if constexpr (VEC) {
            v += pb[b];
            v += pa[b];
            v += pr[b];
            *reinterpret_cast<f32x4*>(crow + n) = v;
            if (g.dup_rows) *reinterpret_cast<f32x4*>(crow + g.dup_rows * g.ldc + n) = v;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (n + i >= g.N) continue;
                float x = v[i];
                if (bias) x += bias[n + i];
                if (arow) x += arow[n + i];
                if (rrow) x += rrow[n + i];
                crow[n + i] = x;
                if (g.dup_rows) crow[g.dup_rows * g.ldc + n + i] = x;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// gemm_tail_k: the folded decoder tail of the large-batch schedule as ONE pass (round 4; stmogen.py:505-544, 757-760):
//     x0[r] = (w_c h[r] + w_u h[r + half]) W0^T + (w_c a[r] + w_u a[r + half]) W1^T + b0 + b1
// gemm_small16_k's tile (64 x 16 NBLK, v_mfma_f32_16x16x4_f32, W slabs by LDS-DMA into the same ring) with
//   * the CFG combination formed while the A slab is staged (two global loads + 2 VALU ops per element through registers, written
//     into the image the DMA would have produced): no axpby_pair_k pass, h_c / a_c never exist in HBM
//   * both K groups walked by one accumulator (k-tiles of h, then of a): one output, no partial sums for the sampler kernel
// Order of a wave's vector-memory ops per iteration: [A loads of tile kt + 3] [W DMAs of stage kt + 3]; at the top of iteration kt
// everything up to the A loads of tile kt + 1 must have landed (in-order vmcnt): s_waitcnt vmcnt(W(kt+1) A(kt+2) W(kt+2) = 2 nw + 4).
// ---------------------------------------------------------------------------------------
// 16-byte global load the compiler does not track: its own s_waitcnt placement counts only the loads it knows, not the LDS-DMAs
// issued between them, and would drain the whole queue (vmcnt(0)) in front of the first use.  The caller waits by count.
__device__ __forceinline__ void gload16(f32x4& v, const float* p) {
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(v) : "v"(p) : "memory");
}

// s_waitcnt vmcnt(n) for a wave-uniform n computed from the pipeline's own counts (the hand-counted waits of the tail kernels: in-order
// vmcnt, "everything but the n youngest operations has landed")
__device__ __forceinline__ void vm_wait(int n) {
    switch (n) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
        case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
        case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
        case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
        case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); break;
        case 12: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
        case 13: asm volatile("s_waitcnt vmcnt(13)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(14)" ::: "memory"); break;      // (n >= 14: waiting for more than asked is always safe)
    }
}

// ROWS (mc_sample_rows): the CFG weights per request row -- A slab row r takes coef_table[((min(r, M - 1) / rows_T)
// % rows_B) coef_stride + {0, 1}].  A thread's slab rows are fixed before the k-loop, so its two pairs are fetched once (tracked loads, landed
// before the first counted load is issued: the hand-counted waits see the queue they were counted for) and the loop keeps its shape.
// ROWS = false is the kernel as it was (TailArgs keeps its size and offsets: rows_T / rows_B sit in its two padding words).
template <int NBLK, bool ROWS = false>
__global__ __launch_bounds__(256) void gemm_tail_k(TailArgs g) {
    constexpr int NB = 16 * NBLK, NWP = NB / 8;
    constexpr int STAGE = (SM + NB) * BK;
    __shared__ __attribute__((aligned(16))) float smem[SRING * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ntn = (g.N + NB - 1) / NB;
    const int bid = (g.tune & kTuneSmallXcd) ? xcd_remap((int)blockIdx.x, (int)gridDim.x) : (int)blockIdx.x;
    const int tm = bid / ntn, tn = bid % ntn;
    const int row0 = tm * SM;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    float wc = g.wc, wu = g.wu;
    if (!ROWS && g.coef_table) { wc = g.coef_table[(long)*g.step_ptr * g.coef_stride]; wu = g.coef_table[(long)*g.step_ptr * g.coef_stride + 1]; }
    // A slab slots of this thread: (row, 16-byte position) = ((tid + 256 j) >> 3, (tid + 256 j) & 7); position p of row r holds chunk p ^ (r & 7)
    long aoff[2];
    int alds[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int i = tid + 256 * j, row = i >> 3, pos = i & 7;
        aoff[j] = (long)min(row0 + row, g.M - 1) * g.lda + ((pos ^ (row & 7)) << 2);
        alds[j] = row * BK + (pos << 2);
    }
    float wcr[2] = {wc, wc}, wur[2] = {wu, wu};
    if constexpr (ROWS) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const long rb = (min(row0 + ((tid + 256 * j) >> 3), g.M - 1) / g.rows_T) % g.rows_B;
            wcr[j] = g.coef_table[rb * g.coef_stride];
            wur[j] = g.coef_table[rb * g.coef_stride + 1];
        }
        asm volatile("" : "+v"(wcr[0]), "+v"(wcr[1]), "+v"(wur[0]), "+v"(wur[1]));
    }
    const int dr = lane >> 3, dc = ((lane & 7) ^ dr) * 4;
    constexpr int MAXW = (NWP + 3) / 4;
    unsigned vow[MAXW];
#pragma unroll
    for (int q = 0; q < MAXW; ++q) vow[q] = (unsigned)(((long)min(tn * NB + 8 * (wave + 4 * q) + dr, g.N - 1) * g.ldw + dc) * 4);
    const int nw = (NWP - wave_u + 3) / 4;                    // W pieces of this wave (uniform)
    const unsigned lds_base = (unsigned)(size_t)smem;
    const int nk = g.K / BK, NK = 2 * nk;
    auto a_load = [&](int kt, f32x4 (&c)[2], f32x4 (&u)[2]) {
        const float* A = (kt < nk ? g.H : g.Af) + (long)(kt < nk ? kt : kt - nk) * BK;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            gload16(c[j], A + aoff[j]);
            gload16(u[j], A + g.half + aoff[j]);
        }
    };
    auto a_store = [&](int kt, const f32x4 (&c)[2], const f32x4 (&u)[2]) {
        float* St = smem + (kt & (SRING - 1)) * STAGE;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            f32x4 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = wcr[j] * c[j][i] + wur[j] * u[j][i];
            *reinterpret_cast<f32x4*>(St + alds[j]) = v;
        }
    };
    auto w_issue = [&](int kt) {
        const float* Wb = g.W + (kt < nk ? 0 : g.w_gstride) + (long)(kt < nk ? kt : kt - nk) * BK;
        const unsigned l = lds_base + (unsigned)(kt & (SRING - 1)) * (STAGE * 4) + SM * BK * 4;
#pragma unroll
        for (int q = 0; q < MAXW; ++q)
            if (q < nw) dma16(vow[q], Wb, l + (unsigned)(8 * (wave_u + 4 * q)) * BK * 4);
    };
    f32x4 acc[NBLK];
#pragma unroll
    for (int b = 0; b < NBLK; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int frow = lane & 15, kg = lane >> 4;
    const int sw = frow & 7;
    // three A register sets in rotation (tile k lives in set k % 3): a tile is requested three iterations before it is written into its
    // LDS stage (one iteration of 24 MFMAs is ~0.3 us, a round trip to L2 / HBM several times that)
    f32x4 c0[2], u0[2], c1[2], u1[2], c2[2], u2[2];
    a_load(0, c0, u0);
    w_issue(0);
    if (NK > 1) { a_load(1, c1, u1); w_issue(1); }
    if (NK > 2) { a_load(2, c2, u2); w_issue(2); }
    // A(0) has landed once at most W0 A1 W1 A2 W2 are outstanding (NK >= 3 for every model width; otherwise wait for everything)
    constexpr int A_OPS = 4;                                  // vector-memory operations of one a_load: 2 slots x (conditional + unconditional row)
    static_assert(NWP <= 8, "a wave issues at most two W pieces per stage: the counted waits below assume nw <= 2");
    vm_wait(NK > 2 ? 3 * nw + 2 * A_OPS : 0);
    asm volatile("" : "+v"(c0[0]), "+v"(c0[1]), "+v"(u0[0]), "+v"(u0[1]));      // (the loaded set is consumed only behind the wait: ADVICE r04)
    a_store(0, c0, u0);
    // one iteration: stage kt is consumed; A(kt + 1) (set `st`) goes into its LDS stage; A(kt + 3) is requested into the set tile kt used
    auto step = [&](int kt, f32x4 (&cs)[2], f32x4 (&us)[2], f32x4 (&cl)[2], f32x4 (&ul)[2]) {
        // everything up to A(kt + 1) has landed once only W(kt+1) A(kt+2) W(kt+2) are outstanding
        vm_wait(kt + 2 < NK ? 2 * nw + A_OPS : 0);
        asm volatile("" : "+v"(cs[0]), "+v"(cs[1]), "+v"(us[0]), "+v"(us[1]));
        __syncthreads();
        if (kt + 1 < NK) a_store(kt + 1, cs, us);
        if (kt + 3 < NK) { a_load(kt + 3, cl, ul); w_issue(kt + 3); }
        const float* St = smem + (kt & (SRING - 1)) * STAGE;
        const float* At = St + (16 * wave + frow) * BK;
        const float* Bt = St + SM * BK + frow * BK;
        f32x4 fa[2], fb[NBLK][2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int pos = ((4 * j + kg) ^ sw) * 4;
            fa[j] = *reinterpret_cast<const f32x4*>(At + pos);
#pragma unroll
            for (int b = 0; b < NBLK; ++b) fb[b][j] = *reinterpret_cast<const f32x4*>(Bt + b * 16 * BK + pos);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int b = 0; b < NBLK; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fb[b][j][i], fa[j][i], acc[b], 0, 0, 0);
    };
    for (int kt = 0; kt < NK; kt += 3) {
        step(kt, c1, u1, c0, u0);
        if (kt + 1 < NK) step(kt + 1, c2, u2, c1, u1);
        if (kt + 2 < NK) step(kt + 2, c0, u0, c2, u2);
    }
    const int m = row0 + 16 * wave + frow;
    if (m >= g.M) return;
    float* crow = g.C + (long)m * g.ldc;
#pragma unroll
    for (int b = 0; b < NBLK; ++b) {
        const int n = tn * NB + 16 * b + 4 * kg;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (n + i >= g.N) continue;
            crow[n + i] = acc[b][i] + (g.bias[n + i] + g.bias[g.b_gstride + n + i]);
        }
    }
}

// ---------------------------------------------------------------------------------------
// gemm_tail2_k (round 5): the same folded decoder tail, A read ONCE.  gemm_tail_k cuts N = 322 into seven 48-wide column tiles and every
// one of them re-reads (and re-combines) the A rows: 548 MB fetched per launch against the 308 MB of h and a (both CFG halves) + 4 MB of
// W, 0.48 of the MFMA peak.  Here the launch is a flat list of 16 x 16 output blocks in row-tile-major order (784 row tiles x 21 column
// blocks at B = 64) cut into one CONTIGUOUS range per workgroup, one workgroup per CU (the stream-K idea applied to blocks: 12544 rows
// are 49 per CU, so whole row tiles per workgroup can only reach 77 % of the CUs' MFMA time; ranges of 64 / 65 blocks reach 98 %).
// A workgroup stages the <= 5 row tiles its range touches (CFG combination formed in registers on the way, as in gemm_tail_k) and ALL
// column blocks of W per k-tile, so A is fetched once per workgroup and W streams from L2.  The two K groups (h x W0, a x W1) are TWO
// workgroups over the same range (two per CU, 78 KB of LDS each: they drift freely and cover each other's barrier / issue phases; a first
// version with both groups as wave quads of one 512-thread workgroup met at one barrier per k-tile and ran at half this speed); each
// writes its partial product (C, C2), which the sampler-update kernel adds -- the x0a + x0b form it already had for the grouped tail.
// Inside a workgroup the range is cut into four contiguous pieces of <= NBW + 1 blocks, one per wave; every block reads its own A fragment
// (a scalar offset picks the row tile: no per-block register select; 34 ds_read_b128 per 64 MFMAs = a quarter of the LDS read rate).
// k-tiles of 16 columns; LDS stage of a quad = [80 A rows | 336 W rows][16 floats], 16-byte chunk c of row r at position c ^ F[(r >> 2) & 3],
// F = {0, 2, 3, 1}: conflict-free for the 16 x 16 fragment read (lane = row l & 15, chunk l >> 4) in ds_read_b128's lane groups.
// Ring of 3 stages = 78 KB.  Per iteration kt a wave issues [A loads of tile kt + 3][W DMAs of tile kt + 2]; at its top
// A(kt + 1) and W(kt) must have landed: everything but the previous iteration's na + nwp operations (in-order vmcnt).
// ---------------------------------------------------------------------------------------
constexpr int T2_BK = 16, T2_MAXCB = 21, T2_MAXRT = 5, T2_RING = 3;
constexpr int T2_STAGE = 16 * (T2_MAXRT + T2_MAXCB) * T2_BK;            // floats per stage (26 KB)
constexpr int T2_WROW0 = 16 * T2_MAXRT;                                 // first W row of a stage

__device__ __forceinline__ int t2_swz(int row) { return (0x78 >> (2 * ((row >> 2) & 3))) & 3; }      // F = {0, 2, 3, 1}, two bits each: 0b01111000 >> {0, 2, 4, 6}

template <int NBW, bool ROWS = false>        // blocks per wave handled by the static part (a wave's piece has <= NBW + 1 blocks); ROWS: as in gemm_tail_k
__global__ __launch_bounds__(256, 2) void gemm_tail2_k(TailArgs g, int ncb, long nblocks) {
    static_assert(NBW % 4 == 0 && NBW >= 4 && NBW <= 16, "NBW");
    constexpr int PH = 4;                                                // blocks per fragment phase (8 spills address registers at NBW = 16, and spill reloads share the vmcnt queue)
    __shared__ __attribute__((aligned(16))) float smem[T2_RING * T2_STAGE];      // 78 KB: two workgroups per CU
    const int tid = threadIdx.x, lane = tid & 63;
    const int qw = __builtin_amdgcn_readfirstlane(tid >> 6);
    float wc = g.wc, wu = g.wu;
    if (!ROWS && g.coef_table) { wc = g.coef_table[(long)*g.step_ptr * g.coef_stride]; wu = g.coef_table[(long)*g.step_ptr * g.coef_stride + 1]; }
    // workgroup -> (block range, K group); consecutive ranges (neighbouring rows) share an XCD's L2
    const int G = gridDim.x >> 1, rid = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    const int wg = rid >> 1, grp = rid & 1;
    const long gb0 = nblocks * wg / G, gb1 = nblocks * (wg + 1) / G;
    const int n = (int)(gb1 - gb0);
    if (n <= 0) return;
    const int rt_first = (int)(gb0 / ncb), nrt = (int)((gb1 - 1) / ncb) - rt_first + 1;      // <= T2_MAXRT (launcher)
    // this wave's piece
    const int wb0 = qw * n / 4, wb1 = (qw + 1) * n / 4, nb = wb1 - wb0;                        // <= NBW + 1 (launcher)
    const int frow = lane & 15, kg = lane >> 4;
    const int lfrag = frow * T2_BK + ((kg ^ t2_swz(frow)) << 2);                               // lane part of a fragment address (floats)
    const int g0 = (int)(gb0 - (long)rt_first * ncb) + wb0;                                    // first block of the piece, relative to the range's first row tile
    int aoff[NBW + 1], boff[NBW + 1];                                                          // per block: its A row tile / W column block inside a stage
    {
        // (one division per wave, then a walk: blocks past the piece repeat its last one -- computed, never stored)
        int rt = g0 / ncb, cb = g0 - rt * ncb;
#pragma unroll
        for (int b = 0; b <= NBW; ++b) {
            aoff[b] = rt * 16 * T2_BK;
            boff[b] = (T2_WROW0 + 16 * cb) * T2_BK;
            if (b + 1 < nb) { if (++cb == ncb) { cb = 0; ++rt; } }
        }
    }
    // ---- A staging: 16-byte slot s = (row s >> 2, position s & 3), s = tid (+ 256 for the fifth row tile) ----
    const float* Asrc = grp ? g.Af : g.H;
    long a_go[2];
    int a_lds[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int s = tid + 256 * j, row = s >> 2, pos = s & 3;
        long grow = (long)rt_first * 16 + row;
        if (grow > g.M - 1) grow = g.M - 1;
        a_go[j] = grow * g.lda + ((pos ^ t2_swz(row)) << 2);
        a_lds[j] = row * T2_BK + (pos << 2);
    }
    float wcr[2] = {wc, wc}, wur[2] = {wu, wu};
    if constexpr (ROWS) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            long grow = (long)rt_first * 16 + ((tid + 256 * j) >> 2);
            if (grow > g.M - 1) grow = g.M - 1;
            const long rb = (grow / g.rows_T) % g.rows_B;
            wcr[j] = g.coef_table[rb * g.coef_stride];
            wur[j] = g.coef_table[rb * g.coef_stride + 1];
        }
        asm volatile("" : "+v"(wcr[0]), "+v"(wcr[1]), "+v"(wur[0]), "+v"(wur[1]));
    }
    const int nslot = (qw < nrt ? 1 : 0) + ((4 + qw) < nrt ? 1 : 0);                           // slots of this wave's threads (uniform): 64 slots per row tile
    const int na = 2 * nslot;
    // ---- W DMA: piece p = rows [16 p, 16 p + 16) of the group's weight, pieces qw, qw + 4, ... of this wave ----
    constexpr int MAXP = (T2_MAXCB + 3) / 4;
    unsigned vow[MAXP];
    {
        const int dr = lane >> 2, pos = lane & 3;
#pragma unroll
        for (int q = 0; q < MAXP; ++q) {
            int wr = 16 * (qw + 4 * q) + dr;
            if (wr > g.N - 1) wr = g.N - 1;
            vow[q] = (unsigned)(((long)wr * g.ldw + ((pos ^ t2_swz(dr)) << 2)) * 4);
        }
    }
    const int nwp = qw < ncb ? (ncb - qw + 3) / 4 : 0;
    const float* Wsrc = g.W + (grp ? g.w_gstride : 0);
    const unsigned lds_q = (unsigned)(size_t)smem;
    const int nk = g.K / T2_BK;
    auto a_load = [&](int kt, f32x4 (&c)[2], f32x4 (&u)[2]) {
        const float* A = Asrc + (long)kt * T2_BK;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (j < nslot) { gload16(c[j], A + a_go[j]); gload16(u[j], A + g.half + a_go[j]); }
    };
    auto a_store = [&](int kt, const f32x4 (&c)[2], const f32x4 (&u)[2]) {
        float* St = smem + (kt % T2_RING) * T2_STAGE;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (j < nslot) {
                f32x4 v;
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = wcr[j] * c[j][i] + wur[j] * u[j][i];
                *reinterpret_cast<f32x4*>(St + a_lds[j]) = v;
            }
    };
    auto w_issue = [&](int kt) {
        const float* Wb = Wsrc + (long)kt * T2_BK;
        const unsigned l = lds_q + (unsigned)((kt % T2_RING) * T2_STAGE + T2_WROW0 * T2_BK) * 4;
#pragma unroll
        for (int q = 0; q < MAXP; ++q)
            if (q < nwp) dma16(vow[q], Wb, l + (unsigned)(16 * (qw + 4 * q)) * T2_BK * 4);
    };
    f32x4 acc[NBW + 1];
#pragma unroll
    for (int b = 0; b <= NBW; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
    // two A register sets in rotation: tile k lives in set k & 1, requested three iterations before it is consumed
    f32x4 c0[2], u0[2], c1[2], u1[2];
    a_load(0, c0, u0);
    vm_wait(0);
    asm volatile("" : "+v"(c0[0]), "+v"(c0[1]), "+v"(u0[0]), "+v"(u0[1]));
    a_store(0, c0, u0);
    a_load(1, c1, u1);
    w_issue(0);
    if (nk > 2) a_load(2, c0, u0);
    if (nk > 1) w_issue(1);
    // queue now: A(1) W(0) A(2) W(1)
    auto step = [&](int kt, f32x4 (&cs)[2], f32x4 (&us)[2]) {
        // A(kt + 1) and W(kt) have landed once only the previous iteration's issues -- A(kt + 2), W(kt + 1) -- are outstanding
        vm_wait((kt + 2 < nk ? na : 0) + (kt + 1 < nk ? nwp : 0));
        asm volatile("" : "+v"(cs[0]), "+v"(cs[1]), "+v"(us[0]), "+v"(us[1]));              // (the set is consumed only behind the wait)
        if (kt + 1 < nk) a_store(kt + 1, cs, us);
        __syncthreads();
        if (kt + 3 < nk) a_load(kt + 3, cs, us);                                              // (set (kt + 1) & 1 is free again)
        if (kt + 2 < nk) w_issue(kt + 2);
        const float* St = smem + (kt % T2_RING) * T2_STAGE + lfrag;
#pragma unroll
        for (int p0 = 0; p0 < NBW; p0 += PH) {
            f32x4 fa[PH], fb[PH];
#pragma unroll
            for (int b = 0; b < PH; ++b) {
                fa[b] = *reinterpret_cast<const f32x4*>(St + aoff[p0 + b]);
                fb[b] = *reinterpret_cast<const f32x4*>(St + boff[p0 + b]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int b = 0; b < PH; ++b)
                    acc[p0 + b] = __builtin_amdgcn_mfma_f32_16x16x4f32(fb[b][i], fa[b][i], acc[p0 + b], 0, 0, 0);
        }
        if (nb > NBW) {          // the piece's extra block (uniform branch)
            const f32x4 fa = *reinterpret_cast<const f32x4*>(St + aoff[NBW]);
            const f32x4 fb = *reinterpret_cast<const f32x4*>(St + boff[NBW]);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[NBW] = __builtin_amdgcn_mfma_f32_16x16x4f32(fb[i], fa[i], acc[NBW], 0, 0, 0);
        }
    };
    for (int kt = 0; kt < nk; kt += 2) {
        step(kt, c1, u1);
        if (kt + 1 < nk) step(kt + 1, c0, u0);
    }
    // ---- this K group's partial product: group 0 -> C (+ both biases), group 1 -> C2; the sampler kernel adds the two ----
    float* Cout = grp ? g.C2 : g.C;
    {
        int rt = g0 / ncb, cb = g0 - rt * ncb;
#pragma unroll
        for (int b = 0; b <= NBW; ++b) {
            if (b < nb) {
                const long m = ((long)rt_first + rt) * 16 + frow;
                const int n0 = cb * 16 + 4 * kg;
                if (m < g.M) {
                    float* crow = Cout + m * g.ldc;
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (n0 + i < g.N) crow[n0 + i] = grp ? acc[b][i] : acc[b][i] + (g.bias[n0 + i] + g.bias[g.b_gstride + n0 + i]);
                }
                if (++cb == ncb) { cb = 0; ++rt; }
            }
        }
    }
}

}  // namespace

// launch options left at their GemmArgs defaults (context-free launches: mc_op_*, the encoders) come from the process options
static int resolve_opts(GemmArgs& g) {
    if (g.tune >= 0 && g.small_tile_n && g.wp_grid) return MC_OK;
    const McOptions* o = mc_process_options();
    if (!o) return MC_ERR_ARG;
    GemmArgs p;
    mc_gemm_opts(*o, p);
    g.tune = g.tune < 0 ? p.tune : g.tune;
    g.small_tile_n = g.small_tile_n ? g.small_tile_n : p.small_tile_n;
    g.wp_grid = g.wp_grid ? g.wp_grid : p.wp_grid;
    return MC_OK;
}
int mc_launch_gemm_small(const GemmArgs& g, hipStream_t stream, int groups) {
    MC_REQUIRE(g.K % BK == 0 && g.lda % 4 == 0 && g.ldw % 4 == 0 && g.a_col % 4 == 0 && g.a_gstride % 4 == 0 && g.w_gstride % 4 == 0 &&
                   g.act == ACT_NONE,
               "gemm_small: unsupported shape / options (M=%d N=%d K=%d)", g.M, g.N, g.K);
    if (g.M <= 0 || g.N <= 0) return MC_OK;
    MC_REQUIRE((long)g.M * g.lda * 4 < (1L << 32) && (long)g.N * g.ldw * 4 < (1L << 32),
               "gemm_small: operands beyond 4 GB (the DMA takes 32-bit byte offsets into A and W; this kernel is for a few thousand rows)");
    const bool vec = g.N % SN == 0 && g.ldc % 4 == 0 && g.c_col % 4 == 0 && g.c_gstride % 4 == 0 && (!g.R || (g.ldr % 4 == 0 && (g.r_gstride < 0 || g.r_gstride % 4 == 0))) &&
                     (!g.add || g.ld_add % 4 == 0) && g.b_gstride % 4 == 0;
    // Tile width per launch.  The launch is bound by the MFMA pipe of the busiest CU: mc_cu_load (mc_gemm.h) gives its load
    // in tile times; a 64 x 48 / 64 x 64 / 64 x 96 tile costs 23 / 30 / 41 units (the 32x32-MFMA
    // kernel is ~15 % more efficient per flop than the 16x16 one).  Fitted on 392 B x 1536 x 1536 for B = 1 .. 16
    // (tools/gemm_sweep.py): picks the measured-best width in every case, e.g. 48 at B = 1, 2, 7, 96 at B = 4, 5, 10, else 64.
    // (only widths that divide N: the decoder tail, N = 322, would be 7 x 48 instead of 6 x 64 tiles and 5 us faster at B=1,
    // but the 16x16 kernel accumulates k in another order, and that 1-ulp change of the decoded x0 was enough to move a
    // near-tie gate decision of the free-running full-size 50-step golden -- 0.63 off the reference's final pose with
    // per-step parity at 6e-6; the 64-wide kernel keeps the trajectory the golden test pins)
    const int ng = groups > 0 ? groups : 1;
    GemmArgs gg = g;
    if (int r = resolve_opts(gg)) return r;
    auto cost = [&](int nb, double unit) { return mc_cu_load((long)cdiv(g.M, SM) * cdiv(g.N, nb) * ng) * unit; };
    int nb = SN;
    double best = cost(SN, 30.0);
    // (beyond the small-batch sizes -- M > 6400 rows, i.e. the folded decoder tail of a large batch, whose goldens are lockstep
    //  comparisons and not free-running trajectories -- any width may be taken: N = 322 as 7 x 48 = 336 columns instead of 6 x 64 = 384)
    const bool any_width = g.M > 6400;
    if ((g.N % 48 == 0 || any_width) && cost(48, 23.0) < 0.97 * best) { nb = 48; best = cost(48, 23.0); }     // (3 % margin: near ties go to the more efficient kernel)
    if ((g.N % 96 == 0 || any_width) && cost(96, 41.0) < 0.97 * best) { nb = 96; best = cost(96, 41.0); }
    if (gg.small_tile_n == 64 || gg.small_tile_n == 48 || gg.small_tile_n == 96) nb = gg.small_tile_n;
    dim3 grid(cdiv(g.M, SM) * cdiv(g.N, nb), ng);
    const bool vec16 = vec && g.N % nb == 0;       // the float4 epilogue has no column guard
    MC_LEDGER(nb == 48 ? "gemm_small16_k<3" : nb == 96 ? "gemm_small16_k<6" : "gemm_small_k", grid, 2.0 * g.M * g.N * g.K * ng);
    if (nb == 48) {
        if (vec16) hipLaunchKernelGGL((gemm_small16_k<3, true>), grid, dim3(256), 0, stream, gg);
        else hipLaunchKernelGGL((gemm_small16_k<3, false>), grid, dim3(256), 0, stream, gg);
    } else if (nb == 96) {
        if (vec16) hipLaunchKernelGGL((gemm_small16_k<6, true>), grid, dim3(256), 0, stream, gg);
        else hipLaunchKernelGGL((gemm_small16_k<6, false>), grid, dim3(256), 0, stream, gg);
    } else {
        if (vec) hipLaunchKernelGGL(gemm_small_k<true>, grid, dim3(256), 0, stream, gg);
        else hipLaunchKernelGGL(gemm_small_k<false>, grid, dim3(256), 0, stream, gg);
    }
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int mc_launch_gemm(int mode, const GemmArgs& g0, int groups, int max_tiles, hipStream_t stream) {
    GemmArgs g = g0;
    if (int r = resolve_opts(g)) return r;
    const int ntn = cdiv(g.N, BN);
    int ntm = (mode == GM_EXP1 || mode == GM_EXP2) ? max_tiles : cdiv(g.M, BM);
    if (ntm <= 0 || ntn <= 0) return MC_OK;
    if (mode != GM_ENC) MC_REQUIRE(g.K % 4 == 0 && g.lda % 4 == 0 && g.ldw % 4 == 0, "gemm: K/lda/ldw must be multiples of 4");
    // the row-periodic table and the duplicate rows exist in the vector epilogue only (gemm_k's `vec` condition)
    if (mode == GM_ENC && (g.add || g.dup_rows))
        MC_REQUIRE(g.N % 4 == 0 && g.ldc % 4 == 0 && g.c_col % 4 == 0 && g.c_gstride % 4 == 0 && (!g.add || g.ld_add % 4 == 0) &&
                       (!g.R || (g.ldr % 4 == 0 && (g.r_gstride < 0 || g.r_gstride % 4 == 0))),
                   "gemm: an add table or duplicate rows need 16-byte aligned output rows (N=%d ldc=%ld)", g.N, g.ldc);
    dim3 grid(ntm * ntn, groups > 0 ? groups : 1, 1);
    const bool vec_out = (g.ldc % 4 == 0) && (g.c_col % 4 == 0) && (!g.R || g.ldr % 4 == 0);
    // (GM_ENC with aligned operands -- the padded pose rows of the large-batch encoder -- is a plain GEMM + row-periodic table + duplicate
    //  rows: it takes the wave-private kernel too, tune bit 9; gemm_k<GM_ENC> ran it at 71 TFLOP/s: K = 352 is 11 k-tiles, all prologue)
    const bool wp_ok = (g.tune & kTuneWp) && g.K % WBK == 0 && (long)g.M * g.lda * 4 < (1L << 32) && (long)g.N * g.ldw * 4 < (1L << 32);
    const bool enc_fast = mode == GM_ENC && (g.tune & kTuneEncWp) && wp_ok && !g.R && g.add && g.ld_add % 4 == 0 && g.act == ACT_NONE;
    if ((g.tune & kTuneDma) && (mode == GM_PLAIN || enc_fast) && groups <= 1 && g.M % BM == 0 && g.N % BN == 0 && (g.K % BK == 0 || enc_fast) &&
        g.lda % 4 == 0 && g.ldw % 4 == 0 && g.a_col % 4 == 0 && vec_out && g.act != ACT_QUICKGELU && !g.act_after_res &&
        (enc_fast || (!g.add && !g.dup_rows))) {
        // bit 5: wave-private pipeline variant (no k-loop barrier); needs 32-bit byte offsets into A and W
        if (wp_ok) {
            const int persistent = g.wp_grid > 0 ? g.wp_grid : (int)grid.x;      // default 512: 2 workgroups per CU (64 KB of LDS each) on 256 CUs
            MC_LEDGER("gemm_wp_k", dim3(grid.x < persistent ? grid.x : persistent), 2.0 * g.M * g.N * g.K);
            hipLaunchKernelGGL(gemm_wp_k, dim3(grid.x < persistent ? grid.x : persistent), dim3(256), 0, stream, g);
        } else {
            MC_LEDGER("gemm_dma_k", grid, 2.0 * g.M * g.N * g.K);
            hipLaunchKernelGGL(gemm_dma_k, grid, dim3(256), 0, stream, g);
        }
        MC_LAUNCH_CHECK();
        return MC_OK;
    }
    if (mc_ledger_on) {      // expert modes: booked at the tile capacity of the launch (the real tile count lives on the device)
        char name[24];
        snprintf(name, sizeof(name), "gemm_k<%d>", mode);
        const double rows = (mode == GM_EXP1 || mode == GM_EXP2) ? (double)ntm * BM : (double)g.M;
        MC_LEDGER(name, grid, 2.0 * rows * g.N * g.K * (groups > 0 ? groups : 1));
    }
    switch (mode) {
        case GM_PLAIN: hipLaunchKernelGGL(gemm_k<GM_PLAIN>, grid, dim3(256), 0, stream, g); break;
        case GM_EXP1: hipLaunchKernelGGL(gemm_k<GM_EXP1>, grid, dim3(256), 0, stream, g); break;
        case GM_EXP2: hipLaunchKernelGGL(gemm_k<GM_EXP2>, grid, dim3(256), 0, stream, g); break;
        case GM_COMB: hipLaunchKernelGGL(gemm_k<GM_COMB>, grid, dim3(256), 0, stream, g); break;
        case GM_ENC: hipLaunchKernelGGL(gemm_k<GM_ENC>, grid, dim3(256), 0, stream, g); break;
        default: mc_set_error("bad gemm mode %d", mode); return MC_ERR_ARG;
    }
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int mc_device_cus() {
    static int v = 0;
    if (v <= 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) v = prop.multiProcessorCount;
        if (v <= 0) v = 256;
    }
    return v;
}

// grid of the block-range form for this launch, or 0: the column-tile kernel runs (tune bit 10 off, no second output, N > 336, ranges too long)
static int tail2_grid(const TailArgs& g, int tune, int* per_wave_out) {
    const int ncb = cdiv(g.N, 16);
    const long nblocks = (long)cdiv(g.M, 16) * ncb;
    if (!(tune & kTuneTail2) || !g.C2 || ncb > T2_MAXCB || g.K < 3 * T2_BK || g.K % T2_BK) return 0;
    int G = mc_device_cus();
    if (nblocks < (long)G * 16) G = (int)(nblocks / 16) > 0 ? (int)(nblocks / 16) : 1;          // small launches: >= 16 blocks per workgroup
    else G *= (int)cdiv(nblocks, (long)G * 66);                                                 // large ones: several ranges per CU, each within a wave's 17 blocks
    const int nmax = (int)cdiv(nblocks, (long)G);                                               // largest range; its pieces have <= ceil(nmax / 4) blocks
    const int per_wave = cdiv(nmax, 4);
    const int max_rt = (ncb - 1 + nmax - 1) / ncb + 1;                                          // row tiles a range of nmax blocks can touch
    if (per_wave > 17 || max_rt > T2_MAXRT) return 0;
    if (per_wave_out) *per_wave_out = per_wave;
    return G;
}

bool mc_gemm_tail_two_outputs(const TailArgs& g) { return tail2_grid(g, g.tune, nullptr) > 0; }

// The tail kernels wait for their LDS-DMA pieces with HAND-COUNTED s_waitcnt vmcnt(n) values: correct only while the compiler emits no
// vector-memory instruction of its own inside the k-loop.  A register spill (scratch) would add such instructions and make the loops
// under-wait without any error, so a build whose tail kernels use scratch is refused here, once per process.
static int tail_kernels_scratch_free() {
    static const int verdict = [] {
        const void* fns[] = {(const void*)gemm_tail_k<3>, (const void*)gemm_tail2_k<4>, (const void*)gemm_tail2_k<8>, (const void*)gemm_tail2_k<12>,
                             (const void*)gemm_tail2_k<16>, (const void*)gemm_tail_k<3, true>, (const void*)gemm_tail2_k<4, true>,
                             (const void*)gemm_tail2_k<8, true>, (const void*)gemm_tail2_k<12, true>, (const void*)gemm_tail2_k<16, true>};
        for (const void* f : fns) {
            hipFuncAttributes at;
            if (hipFuncGetAttributes(&at, f) != hipSuccess) return -1;
            if (at.localSizeBytes != 0) return (int)at.localSizeBytes;
        }
        return 0;
    }();
    return verdict;
}

int mc_launch_gemm_tail(const TailArgs& g, hipStream_t stream) {
    MC_REQUIRE(g.H && g.Af && g.W && g.bias && g.C && g.tune >= 0, "gemm_tail: null operand or unset tune bits");
    MC_REQUIRE(tail_kernels_scratch_free() == 0,
               "gemm_tail: a tail kernel of this build uses scratch memory (%d bytes per lane; -1 = attributes unreadable): its hand-counted vmcnt "
               "waits are invalid -- rebuild with the toolchain the kernels were counted for", tail_kernels_scratch_free());
    MC_REQUIRE(g.K % BK == 0 && g.K >= BK && g.lda % 4 == 0 && g.ldw % 4 == 0 && g.half % 4 == 0 && g.w_gstride % 4 == 0,
               "gemm_tail: unsupported shape (M=%d N=%d K=%d)", g.M, g.N, g.K);
    if (g.M <= 0 || g.N <= 0) return MC_OK;
    MC_REQUIRE((long)g.N * g.ldw * 4 < (1L << 32), "gemm_tail: weight beyond 4 GB");
    const bool rows = g.rows_T > 0;      // per-row CFG weights: the same kernel forms over the same grids, ROWS instantiations
    MC_REQUIRE(!rows || (g.coef_table && g.rows_B > 0 && g.coef_stride >= 2 && !g.step_ptr), "gemm_tail: per-row weights need a table, B, a stride and no graph step");
    TailArgs gg = g;
    // tune bit 10 (round 5): the block-range form, A read once, one partial product per K group (gemm_tail2_k)
    int per_wave = 0;
    if (const int G = tail2_grid(gg, gg.tune, &per_wave)) {
        const int ncb = cdiv(g.N, 16);
        const long nblocks = (long)cdiv(g.M, 16) * ncb;
        dim3 grid(2 * G);                      // (range, K group)
        MC_LEDGER("gemm_tail2_k", grid, 2.0 * g.M * g.N * g.K * 2);      // both K groups
        if (rows) {
            if (per_wave <= 5) hipLaunchKernelGGL((gemm_tail2_k<4, true>), grid, dim3(256), 0, stream, gg, ncb, nblocks);
            else if (per_wave <= 9) hipLaunchKernelGGL((gemm_tail2_k<8, true>), grid, dim3(256), 0, stream, gg, ncb, nblocks);
            else if (per_wave <= 13) hipLaunchKernelGGL((gemm_tail2_k<12, true>), grid, dim3(256), 0, stream, gg, ncb, nblocks);
            else hipLaunchKernelGGL((gemm_tail2_k<16, true>), grid, dim3(256), 0, stream, gg, ncb, nblocks);
        }
        else if (per_wave <= 5) hipLaunchKernelGGL((gemm_tail2_k<4>), grid, dim3(256), 0, stream, gg, ncb, nblocks);
        else if (per_wave <= 9) hipLaunchKernelGGL((gemm_tail2_k<8>), grid, dim3(256), 0, stream, gg, ncb, nblocks);
        else if (per_wave <= 13) hipLaunchKernelGGL((gemm_tail2_k<12>), grid, dim3(256), 0, stream, gg, ncb, nblocks);
        else hipLaunchKernelGGL((gemm_tail2_k<16>), grid, dim3(256), 0, stream, gg, ncb, nblocks);
        MC_LAUNCH_CHECK();
        return MC_OK;
    }
    dim3 grid(cdiv(g.M, SM) * cdiv(g.N, 48));
    MC_LEDGER("gemm_tail_k", grid, 2.0 * g.M * g.N * g.K * 2);
    if (rows) hipLaunchKernelGGL((gemm_tail_k<3, true>), grid, dim3(256), 0, stream, gg);
    else hipLaunchKernelGGL((gemm_tail_k<3>), grid, dim3(256), 0, stream, gg);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
