// HBM-bound row kernels of the STMoGen denoiser (gfx950): LayerNorm rows, StylizationBlock
// prologue (LN + FiLM + SiLU), timestep embedding, CFG-combine + DDPM/DDIM update.
// All loads/stores are 16 B per lane, rows are reduced with wavefront shuffles (wave = 64).
#include <type_traits>
#include "mc_common.h"
#include "mc_kernels.h"
#include "mc_chain.h"

namespace {

// ---------------------------------------------------------------------------------------
// LayerNorm over short rows (L = 16..256, L/4 a power of two): LPR = L/4 lanes per row, one
// float4 per lane, 256/LPR rows per workgroup.  Two-pass variance like torch.layer_norm.
// reference: nn.LayerNorm(latent_dim) at st_attention.py:78-79,116-120, efficient_attention.py:15,32
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ln_rows_k(const float* __restrict__ X, long ldx, int x_col,
                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                 const float* __restrict__ add, int add_mod,
                                                 float* __restrict__ Y, long ldy, long rows, int L) {
    const int lpr = L >> 2;
    const int rpb = 256 / lpr;
    const int sub = threadIdx.x % lpr;
    const long r = (long)blockIdx.x * rpb + threadIdx.x / lpr;
    const bool ok = r < rows;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (ok) v = *reinterpret_cast<const f32x4*>(X + r * ldx + x_col + sub * 4);
    float s = group_sum(v[0] + v[1] + v[2] + v[3], lpr);
    const float mean = s / (float)L;
    f32x4 d = {v[0] - mean, v[1] - mean, v[2] - mean, v[3] - mean};
    float q = group_sum(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3], lpr);
    const float rstd = rsqrtf(q / (float)L + 1e-5f);
    if (!ok) return;
    const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + sub * 4);
    const f32x4 b = *reinterpret_cast<const f32x4*>(beta + sub * 4);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = d[j] * rstd * g[j] + b[j];
    if (add) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(add + (long)(r % add_mod) * L + sub * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] += a[j];
    }
    *reinterpret_cast<f32x4*>(Y + r * ldy + sub * 4) = o;
}

// ---------------------------------------------------------------------------------------
// StylizationBlock prologue: one wavefront per row of D (<= 2048) channels kept in registers.
//   a = silu( LN_D(y1 + y2) * (1 + scale) + shift )        stylization_block.py:36-39
// scale/shift = emb_layers(emb) are batch-invariant (same timestep for the whole batch) and
// precomputed per (step, layer, block): ss[0:D] = scale, ss[D:2D] = shift.
// ---------------------------------------------------------------------------------------
// RS (mc_sample_rows): FilmOneStep -- the whole launch sits at one schedule index (the default: nothing is read,
// the instruction stream of the kernel without the parameter); FilmRowSteps -- every row at the index of its request row,
// step[((row0 + r) / T) % B] (sample b + B is the CFG twin of b), with `ss` the table's row of index 0: one scalar table load per wave.
// `r` is the row this wave really works on (the fragment-major remap included); the twin alias only redirects the Y1 READ, the
// row's own schedule index stays its own (a twin shares its original's entry anyway).
constexpr int FILM_MAXC = 8;  // 8 float4 chunks x 64 lanes = 2048 channels
struct FilmOneStep {};
struct FilmRowSteps { const int* step; int B, T; long stride; };
template <class RS = FilmOneStep>
__global__ __launch_bounds__(256, 6) void film_rows_k(const float* __restrict__ Y1, const float* __restrict__ Y2,
                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                   const float* __restrict__ ss, float* __restrict__ A,
                                                   long rows, int D, TwinAlias y1_alias, long row0, StepRef step, int y1_parts,
                                                   long y1_pstride, int planes, long plane_stride, RS rs) {
    extern __shared__ __attribute__((aligned(16))) _Float16 film_stage[];      // fragment-major mode only: [plane][4 rows][D + 8] halves
    if (step.ptr) ss += (long)(*step.ptr) * step.stride;
    const int lane = threadIdx.x & 63;
    long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (planes & 4) {
        // fragment-major planes: a 32-row block is ONE 1 KB run per (k-step, plane), written 16 bytes per lane pair.  The eight workgroups that share a block are
        // given the same XCD (workgroup b lands on XCD b % 8 -- speed only) and consecutive dispatch slots there, so their pieces meet in ONE L2 and leave it as
        // whole lines: block = 8 (j / 8) + b % 8, rows 4 (j % 8) .. + 3 of it, j = b / 8 (the grid is padded to whole groups of 64: surplus workgroups leave)
        const long j = blockIdx.x >> 3;
        const long rb = (j >> 3) * 8 + (blockIdx.x & 7);
        r = rb * 32 + (j & 7) * 4 + (threadIdx.x >> 6);
    }
    if (r >= rows) return;
    if constexpr (std::is_same<RS, FilmRowSteps>::value) {
        // (a wave holds one row: the index is wave-uniform -- 32-bit division on the scalar side, `ss` stays a scalar pointer)
        const int rq = __builtin_amdgcn_readfirstlane((int)(((unsigned)(row0 + r) / (unsigned)rs.T) % (unsigned)rs.B));
        ss += (long)rs.step[rq] * rs.stride;
    }
    // CFG twin aliasing (base layer 0): Y1 rows that were not produced are read from their twin
    long r1 = r;
    if (y1_alias.split_flag && row0 + r >= y1_alias.from && *y1_alias.split_flag == 0) r1 = r - y1_alias.from;
    const int nch = D >> 2;
    f32x4 v[FILM_MAXC];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < FILM_MAXC; ++c) {
        const int ch = c * 64 + lane;
        v[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ch < nch) {
            v[c] = *reinterpret_cast<const f32x4*>(Y1 + r1 * D + ch * 4);
            // Y1 left as split-hidden partial sums by the producer (small batches): summed here, parts ascending like splitk_reduce_k
            for (int p = 1; p < y1_parts; ++p) v[c] += *reinterpret_cast<const f32x4*>(Y1 + (long)p * y1_pstride + r1 * D + ch * 4);
            if (Y2) {
                const f32x4 w = *reinterpret_cast<const f32x4*>(Y2 + r * D + ch * 4);
                v[c] += w;
            }
            s += v[c][0] + v[c][1] + v[c][2] + v[c][3];
        }
    }
    const float mean = group_sum(s, 64) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < FILM_MAXC; ++c) {
        const int ch = c * 64 + lane;
        if (ch < nch) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[c][j] -= mean;
                q += v[c][j] * v[c][j];
            }
        }
    }
    const float rstd = rsqrtf(group_sum(q, 64) / (float)D + 1e-5f);
#pragma unroll
    for (int c = 0; c < FILM_MAXC; ++c) {
        const int ch = c * 64 + lane;
        if (ch < nch) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + ch * 4);
            const f32x4 b = *reinterpret_cast<const f32x4*>(beta + ch * 4);
            const f32x4 sc = *reinterpret_cast<const f32x4*>(ss + ch * 4);
            const f32x4 sh = *reinterpret_cast<const f32x4*>(ss + D + ch * 4);
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = silu_f((v[c][j] * rstd * g[j] + b[j]) * (1.0f + sc[j]) + sh[j]);
            if ((planes & 3) == 0) *reinterpret_cast<f32x4*>(A + r * D + ch * 4) = o;
            else {
                // reduced-precision contexts: the GEMM that consumes `a` wants fp16 operand planes (hi, and lo = fp16(x - hi) in the
                // split mode: the arithmetic of split8, mc_half.hip) -- written here ONCE instead of converted by every column tile
                // of the GEMM.  A then is [rows][D] halves, the lo plane plane_stride halves behind it.
                typedef _Float16 h4 __attribute__((ext_vector_type(4)));
                h4 hi, lo;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float x = o[j];
                    asm volatile("" : "+v"(x));          // pinned: hi and lo must see the SAME fp32 value (no fused convert of the producer's product)
                    const _Float16 hx = (_Float16)x;
                    float hxf = (float)hx;
                    asm volatile("" : "+v"(hxf));
                    hi[j] = hx;
                    lo[j] = (_Float16)(x - hxf);
                }
                _Float16* Ah = reinterpret_cast<_Float16*>(A);
                if (planes & 4) {
                    // fragment-major planes: staged per workgroup (4 rows) and written out below in 64-byte runs
                    _Float16* st = film_stage + (threadIdx.x >> 6) * (D + 8) + ch * 4;
                    *reinterpret_cast<h4*>(st) = hi;
                    if ((planes & 3) == 2) *reinterpret_cast<h4*>(st + 4 * (D + 8)) = lo;
                } else {
                    *reinterpret_cast<h4*>(Ah + r * D + ch * 4) = hi;
                    if ((planes & 3) == 2) *reinterpret_cast<h4*>(Ah + plane_stride + r * D + ch * 4) = lo;
                }
            }
        }
    }
    if (planes & 4) {
        // FRAGMENT-MAJOR planes for gemm_hf_k: per 32-row block and 16-wide k-step the 64 lanes' MFMA operands contiguous -- [row block][k-step][lane = (row & 31) +
        // 32 ((k >> 3) & 1)][8 halves], rows local to this launch.  The workgroup's 4 consecutive rows are 4 consecutive lanes of a block: every (k-step, half)
        // slot gets one 64-byte run (4 threads x 16 bytes); the 8 workgroups of a block share an XCD (above) and complete the lines in its L2
        __syncthreads();
        const long rbase = r - (threadIdx.x >> 6);               // first row of this workgroup (a multiple of 4 inside one 32-row block)
        _Float16* Ah = reinterpret_cast<_Float16*>(A);
        const int npiece = 4 * (D >> 3);
        for (int pl = 0; pl < (planes & 3); ++pl)
            for (int p = threadIdx.x; p < npiece; p += 256) {
                const int row = p & 3, slot = p >> 2, ks = slot >> 1, hfk = slot & 1;
                const uint4 v = *reinterpret_cast<const uint4*>(film_stage + (pl * 4 + row) * (D + 8) + ks * 16 + hfk * 8);
                const long rr = rbase + row;
                *reinterpret_cast<uint4*>(Ah + pl * plane_stride + (((rr >> 5) * (long)(D >> 4) + ks) * 64 + (rr & 31) + 32 * hfk) * 8) = v;
            }
    }
}

// timestep_embedding (position_encoding.py:42-60): cat(cos(t f_j), sin(t f_j)), f_j = exp(-ln(1e4) j / half)
__global__ void timestep_embedding_k(const int* __restrict__ t_orig, float* __restrict__ te, int S, int D) {
    const int half = D / 2;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)S * D) return;
    const int s = (int)(i / D), j = (int)(i % D);
    float v = 0.f;
    if (j < 2 * half) {
        const int jj = j < half ? j : j - half;
        const float f = expf(-9.210340371976184f * (float)jj / (float)half);
        const float a = (float)t_orig[s] * f;
        v = j < half ? cosf(a) : sinf(a);
    }
    te[i] = v;
}

// out[r][c] = a[r][c] (or 0) + b[r][c] (or 0) + bias[c] (or 0), D % 4 == 0
__global__ __launch_bounds__(256) void add_rows_k(float* __restrict__ out, const float* __restrict__ a,
                                                  const float* __restrict__ b, const float* __restrict__ bias,
                                                  long rows, int D) {
    const long n4 = rows * (D / 4);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (a) v += *reinterpret_cast<const f32x4*>(a + i * 4);
        if (b) v += *reinterpret_cast<const f32x4*>(b + i * 4);
        if (bias) v += *reinterpret_cast<const f32x4*>(bias + (i % (D / 4)) * 4);
        *reinterpret_cast<f32x4*>(out + i * 4) = v;
    }
}

__global__ void silu_k(const float* __restrict__ X, float* __restrict__ Y, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) Y[i] = silu_f(X[i]);
}

__global__ void softmax_rows_small_k(const float* __restrict__ W, float* __restrict__ out, int rows, int cols) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    float m = -INFINITY;
    for (int c = 0; c < cols; ++c) m = fmaxf(m, W[r * cols + c]);
    float s = 0.f;
    for (int c = 0; c < cols; ++c) s += expf(W[r * cols + c] - m);
    for (int c = 0; c < cols; ++c) out[r * cols + c] = expf(W[r * cols + c] - m) / s;
}

// ---------------------------------------------------------------------------------------
// CFG combine (stmogen.py:753-760) fused with p_sample (gaussian_diffusion.py:634-696) or
// ddim_sample (:799-852).  5 (DDPM) streams of B*T*322 floats: HBM-bound, grid-stride.
// ---------------------------------------------------------------------------------------
// Device-side standard-normal draws for the fused sampler loop (mc_sample_loop): Philox4x32-10 (Salmon et al., SC'11), counter =
// (element / 4 [64 bit], draw index [64 bit]), key = the loop's 64-bit seed; the four 32-bit words of one call give the normals
// of elements 4g .. 4g+3 by two Box-Muller pairs, u = r 2^-32 + 2^-33 in (0, 1] (|z| <= 6.76).  Restated bit for bit (the
// integer part) in oracle/philox_oracle.py; the reference draws with th.randn_like (gaussian_diffusion.py:684, 847).
__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0], p1 = (unsigned long long)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[1] = (uint32_t)p1; c[3] = (uint32_t)p0; c[0] = n0; c[2] = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}
__device__ __forceinline__ void box_muller(uint32_t ra, uint32_t rb, float& z0, float& z1) {
    const float u1 = fmaf((float)ra, 2.3283064365386963e-10f, 1.1641532182693481e-10f);
    const float u2 = fmaf((float)rb, 2.3283064365386963e-10f, 1.1641532182693481e-10f);
    const float rad = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincospif(2.0f * u2, &sn, &cs);
    z0 = rad * cs;
    z1 = rad * sn;
}
__device__ __forceinline__ f32x4 philox_normal4(long group, RngArgs rng) {
    uint32_t c[4] = {(uint32_t)group, (uint32_t)((unsigned long long)group >> 32), rng.draw_lo, rng.draw_hi};
    philox4x32_10(c, rng.seed_lo, rng.seed_hi);
    f32x4 z;
    float a, b;
    box_muller(c[0], c[1], a, b); z[0] = a; z[1] = b;
    box_muller(c[2], c[3], a, b); z[2] = a; z[3] = b;
    return z;
}

// Row-keyed draws (mc_ctx_set_row_seeds): element r of row b of [B][TC] is element r of the Philox stream keyed by
// keys[b] -- counter (r / 4, draw), lane r % 4 -- so a row's noise depends neither on B nor on where the row sits.  -> the normals of the
// flat elements [i, i + 4), i % 4 == 0 (elements at or past n stay 0: no key is read for a row that does not exist).  One Philox call
// where the four share a row and a counter (always when TC % 4 == 0); where TC % 4 != 0 shifts the rows against the flat groups, or a
// group straddles two rows, one call per (row, counter) it touches: three at the most.
__device__ __forceinline__ f32x4 philox_rows4(long i, long n, RowKeys rk, RngArgs rng) {
    long b = i / rk.TC;
    int r = (int)(i - b * rk.TC);
    if ((r & 3) == 0 && r + 4 <= rk.TC && i + 4 <= n) {
        rng.seed_lo = rk.keys[2 * b]; rng.seed_hi = rk.keys[2 * b + 1];
        return philox_normal4(r >> 2, rng);
    }
    f32x4 z = {0.f, 0.f, 0.f, 0.f}, cur = z;
    long cb = -1;
    int cc = -1;
    for (int j = 0; j < 4 && i + j < n; ++j) {
        if (b != cb || (r >> 2) != cc) {
            cb = b; cc = r >> 2;
            rng.seed_lo = rk.keys[2 * b]; rng.seed_hi = rk.keys[2 * b + 1];
            cur = philox_normal4(cc, rng);
        }
        const int l = r & 3;
        z[j] = l == 0 ? cur[0] : l == 1 ? cur[1] : l == 2 ? cur[2] : cur[3];
        if (++r == rk.TC) { r = 0; ++b; }
    }
    return z;
}
// the in-kernel noise of flat group gi: from the call's one stream (RngArgs, the default), or from the rows' own streams
struct RowNoise { RngArgs rng; RowKeys rk; };
__device__ __forceinline__ f32x4 noise4(long gi, long, RngArgs rng) { return philox_normal4(gi, rng); }
__device__ __forceinline__ f32x4 noise4(long gi, long n, const RowNoise& r) { return philox_rows4(gi * 4, n, r.rk, r.rng); }

struct SamplerDerived { float sigma_ddpm, sq_abp, dir, sigma; };
__device__ __forceinline__ SamplerDerived sampler_derive(const SamplerCoefs& c) {
    SamplerDerived d;
    d.sigma_ddpm = c.nonzero * expf(0.5f * c.log_var);
    d.sq_abp = 0.f; d.dir = 0.f; d.sigma = 0.f;
    if (c.mode == 1) {
        d.sigma = __fmul_rn(__fmul_rn(c.eta, sqrtf(__fdiv_rn(1.f - c.ab_prev, 1.f - c.ab))), sqrtf(__fsub_rn(1.f, __fdiv_rn(c.ab, c.ab_prev))));
        d.sq_abp = sqrtf(c.ab_prev);
        d.dir = sqrtf(fmaf(-d.sigma, d.sigma, 1.f - c.ab_prev));
    }
    return d;
}
// one element of p_sample / ddim_sample -- the ONE place the update arithmetic lives (the host-noise and the device-noise
// kernels give the same bits for the same noise).  Which products are fused is spelled out with fmaf instead of being left to
// -ffp-contract: the free-running full-size golden (tests/golden/full_ddim.npz, 50 steps, 200 capacity-limited routings) is
// chaotic at near-tie gate decisions, so a 1-ulp change of x_{t-1} can move the final pose by O(0.5); these
// are the roundings that golden was recorded against in round 1 and they stay put whatever the compiler's contraction does.
// (Evaluating every reference op with its own rounding -- __fmul_rn / __fadd_rn in gaussian_diffusion.py's order -- was tried in
// round 3: per-step parity unchanged at 4e-6, but that trajectory meets a near-tie the reference resolves the other way.)
//   p_sample    :445-449, 693-694   mean = c1 x0 + c2 x;  sample = mean + (nonzero exp(0.5 log_var)) noise
//   ddim_sample :587-591, 847-852   eps = (sr x - x0) / srm1;  mean = x0 sqrt(abp) + sqrt(1 - abp - sigma^2) eps;  sample = mean + (nonzero sigma) noise
__device__ __forceinline__ float sampler_elem(float x, float x0, float nz, const SamplerCoefs& c, const SamplerDerived& d) {
    if (c.mode == 0) return fmaf(d.sigma_ddpm, nz, fmaf(c.c2, x, __fmul_rn(c.c1, x0)));
    const float eps = __fdiv_rn(fmaf(c.sqrt_recip, x, -x0), c.sqrt_recipm1);
    return fmaf(__fmul_rn(c.nonzero, d.sigma), nz, fmaf(d.sq_abp, x0, __fmul_rn(d.dir, eps)));
}
__device__ __forceinline__ float cfg_elem(float a, float b, const SamplerCoefs& c) { return fmaf(a, c.text_coef, __fmul_rn(b, c.none_coef)); }

// x_prev may alias x_t (in-place update: every element is read before it is written by the same thread; no __restrict__ on the two)
// VEC: every operand 16-byte aligned (float4 loads / stores); otherwise the same groups of 4 elements go element by element
// (C = 263 / 251 at odd B*T, or the second partial product of the folded tail at out2 + B*T*C: 8-byte aligned at best)
// NZ: the in-kernel draw (RNG) -- RngArgs, or RowNoise while the context holds a seed table; same groups, same straddle rule
template <bool RNG, bool VEC, class NZ = RngArgs>
__global__ __launch_bounds__(256) void sampler_update_k(const float* x_t, const float* __restrict__ o_text,
                                                        const float* __restrict__ o_none, const float* __restrict__ noise,
                                                        float* x_prev, float* __restrict__ x0_out, long n,
                                                        SamplerCoefs c, const SamplerCoefs* __restrict__ table,
                                                        const int* __restrict__ step_ptr, NZ rng, PadOut po) {
    if (table) {          // graph replay: this step's schedule coefficients from the device table
        const float tc = c.text_coef, nc = c.none_coef;
        c = table[*step_ptr];
        c.text_coef = tc;
        c.none_coef = nc;
    }
    const SamplerDerived d = sampler_derive(c);
    const long ngroups = (n + 3) >> 2;
    for (long gi = (long)blockIdx.x * blockDim.x + threadIdx.x; gi < ngroups; gi += (long)gridDim.x * blockDim.x) {
        const long i = gi * 4;
        if (VEC && i + 4 <= n) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(x_t + i);
            const f32x4 a = *reinterpret_cast<const f32x4*>(o_text + i), b = *reinterpret_cast<const f32x4*>(o_none + i);
            f32x4 nz;
            if constexpr (RNG) nz = noise4(gi, n, rng);
            else nz = *reinterpret_cast<const f32x4*>(noise + i);
            f32x4 out, x0v;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                x0v[j] = cfg_elem(a[j], b[j], c);
                out[j] = sampler_elem(x[j], x0v[j], nz[j], c, d);
            }
            *reinterpret_cast<f32x4*>(x_prev + i) = out;
            if (x0_out) *reinterpret_cast<f32x4*>(x0_out + i) = x0v;
            if (po.xpad) {        // the next step's pose-encoder operand: the same rows at the padded stride (pad columns stay zero)
                long row = i / po.C;
                int col = (int)(i - row * po.C);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    po.xpad[row * po.Cp + col] = out[j];
                    if (++col == po.C) { col = 0; ++row; }
                }
            }
        } else {
            f32x4 nz = {0.f, 0.f, 0.f, 0.f};
            if constexpr (RNG) nz = noise4(gi, n, rng);
            for (int j = 0; j < 4 && i + j < n; ++j) {
                const float x0 = cfg_elem(o_text[i + j], o_none[i + j], c);
                const float z = RNG ? nz[j] : noise[i + j];
                const float o = sampler_elem(x_t[i + j], x0, z, c, d);
                x_prev[i + j] = o;
                if (x0_out) x0_out[i + j] = x0;
                if (po.xpad) po.xpad[(i + j) / po.C * po.Cp + (i + j) % po.C] = o;
            }
        }
    }
}

// Multistep update (mode 2: DPM-Solver++ 2M on the data prediction; coefficients from GaussianDiffusion.multistep_coefs):
//   x0 = cfg_elem(o_text, o_none);   x_prev = k1 x0_prev + (kx x + k0 x0);   hist <- x0      with kx = c2, k0 = c1, k1 = eta
// A kernel of its own: sampler_elem / sampler_update_k keep the rounding sequence their goldens were recorded against.  Same operand
// forms as sampler_update_k (x_prev may alias x_t; VEC = every operand 16-byte aligned; table / step_ptr under graph replay; PadOut).
// `hist` is in-out: every thread reads its own elements before it writes them, and only when k1 != 0 (kernel-uniform) -- a first step
// meets an uninitialised buffer, and 0 x NaN would be NaN.  The products are spelled out so the bits do not depend on contraction.
__device__ __forceinline__ float multistep_elem(float x, float x0, float x0_prev, float kx, float k0, float k1) {
    return fmaf(k1, x0_prev, fmaf(kx, x, __fmul_rn(k0, x0)));
}
template <bool VEC>
__global__ __launch_bounds__(256) void sampler_multistep_k(const float* x_t, const float* __restrict__ o_text,
                                                           const float* __restrict__ o_none, float* __restrict__ hist,
                                                           float* x_prev, float* __restrict__ x0_out, long n, SamplerCoefs c,
                                                           const SamplerCoefs* __restrict__ table,
                                                           const int* __restrict__ step_ptr, PadOut po) {
    if (table) {          // graph replay: this step's schedule coefficients from the device table
        const float tc = c.text_coef, nc = c.none_coef;
        c = table[*step_ptr];
        c.text_coef = tc;
        c.none_coef = nc;
    }
    const float kx = c.c2, k0 = c.c1, k1 = c.eta;
    const bool use_hist = k1 != 0.f;
    const long ngroups = (n + 3) >> 2;
    for (long gi = (long)blockIdx.x * blockDim.x + threadIdx.x; gi < ngroups; gi += (long)gridDim.x * blockDim.x) {
        const long i = gi * 4;
        if (VEC && i + 4 <= n) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(x_t + i);
            const f32x4 a = *reinterpret_cast<const f32x4*>(o_text + i), b = *reinterpret_cast<const f32x4*>(o_none + i);
            f32x4 hp = {0.f, 0.f, 0.f, 0.f};
            if (use_hist) hp = *reinterpret_cast<const f32x4*>(hist + i);
            f32x4 out, x0v;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                x0v[j] = cfg_elem(a[j], b[j], c);
                out[j] = multistep_elem(x[j], x0v[j], hp[j], kx, k0, k1);
            }
            *reinterpret_cast<f32x4*>(x_prev + i) = out;
            *reinterpret_cast<f32x4*>(hist + i) = x0v;
            if (x0_out) *reinterpret_cast<f32x4*>(x0_out + i) = x0v;
            if (po.xpad) {        // the next step's pose-encoder operand: the same rows at the padded stride (pad columns stay zero)
                long row = i / po.C;
                int col = (int)(i - row * po.C);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    po.xpad[row * po.Cp + col] = out[j];
                    if (++col == po.C) { col = 0; ++row; }
                }
            }
        } else {
            for (int j = 0; j < 4 && i + j < n; ++j) {
                const float x0 = cfg_elem(o_text[i + j], o_none[i + j], c);
                const float hp = use_hist ? hist[i + j] : 0.f;
                const float o = multistep_elem(x_t[i + j], x0, hp, kx, k0, k1);
                x_prev[i + j] = o;
                hist[i + j] = x0;
                if (x0_out) x0_out[i + j] = x0;
                if (po.xpad) po.xpad[(i + j) / po.C * po.Cp + (i + j) % po.C] = o;
            }
        }
    }
}

// ---- per-row schedules (mc_sample_rows) ----
// Every request row b of [B][TC] walks its own schedule: element e takes coefs[e / TC], and under a seed table draw number draw[e / TC]
// (key keys[b], counter (row-local element / 4, draw[b])).  Kernels of their own beside sampler_update_k / sampler_multistep_k (whose
// instruction streams stay put) over the SAME device functions, flat groups of four, VEC rule and PadOut, so that equal entries in
// every row give the uniform kernels' bits.  A group that straddles two rows (TC % 4 != 0) goes on in the next row's coefficients from
// its first element there: every element takes its own row's, the rule philox_rows4 follows for keys.
// text_coef / none_coef of an entry are the CFG weights of the decoder tail in front (RowTab::coefs); here x0 arrives combined, as one
// array or two partial products, so the two weights are the launch's (tc, nc) like in the graph-table form.
__device__ __forceinline__ SamplerCoefs row_coefs(const SamplerCoefs* __restrict__ tab, long b, float tc, float nc) {
    SamplerCoefs c = tab[b];
    c.text_coef = tc; c.none_coef = nc;
    return c;
}
// philox_rows4 with the draw number per row, draw[b] ^ flip (flip: 0 for the step noise, MC_EDIT_DRAW_FLIP for the kept region's, section 4p)
__device__ __forceinline__ f32x4 philox_rows4x(long i, long n, RowKeys rk, const uint64_t* __restrict__ draw, uint64_t flip) {
    long b = i / rk.TC;
    int r = (int)(i - b * rk.TC);
    RngArgs rng;
    f32x4 z = {0.f, 0.f, 0.f, 0.f}, cur = z;
    long cb = -1;
    int cc = -1;
    for (int j = 0; j < 4 && i + j < n; ++j) {
        if (b != cb || (r >> 2) != cc) {
            cb = b; cc = r >> 2;
            const uint64_t dr = draw[b] ^ flip;
            rng.seed_lo = rk.keys[2 * b]; rng.seed_hi = rk.keys[2 * b + 1];
            rng.draw_lo = (uint32_t)dr; rng.draw_hi = (uint32_t)(dr >> 32);
            cur = philox_normal4(cc, rng);
        }
        const int l = r & 3;
        z[j] = l == 0 ? cur[0] : l == 1 ? cur[1] : l == 2 ? cur[2] : cur[3];
        if (++r == rk.TC) { r = 0; ++b; }
    }
    return z;
}
__device__ __forceinline__ f32x4 philox_rows4d(long i, long n, RowKeys rk, const uint64_t* __restrict__ draw) { return philox_rows4x(i, n, rk, draw, 0); }

template <bool RNG, bool VEC>
__global__ __launch_bounds__(256) void sampler_update_rows_k(const float* x_t, const float* __restrict__ o_text,
                                                             const float* __restrict__ o_none, const float* __restrict__ noise,
                                                             float* x_prev, float* __restrict__ x0_out, long n, float tc, float nc,
                                                             const SamplerCoefs* __restrict__ tab, RowKeys rk,
                                                             const uint64_t* __restrict__ draw, PadOut po) {
    const long ngroups = (n + 3) >> 2;
    for (long gi = (long)blockIdx.x * blockDim.x + threadIdx.x; gi < ngroups; gi += (long)gridDim.x * blockDim.x) {
        const long i = gi * 4;
        long b = i / rk.TC;
        int r = (int)(i - b * rk.TC);
        SamplerCoefs c = row_coefs(tab, b, tc, nc);
        SamplerDerived d = sampler_derive(c);
        f32x4 nz = {0.f, 0.f, 0.f, 0.f};
        if constexpr (RNG) nz = philox_rows4d(i, n, rk, draw);
        if (VEC && i + 4 <= n) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(x_t + i);
            const f32x4 a = *reinterpret_cast<const f32x4*>(o_text + i), bb = *reinterpret_cast<const f32x4*>(o_none + i);
            if constexpr (!RNG) nz = *reinterpret_cast<const f32x4*>(noise + i);
            f32x4 out, x0v;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                x0v[j] = cfg_elem(a[j], bb[j], c);
                out[j] = sampler_elem(x[j], x0v[j], nz[j], c, d);
                if (j < 3 && ++r == rk.TC) { r = 0; ++b; c = row_coefs(tab, b, tc, nc); d = sampler_derive(c); }
            }
            *reinterpret_cast<f32x4*>(x_prev + i) = out;
            if (x0_out) *reinterpret_cast<f32x4*>(x0_out + i) = x0v;
            if (po.xpad) {
                long row = i / po.C;
                int col = (int)(i - row * po.C);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    po.xpad[row * po.Cp + col] = out[j];
                    if (++col == po.C) { col = 0; ++row; }
                }
            }
        } else {
            for (int j = 0; j < 4 && i + j < n; ++j) {
                const float x0 = cfg_elem(o_text[i + j], o_none[i + j], c);
                const float z = RNG ? nz[j] : noise[i + j];
                const float o = sampler_elem(x_t[i + j], x0, z, c, d);
                x_prev[i + j] = o;
                if (x0_out) x0_out[i + j] = x0;
                if (po.xpad) po.xpad[(i + j) / po.C * po.Cp + (i + j) % po.C] = o;
                if (i + j + 1 < n && ++r == rk.TC) { r = 0; ++b; c = row_coefs(tab, b, tc, nc); d = sampler_derive(c); }
            }
        }
    }
}

// mode 2 per row: kx, k0, k1 of the element's row; the history is read only where the row's k1 != 0 (a row's first step meets whatever
// the buffer holds there, and 0 x NaN would be NaN)
template <bool VEC>
__global__ __launch_bounds__(256) void sampler_multistep_rows_k(const float* x_t, const float* __restrict__ o_text,
                                                                const float* __restrict__ o_none, float* __restrict__ hist,
                                                                float* x_prev, float* __restrict__ x0_out, long n, float tc, float nc,
                                                                const SamplerCoefs* __restrict__ tab, int TC, PadOut po) {
    const long ngroups = (n + 3) >> 2;
    for (long gi = (long)blockIdx.x * blockDim.x + threadIdx.x; gi < ngroups; gi += (long)gridDim.x * blockDim.x) {
        const long i = gi * 4;
        long b = i / TC;
        int r = (int)(i - b * TC);
        SamplerCoefs c = row_coefs(tab, b, tc, nc);
        if (VEC && i + 4 <= n) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(x_t + i);
            const f32x4 a = *reinterpret_cast<const f32x4*>(o_text + i), bb = *reinterpret_cast<const f32x4*>(o_none + i);
            const f32x4 hv = *reinterpret_cast<const f32x4*>(hist + i);
            f32x4 out, x0v;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                x0v[j] = cfg_elem(a[j], bb[j], c);
                out[j] = multistep_elem(x[j], x0v[j], c.eta != 0.f ? hv[j] : 0.f, c.c2, c.c1, c.eta);
                if (j < 3 && ++r == TC) { r = 0; ++b; c = row_coefs(tab, b, tc, nc); }
            }
            *reinterpret_cast<f32x4*>(x_prev + i) = out;
            *reinterpret_cast<f32x4*>(hist + i) = x0v;
            if (x0_out) *reinterpret_cast<f32x4*>(x0_out + i) = x0v;
            if (po.xpad) {
                long row = i / po.C;
                int col = (int)(i - row * po.C);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    po.xpad[row * po.Cp + col] = out[j];
                    if (++col == po.C) { col = 0; ++row; }
                }
            }
        } else {
            for (int j = 0; j < 4 && i + j < n; ++j) {
                const float x0 = cfg_elem(o_text[i + j], o_none[i + j], c);
                const float hp = c.eta != 0.f ? hist[i + j] : 0.f;
                const float o = multistep_elem(x_t[i + j], x0, hp, c.c2, c.c1, c.eta);
                x_prev[i + j] = o;
                hist[i + j] = x0;
                if (x0_out) x0_out[i + j] = x0;
                if (po.xpad) po.xpad[(i + j) / po.C * po.Cp + (i + j) % po.C] = o;
                if (i + j + 1 < n && ++r == TC) { r = 0; ++b; c = row_coefs(tab, b, tc, nc); }
            }
        }
    }
}

// ---- edited rows (mc_ctx_set_edit_rows) ----
// Element e of [B][TC] with keep[e] != 0 is GIVEN: x0 = keep ? gt : cfg_elem(..) -- a select, never a product, so whatever gt holds
// where keep == 0 (a NaN included) reaches no output -- and the row kernels' update goes on from that x0 (gaussian_diffusion.py:492-501).
// Mode 1 also replaces the new sample there, x_prev = sqrt(ab_prev) gt + sqrt(1 - ab_prev) z2 (:855-877 without the cross-fade), z2 a
// second normal: read from gt_noise, or (RNG) draw number draw[b] ^ 2^63 of the row's key at the row-local counter of the step draw,
// drawn only for groups that hold a kept element.  Kernels of their own beside the two row kernels over the same device functions, flat
// groups of four, VEC rule, straddle rule and PadOut: a row whose keep bytes are all zero gets the row kernels' bits.  The four keep
// bytes of a whole group inside n are one 32-bit load (kword: the table is 4-byte aligned); gt is read only for groups with a kept
// element.  x0_out, the history (mode 2) and xpad receive the edited values.
constexpr uint64_t MC_EDIT_DRAW_FLIP = 0x8000000000000000ull;
__device__ __forceinline__ uint32_t keep4(const uint8_t* __restrict__ keep, long i, long n, int kword) {
    if (kword && i + 4 <= n) return *reinterpret_cast<const uint32_t*>(keep + i);
    uint32_t w = 0;
    for (int j = 0; j < 4 && i + j < n; ++j) w |= (keep[i + j] ? 1u : 0u) << (8 * j);
    return w;
}
__device__ __forceinline__ bool kept(uint32_t kw, int j) { return ((kw >> (8 * j)) & 0xffu) != 0; }
// the kept region's new sample in mode 1
__device__ __forceinline__ float edit_renoise(float g, float z2, const SamplerCoefs& c, const SamplerDerived& d) {
    return fmaf(d.sq_abp, g, __fmul_rn(sqrtf(1.f - c.ab_prev), z2));
}

template <bool RNG, bool VEC>
__global__ __launch_bounds__(256) void sampler_edit_rows_k(const float* x_t, const float* __restrict__ o_text,
                                                           const float* __restrict__ o_none, const float* __restrict__ noise, EditTab et,
                                                           float* x_prev, float* __restrict__ x0_out, long n, float tc, float nc,
                                                           const SamplerCoefs* __restrict__ tab, RowKeys rk,
                                                           const uint64_t* __restrict__ draw, PadOut po) {
    const long ngroups = (n + 3) >> 2;
    for (long gi = (long)blockIdx.x * blockDim.x + threadIdx.x; gi < ngroups; gi += (long)gridDim.x * blockDim.x) {
        const long i = gi * 4;
        long b = i / rk.TC;
        int r = (int)(i - b * rk.TC);
        SamplerCoefs c = row_coefs(tab, b, tc, nc);
        SamplerDerived d = sampler_derive(c);
        const uint32_t kw = keep4(et.keep, i, n, et.kword);
        const bool renoise = kw != 0 && c.mode == 1;           // (one mode per launch)
        f32x4 nz = {0.f, 0.f, 0.f, 0.f}, z2 = nz, g = nz;
        if constexpr (RNG) {
            nz = philox_rows4d(i, n, rk, draw);
            if (renoise) z2 = philox_rows4x(i, n, rk, draw, MC_EDIT_DRAW_FLIP);
        }
        if (VEC && i + 4 <= n) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(x_t + i);
            const f32x4 a = *reinterpret_cast<const f32x4*>(o_text + i), bb = *reinterpret_cast<const f32x4*>(o_none + i);
            if constexpr (!RNG) {
                nz = *reinterpret_cast<const f32x4*>(noise + i);
                if (renoise) z2 = *reinterpret_cast<const f32x4*>(et.gt_noise + i);
            }
            if (kw) g = *reinterpret_cast<const f32x4*>(et.gt + i);
            f32x4 out, x0v;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool k = kept(kw, j);
                const float x0m = cfg_elem(a[j], bb[j], c);
                x0v[j] = k ? g[j] : x0m;
                const float o = sampler_elem(x[j], x0v[j], nz[j], c, d);
                out[j] = (k && c.mode == 1) ? edit_renoise(g[j], z2[j], c, d) : o;
                if (j < 3 && ++r == rk.TC) { r = 0; ++b; c = row_coefs(tab, b, tc, nc); d = sampler_derive(c); }
            }
            *reinterpret_cast<f32x4*>(x_prev + i) = out;
            if (x0_out) *reinterpret_cast<f32x4*>(x0_out + i) = x0v;
            if (po.xpad) {
                long row = i / po.C;
                int col = (int)(i - row * po.C);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    po.xpad[row * po.Cp + col] = out[j];
                    if (++col == po.C) { col = 0; ++row; }
                }
            }
        } else {
            for (int j = 0; j < 4 && i + j < n; ++j) {
                const bool k = kept(kw, j);
                const float gj = k ? et.gt[i + j] : 0.f;
                const float x0m = cfg_elem(o_text[i + j], o_none[i + j], c);
                const float x0 = k ? gj : x0m;
                const float z = RNG ? nz[j] : noise[i + j];
                float o = sampler_elem(x_t[i + j], x0, z, c, d);
                if (k && c.mode == 1) o = edit_renoise(gj, RNG ? z2[j] : et.gt_noise[i + j], c, d);
                x_prev[i + j] = o;
                if (x0_out) x0_out[i + j] = x0;
                if (po.xpad) po.xpad[(i + j) / po.C * po.Cp + (i + j) % po.C] = o;
                if (i + j + 1 < n && ++r == rk.TC) { r = 0; ++b; c = row_coefs(tab, b, tc, nc); d = sampler_derive(c); }
            }
        }
    }
}

// mode 2 with the kept region: x0 = keep ? gt : cfg_elem(..);  x_prev = multistep_elem(x, x0, hist, ..);  hist <- x0 (the edited one)
template <bool VEC>
__global__ __launch_bounds__(256) void sampler_multistep_edit_rows_k(const float* x_t, const float* __restrict__ o_text,
                                                                     const float* __restrict__ o_none, float* __restrict__ hist, EditTab et,
                                                                     float* x_prev, float* __restrict__ x0_out, long n, float tc, float nc,
                                                                     const SamplerCoefs* __restrict__ tab, int TC, PadOut po) {
    const long ngroups = (n + 3) >> 2;
    for (long gi = (long)blockIdx.x * blockDim.x + threadIdx.x; gi < ngroups; gi += (long)gridDim.x * blockDim.x) {
        const long i = gi * 4;
        long b = i / TC;
        int r = (int)(i - b * TC);
        SamplerCoefs c = row_coefs(tab, b, tc, nc);
        const uint32_t kw = keep4(et.keep, i, n, et.kword);
        if (VEC && i + 4 <= n) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(x_t + i);
            const f32x4 a = *reinterpret_cast<const f32x4*>(o_text + i), bb = *reinterpret_cast<const f32x4*>(o_none + i);
            const f32x4 hv = *reinterpret_cast<const f32x4*>(hist + i);
            f32x4 g = {0.f, 0.f, 0.f, 0.f};
            if (kw) g = *reinterpret_cast<const f32x4*>(et.gt + i);
            f32x4 out, x0v;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float x0m = cfg_elem(a[j], bb[j], c);
                x0v[j] = kept(kw, j) ? g[j] : x0m;
                out[j] = multistep_elem(x[j], x0v[j], c.eta != 0.f ? hv[j] : 0.f, c.c2, c.c1, c.eta);
                if (j < 3 && ++r == TC) { r = 0; ++b; c = row_coefs(tab, b, tc, nc); }
            }
            *reinterpret_cast<f32x4*>(x_prev + i) = out;
            *reinterpret_cast<f32x4*>(hist + i) = x0v;
            if (x0_out) *reinterpret_cast<f32x4*>(x0_out + i) = x0v;
            if (po.xpad) {
                long row = i / po.C;
                int col = (int)(i - row * po.C);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    po.xpad[row * po.Cp + col] = out[j];
                    if (++col == po.C) { col = 0; ++row; }
                }
            }
        } else {
            for (int j = 0; j < 4 && i + j < n; ++j) {
                const float x0m = cfg_elem(o_text[i + j], o_none[i + j], c);
                const float x0 = kept(kw, j) ? et.gt[i + j] : x0m;
                const float hp = c.eta != 0.f ? hist[i + j] : 0.f;
                const float o = multistep_elem(x_t[i + j], x0, hp, c.c2, c.c1, c.eta);
                x_prev[i + j] = o;
                hist[i + j] = x0;
                if (x0_out) x0_out[i + j] = x0;
                if (po.xpad) po.xpad[(i + j) / po.C * po.Cp + (i + j) % po.C] = o;
                if (i + j + 1 < n && ++r == TC) { r = 0; ++b; c = row_coefs(tab, b, tc, nc); }
            }
        }
    }
}

// Seam-coupled update (window-parallel long sequences): the batch rows are windows of T frames; rows b and b + 1
// flagged as neighbours share `ov` frames -- frames [T - ov, T) of b (its tail) are frames [0, ov) of b + 1 (its head).  A seam element
//   x0 = w[f] x0_right + (1 - w[f]) x0_left;   x_prev = update(x_left, x0, noise_left / hist_left)
// is computed ONCE, by the thread that owns the LEFT (tail) element, and stored to both rows (x_prev, x0_out, hist, xpad); head elements
// of a row with a left neighbour are skipped by their own thread.  All three modes (c.mode is kernel-uniform), host noise or Philox.
// Same flat groups of four as sampler_update_k, so every non-seam element sees the same Philox counter and the same device functions:
// the same bits.  Groups that touch no overlap region keep the f32x4 path; the others go element by element (C is no multiple of 4: a
// group can hold seam and plain elements at once).  x_prev may alias x_t: a thread reads its own x_t elements before it writes, and the
// only foreign elements it writes are head elements, which no thread reads (2 ov <= T: a head element is never a tail element).
// No graph table: a context with a seam table refuses capture.
enum { SEAM_LEFT = 1, SEAM_RIGHT = 2 };      // SeamTab::flags[b]: the row has a left / a right neighbour
template <bool RNG, bool VEC, class NZ = RngArgs>
__global__ __launch_bounds__(256) void sampler_seam_k(const float* x_t, const float* __restrict__ o_text,
                                                      const float* __restrict__ o_none, const float* __restrict__ noise,
                                                      float* hist, float* x_prev, float* x0_out, long n, SamplerCoefs c,
                                                      SeamTab st, NZ rng, PadOut po) {
    const SamplerDerived d = sampler_derive(c);
    const bool ms = c.mode == 2;
    const float kx = c.c2, k0 = c.c1, k1 = c.eta;
    const bool use_hist = ms && k1 != 0.f;
    const int TC = st.T * st.C, headC = st.ov * st.C, tailC = (st.T - st.ov) * st.C;
    const long ngroups = (n + 3) >> 2;
    for (long gi = (long)blockIdx.x * blockDim.x + threadIdx.x; gi < ngroups; gi += (long)gridDim.x * blockDim.x) {
        const long i = gi * 4;
        // classify the four elements: 0 plain, 1 head (skipped), 2 tail (seam owner)
        int b = (int)(i / TC);
        int rem = (int)(i - (long)b * TC);
        int cls[4], rr[4];
        int any = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            cls[j] = 0; rr[j] = rem;
            if (i + j < n) {
                const int fl = st.flags[b];
                if (rem < headC && (fl & SEAM_LEFT)) cls[j] = 1;
                else if (rem >= tailC && (fl & SEAM_RIGHT)) cls[j] = 2;
            }
            any |= cls[j];
            if (++rem == TC) { rem = 0; ++b; }
        }
        if (VEC && i + 4 <= n && !any) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(x_t + i);
            const f32x4 a = *reinterpret_cast<const f32x4*>(o_text + i), bb = *reinterpret_cast<const f32x4*>(o_none + i);
            f32x4 nz = {0.f, 0.f, 0.f, 0.f}, hp = {0.f, 0.f, 0.f, 0.f};
            if (!ms) {
                if constexpr (RNG) nz = noise4(gi, n, rng);
                else nz = *reinterpret_cast<const f32x4*>(noise + i);
            } else if (use_hist) hp = *reinterpret_cast<const f32x4*>(hist + i);
            f32x4 out, x0v;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                x0v[j] = cfg_elem(a[j], bb[j], c);
                out[j] = ms ? multistep_elem(x[j], x0v[j], hp[j], kx, k0, k1) : sampler_elem(x[j], x0v[j], nz[j], c, d);
            }
            *reinterpret_cast<f32x4*>(x_prev + i) = out;
            if (ms) *reinterpret_cast<f32x4*>(hist + i) = x0v;
            if (x0_out) *reinterpret_cast<f32x4*>(x0_out + i) = x0v;
            if (po.xpad) {
                long row = i / po.C;
                int col = (int)(i - row * po.C);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    po.xpad[row * po.Cp + col] = out[j];
                    if (++col == po.C) { col = 0; ++row; }
                }
            }
        } else {
            f32x4 nz = {0.f, 0.f, 0.f, 0.f};
            if constexpr (RNG) { if (!ms) nz = noise4(gi, n, rng); }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (i + j >= n || cls[j] == 1) continue;         // (head: written by the left neighbour's tail thread)
                const long e = i + j;
                float x0 = cfg_elem(o_text[e], o_none[e], c);
                long er = -1;
                if (cls[j] == 2) {                               // (b + 1, f, ch): the flags say that row exists
                    er = e + headC;                              // = e + TC - tailC
                    const float w = st.w[(rr[j] - tailC) / st.C];
                    const float x0r = cfg_elem(o_text[er], o_none[er], c);
                    x0 = fmaf(w, x0r, __fmul_rn(__fsub_rn(1.f, w), x0));
                }
                float o;
                if (ms) o = multistep_elem(x_t[e], x0, use_hist ? hist[e] : 0.f, kx, k0, k1);
                else o = sampler_elem(x_t[e], x0, RNG ? nz[j] : noise[e], c, d);
                x_prev[e] = o;
                if (ms) hist[e] = x0;
                if (x0_out) x0_out[e] = x0;
                if (po.xpad) po.xpad[e / po.C * po.Cp + e % po.C] = o;
                if (er >= 0) {
                    x_prev[er] = o;
                    if (ms) hist[er] = x0;
                    if (x0_out) x0_out[er] = x0;
                    if (po.xpad) po.xpad[er / po.C * po.Cp + er % po.C] = o;
                }
            }
        }
    }
}

// ---- seam-coupled windows in the per-row path (mc_ctx_set_seam_rows) ----
// sampler_seam_k's blend and ownership over sampler_update_rows_k's per-row entries: a long request takes ANY rows of the batch as its
// windows.  Row b's entry of the table (SeamRow, 16-byte aligned: ONE load per group, no dependent second one; gfx950: global_load_dwordx3, the words in use) names its right neighbour right[b] (any
// row, lower or higher, or -1), whether it has a left one, and the global frame its frame 0 shows.  A tail element of a row with a right
// neighbour is the seam's owner: x0 = fmaf(w, x0_right, (1 - w) x0_left) over the two cfg_elem results, the update under the OWNER's
// row entry (the host checked both rows of a seam carry equal entries), stored to both rows (x_prev, x0_out, hist, xpad); the right
// element is e + (right[b] - b) TC - tailC.  Head elements of a row with a left neighbour are skipped by their own thread.
// In place (x_prev == x_t): a thread reads its own x_t / hist elements before it writes them, and the only foreign elements it writes
// are head elements, which NO thread reads (their own thread skips them; 2 ov <= T: a head element is never a tail element) -- that does
// not depend on the sign of right[b] - b, so a right neighbour at a lower row index changes nothing.
// Noise (RNG): the request-global counter rule -- element r of row b is element g = first_frame[b] C + r (64-bit) of the request's
// stream: key keys[b] (every row of a request carries the request's seed), counter (g / 4, draw[b]), lane g % 4.  The two copies of a
// shared frame have the same g, so they would draw the same normal; a row with first_frame 0 draws what philox_rows4x gives it.
// Flat groups of four, VEC rule, straddle rule and PadOut as in sampler_update_rows_k; the index arithmetic is 32-bit (the launcher
// requires n < 2^31: one unsigned division per group).  Groups that touch no overlap region keep f32x4 loads and stores, the others go
// element by element.  The mode is launch-uniform (ms: mode 2; modes 0 / 1 through sampler_elem on the row's entry); the history is
// read only where the row's k1 != 0.  No LDS, no atomics.
__device__ __forceinline__ f32x4 philox_rows4g(uint32_t i, uint32_t n, RowKeys rk, const uint64_t* __restrict__ draw,
                                               const SeamRow* __restrict__ rows, int C, int first0) {
    uint32_t b = i / (uint32_t)rk.TC;
    int r = (int)(i - b * (uint32_t)rk.TC);
    RngArgs rng;
    f32x4 z = {0.f, 0.f, 0.f, 0.f}, cur = z;
    long cb = -1, cc = -1;
    long g = (long)first0 * C + r;               // (first0: first_frame of the group's first row, from the entry the caller holds)
    for (int j = 0; j < 4 && i + j < n; ++j) {
        if ((long)b != cb || (g >> 2) != cc) {
            cb = b; cc = g >> 2;
            const uint64_t dr = draw[b];
            rng.seed_lo = rk.keys[2 * b]; rng.seed_hi = rk.keys[2 * b + 1];
            rng.draw_lo = (uint32_t)dr; rng.draw_hi = (uint32_t)(dr >> 32);
            cur = philox_normal4(cc, rng);
        }
        const int l = (int)(g & 3);
        z[j] = l == 0 ? cur[0] : l == 1 ? cur[1] : l == 2 ? cur[2] : cur[3];
        ++g;
        if (++r == rk.TC) { r = 0; ++b; if (i + j + 1 < n) g = (long)rows[b].first_frame * C; }
    }
    return z;
}

template <bool RNG, bool VEC>
__global__ __launch_bounds__(256) void sampler_seam_rows_k(const float* x_t, const float* __restrict__ o_text,
                                                           const float* __restrict__ o_none, const float* __restrict__ noise,
                                                           float* hist, float* x_prev, float* x0_out, uint32_t n, float tc, float nc,
                                                           const SamplerCoefs* __restrict__ tab, RowKeys rk,
                                                           const uint64_t* __restrict__ draw, SeamRowsTab st, int ms, PadOut po) {
    const int TC = rk.TC, headC = st.ov * st.C, tailC = (st.T - st.ov) * st.C;
    const uint32_t ngroups = (n + 3) >> 2;
    for (uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x; gi < ngroups; gi += gridDim.x * blockDim.x) {
        const uint32_t i = gi * 4;
        uint32_t b = i / (uint32_t)TC;
        int r = (int)(i - b * (uint32_t)TC);
        const bool whole = i + 4 <= n;
        SeamRow sr = st.rows[b];
        // does the group touch an overlap region?  Its elements of row b are [r, min(r + 3, TC - 1)]; a straddling whole group goes on
        // with elements [0, r + 3 - TC] of row b + 1 (TC >= 4: two rows at the most)
        bool any = (sr.has_left && r < headC) || (sr.right >= 0 && (r + 3 >= tailC));
        if (whole && r + 4 > TC) {
            const SeamRow s1 = st.rows[b + 1];
            any = any || s1.has_left || (s1.right >= 0 && r + 3 - TC >= tailC);
        }
        SamplerCoefs c = row_coefs(tab, b, tc, nc);
        SamplerDerived d = sampler_derive(c);
        f32x4 nz = {0.f, 0.f, 0.f, 0.f};
        if constexpr (RNG) { if (!ms) nz = philox_rows4g(i, n, rk, draw, st.rows, st.C, sr.first_frame); }
        if (VEC && whole && !any) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(x_t + i);
            const f32x4 a = *reinterpret_cast<const f32x4*>(o_text + i), bb = *reinterpret_cast<const f32x4*>(o_none + i);
            f32x4 hv = {0.f, 0.f, 0.f, 0.f};
            if (ms) hv = *reinterpret_cast<const f32x4*>(hist + i);
            else if constexpr (!RNG) nz = *reinterpret_cast<const f32x4*>(noise + i);
            f32x4 out, x0v;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                x0v[j] = cfg_elem(a[j], bb[j], c);
                out[j] = ms ? multistep_elem(x[j], x0v[j], c.eta != 0.f ? hv[j] : 0.f, c.c2, c.c1, c.eta) : sampler_elem(x[j], x0v[j], nz[j], c, d);
                if (j < 3 && ++r == TC) { r = 0; ++b; c = row_coefs(tab, b, tc, nc); d = sampler_derive(c); }
            }
            *reinterpret_cast<f32x4*>(x_prev + i) = out;
            if (ms) *reinterpret_cast<f32x4*>(hist + i) = x0v;
            if (x0_out) *reinterpret_cast<f32x4*>(x0_out + i) = x0v;
            if (po.xpad) {
                uint32_t row = i / (uint32_t)po.C;
                int col = (int)(i - row * (uint32_t)po.C);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    po.xpad[(long)row * po.Cp + col] = out[j];
                    if (++col == po.C) { col = 0; ++row; }
                }
            }
        } else {
            for (int j = 0; j < 4 && i + j < n; ++j) {
                const uint32_t e = i + j;
                if (!(sr.has_left && r < headC)) {               // (head: written by the left neighbour's tail thread)
                    float x0 = cfg_elem(o_text[e], o_none[e], c);
                    long er = -1;
                    if (sr.right >= 0 && r >= tailC) {           // the seam's owner: (right[b], f, ch)
                        er = (long)e + ((long)sr.right - (long)b) * TC - tailC;
                        const float w = st.w[(r - tailC) / st.C];
                        const float x0r = cfg_elem(o_text[er], o_none[er], c);
                        x0 = fmaf(w, x0r, __fmul_rn(__fsub_rn(1.f, w), x0));
                    }
                    float o;
                    if (ms) o = multistep_elem(x_t[e], x0, c.eta != 0.f ? hist[e] : 0.f, c.c2, c.c1, c.eta);
                    else o = sampler_elem(x_t[e], x0, RNG ? nz[j] : noise[e], c, d);
                    x_prev[e] = o;
                    if (ms) hist[e] = x0;
                    if (x0_out) x0_out[e] = x0;
                    if (po.xpad) po.xpad[(long)(e / (uint32_t)po.C) * po.Cp + e % (uint32_t)po.C] = o;
                    if (er >= 0) {
                        x_prev[er] = o;
                        if (ms) hist[er] = x0;
                        if (x0_out) x0_out[er] = x0;
                        if (po.xpad) po.xpad[er / po.C * po.Cp + er % po.C] = o;
                    }
                }
                if (e + 1 < n && ++r == TC) { r = 0; ++b; sr = st.rows[b]; c = row_coefs(tab, b, tc, nc); d = sampler_derive(c); }
            }
        }
    }
}

// ---- kept regions on seam-coupled rows (mc_ctx_set_long_edits) ----
// sampler_seam_rows_k's blend and ownership with sampler_edit_rows_k's select behind it, nothing new beyond their order:
//   x0m = cfg_elem(..);  the seam's owner: x0m = fmaf(w, x0_right, (1 - w) x0m);  x0 = keep ? gt : x0m  (a select AFTER the blend)
//   modes 0 / 1: sampler_elem on x0, in mode 1 x_prev = edit_renoise(gt, z2) where kept;  mode 2: multistep_elem, hist <- x0
// The owner reads ITS OWN keep / gt (and noise / gt_noise element) and stores x_prev, x0_out, the history and xpad to both copies of a
// shared element; the head copy's keep / gt entries are never used for an output (its thread skips the element).  gt where keep == 0
// reaches no output.  Noise (RNG): the request-global field of philox_rows4g for both draws, z2 at draw[b] ^ MC_EDIT_DRAW_FLIP, drawn in
// mode 1 only and only for groups whose keep word is non-zero -- both copies of a shared frame would draw the same z2, and a row with
// first_frame 0 draws what sampler_edit_rows_k draws.  One kernel for the three modes (launch-uniform `mode`).  Flat groups of four,
// 32-bit index arithmetic, VEC rule, straddle rule and PadOut as in sampler_seam_rows_k: groups that touch no overlap region keep f32x4
// loads and stores (keep bytes: one 32-bit load; gt / z2 only behind a non-zero word), the others go element by element.  All-zero
// keep bytes give sampler_seam_rows_k's bits; a table without neighbours at first_frame 0 gives the two edit kernels'.  No LDS, no
// atomics.  philox_rows4g with the draw number flipped is a sibling of its own: philox_rows4g keeps its instruction stream.
__device__ __forceinline__ f32x4 philox_rows4gx(uint32_t i, uint32_t n, RowKeys rk, const uint64_t* __restrict__ draw,
                                                const SeamRow* __restrict__ rows, int C, int first0, uint64_t flip) {
    uint32_t b = i / (uint32_t)rk.TC;
    int r = (int)(i - b * (uint32_t)rk.TC);
    RngArgs rng;
    f32x4 z = {0.f, 0.f, 0.f, 0.f}, cur = z;
    long cb = -1, cc = -1;
    long g = (long)first0 * C + r;
    for (int j = 0; j < 4 && i + j < n; ++j) {
        if ((long)b != cb || (g >> 2) != cc) {
            cb = b; cc = g >> 2;
            const uint64_t dr = draw[b] ^ flip;
            rng.seed_lo = rk.keys[2 * b]; rng.seed_hi = rk.keys[2 * b + 1];
            rng.draw_lo = (uint32_t)dr; rng.draw_hi = (uint32_t)(dr >> 32);
            cur = philox_normal4(cc, rng);
        }
        const int l = (int)(g & 3);
        z[j] = l == 0 ? cur[0] : l == 1 ? cur[1] : l == 2 ? cur[2] : cur[3];
        ++g;
        if (++r == rk.TC) { r = 0; ++b; if (i + j + 1 < n) g = (long)rows[b].first_frame * C; }
    }
    return z;
}

template <bool RNG, bool VEC>
__global__ __launch_bounds__(256) void sampler_seam_edit_rows_k(const float* x_t, const float* __restrict__ o_text,
                                                                const float* __restrict__ o_none, const float* __restrict__ noise,
                                                                float* hist, EditTab et, float* x_prev, float* x0_out, uint32_t n, float tc,
                                                                float nc, const SamplerCoefs* __restrict__ tab, RowKeys rk,
                                                                const uint64_t* __restrict__ draw, SeamRowsTab st, int mode, PadOut po) {
    const bool ms = mode == 2, m1 = mode == 1;
    const int TC = rk.TC, headC = st.ov * st.C, tailC = (st.T - st.ov) * st.C;
    const uint32_t ngroups = (n + 3) >> 2;
    for (uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x; gi < ngroups; gi += gridDim.x * blockDim.x) {
        const uint32_t i = gi * 4;
        uint32_t b = i / (uint32_t)TC;
        int r = (int)(i - b * (uint32_t)TC);
        const bool whole = i + 4 <= n;
        SeamRow sr = st.rows[b];
        bool any = (sr.has_left && r < headC) || (sr.right >= 0 && (r + 3 >= tailC));      // (as in sampler_seam_rows_k)
        if (whole && r + 4 > TC) {
            const SeamRow s1 = st.rows[b + 1];
            any = any || s1.has_left || (s1.right >= 0 && r + 3 - TC >= tailC);
        }
        SamplerCoefs c = row_coefs(tab, b, tc, nc);
        SamplerDerived d = sampler_derive(c);
        const uint32_t kw = keep4(et.keep, i, n, et.kword);
        const bool renoise = kw != 0 && m1;
        f32x4 nz = {0.f, 0.f, 0.f, 0.f}, z2 = nz;
        if constexpr (RNG) {
            if (!ms) nz = philox_rows4gx(i, n, rk, draw, st.rows, st.C, sr.first_frame, 0);
            if (renoise) z2 = philox_rows4gx(i, n, rk, draw, st.rows, st.C, sr.first_frame, MC_EDIT_DRAW_FLIP);
        }
        if (VEC && whole && !any) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(x_t + i);
            const f32x4 a = *reinterpret_cast<const f32x4*>(o_text + i), bb = *reinterpret_cast<const f32x4*>(o_none + i);
            f32x4 hv = {0.f, 0.f, 0.f, 0.f}, g = hv;
            if (ms) hv = *reinterpret_cast<const f32x4*>(hist + i);
            else if constexpr (!RNG) {
                nz = *reinterpret_cast<const f32x4*>(noise + i);
                if (renoise) z2 = *reinterpret_cast<const f32x4*>(et.gt_noise + i);
            }
            if (kw) g = *reinterpret_cast<const f32x4*>(et.gt + i);
            f32x4 out, x0v;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool k = kept(kw, j);
                const float x0m = cfg_elem(a[j], bb[j], c);
                x0v[j] = k ? g[j] : x0m;
                const float o = ms ? multistep_elem(x[j], x0v[j], c.eta != 0.f ? hv[j] : 0.f, c.c2, c.c1, c.eta) : sampler_elem(x[j], x0v[j], nz[j], c, d);
                out[j] = (k && m1) ? edit_renoise(g[j], z2[j], c, d) : o;
                if (j < 3 && ++r == TC) { r = 0; ++b; c = row_coefs(tab, b, tc, nc); d = sampler_derive(c); }
            }
            *reinterpret_cast<f32x4*>(x_prev + i) = out;
            if (ms) *reinterpret_cast<f32x4*>(hist + i) = x0v;
            if (x0_out) *reinterpret_cast<f32x4*>(x0_out + i) = x0v;
            if (po.xpad) {
                uint32_t row = i / (uint32_t)po.C;
                int col = (int)(i - row * (uint32_t)po.C);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    po.xpad[(long)row * po.Cp + col] = out[j];
                    if (++col == po.C) { col = 0; ++row; }
                }
            }
        } else {
            for (int j = 0; j < 4 && i + j < n; ++j) {
                const uint32_t e = i + j;
                if (!(sr.has_left && r < headC)) {               // (head: written by the left neighbour's tail thread, its keep / gt unused)
                    const bool k = kept(kw, j);
                    const float gj = k ? et.gt[e] : 0.f;
                    float x0 = cfg_elem(o_text[e], o_none[e], c);
                    long er = -1;
                    if (sr.right >= 0 && r >= tailC) {           // the seam's owner: (right[b], f, ch)
                        er = (long)e + ((long)sr.right - (long)b) * TC - tailC;
                        const float w = st.w[(r - tailC) / st.C];
                        const float x0r = cfg_elem(o_text[er], o_none[er], c);
                        x0 = fmaf(w, x0r, __fmul_rn(__fsub_rn(1.f, w), x0));
                    }
                    x0 = k ? gj : x0;                            // the select, after the blend
                    float o;
                    if (ms) o = multistep_elem(x_t[e], x0, c.eta != 0.f ? hist[e] : 0.f, c.c2, c.c1, c.eta);
                    else o = sampler_elem(x_t[e], x0, RNG ? nz[j] : noise[e], c, d);
                    if (k && m1) o = edit_renoise(gj, RNG ? z2[j] : et.gt_noise[e], c, d);
                    x_prev[e] = o;
                    if (ms) hist[e] = x0;
                    if (x0_out) x0_out[e] = x0;
                    if (po.xpad) po.xpad[(long)(e / (uint32_t)po.C) * po.Cp + e % (uint32_t)po.C] = o;
                    if (er >= 0) {
                        x_prev[er] = o;
                        if (ms) hist[er] = x0;
                        if (x0_out) x0_out[er] = x0;
                        if (po.xpad) po.xpad[er / po.C * po.Cp + er % po.C] = o;
                    }
                }
                if (e + 1 < n && ++r == TC) { r = 0; ++b; sr = st.rows[b]; c = row_coefs(tab, b, tc, nc); d = sampler_derive(c); }
            }
        }
    }
}

// the same draws written to memory (tests; callers that want the loop's noise stream)
__global__ __launch_bounds__(256) void philox_fill_k(float* __restrict__ out, uint32_t* __restrict__ bits, long n, RngArgs rng) {
    const long ngroups = (n + 3) >> 2;
    for (long gi = (long)blockIdx.x * blockDim.x + threadIdx.x; gi < ngroups; gi += (long)gridDim.x * blockDim.x) {
        if (bits) {
            uint32_t c[4] = {(uint32_t)gi, (uint32_t)((unsigned long long)gi >> 32), rng.draw_lo, rng.draw_hi};
            philox4x32_10(c, rng.seed_lo, rng.seed_hi);
            for (int j = 0; j < 4 && gi * 4 + j < n; ++j) bits[gi * 4 + j] = c[j];
        }
        if (out) {
            const f32x4 z = philox_normal4(gi, rng);
            for (int j = 0; j < 4 && gi * 4 + j < n; ++j) out[gi * 4 + j] = z[j];
        }
    }
}

// mc_ctx_draw_rows: out [B][TC] = draw `rng.draw_*` of every row's own stream (philox_rows4).  Flat groups of four: one f32x4 store where
// the group lies inside one row (out + 4 gi is 16-byte aligned when out is), element-wise where TC % 4 != 0 makes it straddle two rows
// or at the ragged end.
__global__ __launch_bounds__(256) void philox_rows_fill_k(float* __restrict__ out, long n, RowKeys rk, RngArgs rng, int vec) {
    const long ngroups = (n + 3) >> 2;
    for (long gi = (long)blockIdx.x * blockDim.x + threadIdx.x; gi < ngroups; gi += (long)gridDim.x * blockDim.x) {
        const long i = gi * 4;
        const f32x4 z = philox_rows4(i, n, rk, rng);
        if (vec && i + 4 <= n && i / rk.TC == (i + 3) / rk.TC) *reinterpret_cast<f32x4*>(out + i) = z;
        else
            for (int j = 0; j < 4 && i + j < n; ++j) out[i + j] = z[j];
    }
}

// ---------------------------------------------------------------------------------------
// RePaint / outpainting variant of the sampler update (long-sequence windows):
//   x0      <- gt on the kept region                                  (gaussian_diffusion.py:492-501)
//   sample  <- p_sample / ddim_sample of (x_t, x0)
//   DDIM only: sample <- sqrt(ab_prev) gt + sqrt(1-ab_prev) gt_noise on the kept region, cross-faded
//   into the model's sample over the first blend_len frames (weights blend_w)      (:855-877)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sampler_inpaint_k(const float* __restrict__ x_t, const float* __restrict__ o_text,
                                                         const float* __restrict__ o_none, const float* __restrict__ noise,
                                                         InpaintArgs ip, float* __restrict__ x_prev,
                                                         float* __restrict__ x0_out, long n, SamplerCoefs c) {
    const float sigma_ddpm = c.nonzero * expf(0.5f * c.log_var);
    float sq_abp = 0.f, dir = 0.f, sigma = 0.f, nw = 0.f;
    if (c.mode == 1) {
        sigma = c.eta * sqrtf((1.f - c.ab_prev) / (1.f - c.ab)) * sqrtf(1.f - c.ab / c.ab_prev);
        sq_abp = sqrtf(c.ab_prev);
        dir = sqrtf(1.f - c.ab_prev - sigma * sigma);
        nw = sqrtf(1.f - c.ab_prev);
    }
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float x = x_t[i];
        const bool keep = ip.keep[i] != 0;
        const float g = keep ? ip.gt[i] : 0.f;
        const float x0 = keep ? g : o_text[i] * c.text_coef + o_none[i] * c.none_coef;
        float out;
        if (c.mode == 0) {
            out = c.c1 * x0 + c.c2 * x + sigma_ddpm * noise[i];
        } else {
            const float eps = (c.sqrt_recip * x - x0) / c.sqrt_recipm1;
            out = x0 * sq_abp + dir * eps + c.nonzero * sigma * noise[i];
            if (keep) {
                float wg = sq_abp * g + nw * ip.gt_noise[i];
                const int frame = (int)((i / ip.C) % ip.T);
                if (frame < ip.blend_len) {
                    const float lw = ip.blend_w[frame];
                    wg = wg * (1.f - lw) + out * lw;
                }
                out = wg;
            }
        }
        x_prev[i] = out;
        if (x0_out) x0_out[i] = x0;
    }
}

// Y[r][0:Cp] = X[r][0:C] zero-extended: the pose rows (322 / 263 / 251 floats, 8-byte aligned at best) become
// 16-byte aligned rows of the encoder GEMM's k-step multiple, so that GEMM takes its vector-load fast path
__global__ __launch_bounds__(256) void pad_rows_k(const float* __restrict__ X, float* __restrict__ Y, long rows, int C, int Cp) {
    const long n = rows * Cp;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long r = i / Cp;
        const int c = (int)(i % Cp);
        Y[i] = c < C ? X[r * C + c] : 0.f;
    }
}

// q_sample (gaussian_diffusion.py:416-421) is three tensor ops: two products, each rounded, then their sum (no FMA)
__device__ __forceinline__ float axpby_unfused(float a, float x, float b, float y) {
#pragma clang fp contract(off)
    const float p0 = a * x;
    const float p1 = b * y;
    return p0 + p1;
}

// the same pass with the reference's per-step seeding of the first frames (SeedArgs, mc_kernels.h): the seeded value goes to
// the padded copy AND back into X (p_sample / ddim_sample overwrite x in place before the network sees it)
__global__ __launch_bounds__(256) void pad_rows_seeded_k(float* __restrict__ X, float* __restrict__ Y, long rows, int C, int Cp,
                                                         SeedArgs sd) {
    const long n = rows * Cp;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long r = i / Cp;
        const int c = (int)(i % Cp);
        if (c >= C) { Y[i] = 0.f; continue; }
        const int t = (int)(r % sd.T);
        const long b = r / sd.T;
        float v = X[r * C + c];
        bool seeded = false;
        if (t < sd.pre_len) {
            const long j = (b * sd.pre_len + t) * C + c;
            v = axpby_unfused(sd.sqrt_ab, sd.pre[j], sd.sqrt_1mab, sd.pre_noise[j]);
            seeded = true;
        }
        if (t < 2) {
            for (int k = 0; k < sd.num_transl; ++k)
                if (sd.transl_channel[k] == c) { v = sd.transl_value[k][t]; seeded = true; }
        }
        if (seeded) X[r * C + c] = v;
        Y[i] = v;
    }
}

// split-K reduction: out[r][n] = sum_s part[s][r][n] (s ascending: deterministic) + bias[n] + res[r][n]
__global__ __launch_bounds__(256) void splitk_reduce_k(const float* __restrict__ part, int S, long MN, int N,
                                                      const float* __restrict__ bias, const float* __restrict__ res,
                                                      float* __restrict__ out, const int* __restrict__ dyn_tiles) {
    if (dyn_tiles) S = mc_mlp_dyn_ways(*dyn_tiles);       // the producer chose its ways on the device (MlpArgs::dyn_split)
    const long n4 = MN >> 2;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        f32x4 v = *reinterpret_cast<const f32x4*>(part + 4 * i);
        for (int s = 1; s < S; ++s) v += *reinterpret_cast<const f32x4*>(part + (long)s * MN + 4 * i);
        if (bias) v += *reinterpret_cast<const f32x4*>(bias + (4 * i) % N);
        if (res) v += *reinterpret_cast<const f32x4*>(res + 4 * i);
        *reinterpret_cast<f32x4*>(out + 4 * i) = v;
    }
}

// out = a x + b noise  (the forward "undo" step of the resampling schedule, gaussian_diffusion.py:429-435)
__global__ __launch_bounds__(256) void axpby_k(const float* __restrict__ x, const float* __restrict__ y, float a, float b,
                                               float* __restrict__ out, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        out[i] = a * x[i] + b * y[i];
}

__global__ __launch_bounds__(256) void cfg_combine_tab_k(const float* __restrict__ x, const float* __restrict__ y,
                                                         const SamplerCoefs* __restrict__ table, const int* __restrict__ step_ptr,
                                                         float* __restrict__ out, long n) {
    const float a = table[*step_ptr].text_coef, b = table[*step_ptr].none_coef;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        out[i] = a * x[i] + b * y[i];
}

// The CFG combine of the folded decoder tail runs on two row sets (h and a): both in one launch, blockIdx.y picks the set.
// Coefficients by value, or (graph replay) from the device table at *step_ptr.
struct AxpbySet { const float* x; const float* y; float* out; };
__global__ __launch_bounds__(256) void axpby_pair_k(AxpbySet s0, AxpbySet s1, float a, float b, const SamplerCoefs* __restrict__ table,
                                                    const int* __restrict__ step_ptr, long n) {
    if (table) { a = table[*step_ptr].text_coef; b = table[*step_ptr].none_coef; }
    const AxpbySet s = blockIdx.y ? s1 : s0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        s.out[i] = a * s.x[i] + b * s.y[i];
}

// The two combines with the CFG weights per request row (mc_sample_rows): element i lies in row i / D of [B T][D], request row
// (i / D / T) % B, and takes coefs[that].{text_coef, none_coef}.  The expressions are those of axpby_k / axpby_pair_k.
__device__ __forceinline__ long cfg_row(long i, int D, int T, int B) { return (i / D / T) % B; }
__global__ __launch_bounds__(256) void axpby_rows_k(const float* __restrict__ x, const float* __restrict__ y,
                                                    const SamplerCoefs* __restrict__ coefs, int D, int T, int B,
                                                    float* __restrict__ out, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long rb = cfg_row(i, D, T, B);
        const float a = coefs[rb].text_coef, b = coefs[rb].none_coef;
        out[i] = a * x[i] + b * y[i];
    }
}
__global__ __launch_bounds__(256) void axpby_pair_rows_k(AxpbySet s0, AxpbySet s1, const SamplerCoefs* __restrict__ coefs, int D, int T,
                                                         int B, long n) {
    const AxpbySet s = blockIdx.y ? s1 : s0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long rb = cfg_row(i, D, T, B);
        const float a = coefs[rb].text_coef, b = coefs[rb].none_coef;
        s.out[i] = a * s.x[i] + b * s.y[i];
    }
}

__global__ void set_int_k(int* dst, int value) { *dst = value; }
// tests only: hold a stream for `ticks` of the 100 MHz s_memtime counter (one lane; mc_ctx_set_option("dbg_delay_us"))
__global__ void spin_k(long ticks) {
    const long long t0 = (long long)wall_clock64();
    while ((long long)wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}

}  // namespace

int mc_launch_ln_rows(const float* X, long ldx, int x_col, const float* gamma, const float* beta,
                      const float* add, int add_mod, float* Y, long ldy, long rows, int L, hipStream_t s) {
    const int lpr = L / 4;
    MC_REQUIRE(L % 4 == 0 && lpr >= 1 && lpr <= 64 && (lpr & (lpr - 1)) == 0, "ln_rows: unsupported L=%d", L);
    if (rows <= 0) return MC_OK;
    const int rpb = 256 / lpr;
    hipLaunchKernelGGL(ln_rows_k, dim3(cdiv(rows, rpb)), dim3(256), 0, s, X, ldx, x_col, gamma, beta, add,
                       add_mod > 0 ? add_mod : 1, Y, ldy, rows, L);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int mc_launch_film_rows(const float* Y1, const float* Y2, const float* gamma, const float* beta,
                        const float* ss, float* A, long rows, int D, hipStream_t s, TwinAlias y1_alias, long row0, StepRef step,
                        int y1_parts, long y1_pstride, int planes, long plane_stride, const RowTab* rt) {
    MC_REQUIRE(D % 4 == 0 && D <= FILM_MAXC * 256, "film_rows: unsupported D=%d", D);
    MC_REQUIRE(planes >= 0 && (planes & 3) <= 2 && (planes & ~7) == 0 && (!(planes & 4) || ((planes & 3) != 0 && rows % 32 == 0 && D % 16 == 0)),
               "film_rows: planes=%d (rows=%ld D=%d)", planes, rows, D);
    if (rows <= 0) return MC_OK;
    const long nwg = (planes & 4) ? (long)cdiv(rows / 32, 8) * 64 : (long)cdiv(rows, 4);
    const size_t lds = (planes & 4) ? (size_t)(planes & 3) * 4 * (D + 8) * 2 : 0;
    if (rt) {        // per-row schedule indices: `ss` is the table's row of index 0
        MC_REQUIRE(rt->step && rt->B > 0 && rt->T > 0 && !step.ptr, "film_rows: row steps need a table, B, T and no graph step");
        hipLaunchKernelGGL((film_rows_k<FilmRowSteps>), dim3((unsigned)nwg), dim3(256), lds, s, Y1, Y2, gamma, beta, ss, A, rows, D, y1_alias, row0, step,
                           y1_parts < 1 ? 1 : y1_parts, y1_pstride, planes, plane_stride, FilmRowSteps{rt->step, rt->B, rt->T, 2L * D});
    } else
        hipLaunchKernelGGL((film_rows_k<FilmOneStep>), dim3((unsigned)nwg), dim3(256), lds, s, Y1, Y2, gamma, beta, ss, A, rows, D, y1_alias, row0, step,
                           y1_parts < 1 ? 1 : y1_parts, y1_pstride, planes, plane_stride, FilmOneStep{});
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int mc_launch_timestep_embedding(const int* t_orig, float* te, int S, int D, hipStream_t s) {
    hipLaunchKernelGGL(timestep_embedding_k, dim3(cdiv((long)S * D, 256)), dim3(256), 0, s, t_orig, te, S, D);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int mc_launch_add_rows(float* out, const float* a, const float* b, const float* bias, long rows, int D, hipStream_t s) {
    MC_REQUIRE(D % 4 == 0, "add_rows: D %% 4 != 0");
    if (rows <= 0) return MC_OK;
    long blocks = (rows * (D / 4) + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(add_rows_k, dim3((unsigned)blocks), dim3(256), 0, s, out, a, b, bias, rows, D);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int mc_launch_silu(const float* X, float* Y, long n, hipStream_t s) {
    hipLaunchKernelGGL(silu_k, dim3(cdiv(n, 256)), dim3(256), 0, s, X, Y, n);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int mc_launch_softmax_rows_small(const float* W, float* out, int rows, int cols, hipStream_t s) {
    hipLaunchKernelGGL(softmax_rows_small_k, dim3(cdiv(rows, 64)), dim3(64), 0, s, W, out, rows, cols);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

// The sampler family's one launcher: every check, the vector rule, the grid and the RNG x VEC selection stated once.
namespace {
template <class F> void with_bool(bool v, F&& f) { if (v) f(std::true_type{}); else f(std::false_type{}); }
}  // namespace
int mc_launch_sampler(const SamplerForm& f, hipStream_t s) {
    const bool ms = f.mode == 2, rows = f.rt != nullptr, seam = f.seam || f.seam_rows;
    const char* const form = f.seam_rows ? (f.edit ? "edited seam rows" : "seam rows") : f.seam ? "seam" : f.edit ? "edited rows" : rows ? "rows" : "uniform";
    MC_REQUIRE(f.x_t && f.out_text && f.out_none && f.x_prev && (f.n >= 0 || !ms), "sampler update (%s): null operand", form);
    MC_REQUIRE(f.mode >= 0 && f.mode <= 2, "sampler update (%s): unknown sampler mode %d", form, f.mode);
    MC_REQUIRE((!f.edit || (rows && !f.seam)) && (!f.seam_rows || rows) && (!f.seam || (!rows && !f.seam_rows)) && (!f.table || (!rows && !seam)),
               "sampler update (%s): no such form", form);
    MC_REQUIRE(!ms || rows || f.table || f.c.mode == 2, "sampler update (%s): coefficients of mode %d in a launch of mode 2", form, f.c.mode);
    // rows of TC elements
    int TC = f.TC, C = 0;
    if (seam) {
        const int T = f.seam ? f.seam->T : f.seam_rows->T, ov = f.seam ? f.seam->ov : f.seam_rows->ov;
        C = f.seam ? f.seam->C : f.seam_rows->C;
        MC_REQUIRE(f.seam ? f.seam->flags && f.seam->w : f.seam_rows->rows && f.seam_rows->w, "sampler update (%s): no seam table", form);
        MC_REQUIRE(T > 0 && C > 0 && ov > 0 && 2 * ov <= T, "sampler update (%s): overlap %d outside (0, %d / 2]", form, ov, T);
        MC_REQUIRE((long)T * C <= 0x7fffffffL, "sampler update (%s): a window of %d x %d floats", form, T, C);
        TC = T * C;
        MC_REQUIRE(f.n % TC == 0, "sampler update (%s): %ld elements are no whole windows of %d", form, f.n, TC);
        MC_REQUIRE(!f.seam_rows || (f.n <= 0x7fffffffL && TC >= 4), "sampler update (%s): %ld floats in rows of %d (the kernel indexes in 32 bits; a row holds at least 4)", form, f.n, TC);
    }
    MC_REQUIRE(!rows || (f.rt->coefs && f.rt->B > 0 && TC > 0 && f.n == (long)f.rt->B * TC), "sampler update (%s): %ld elements for %d rows of %d", form, f.n,
               rows ? f.rt->B : 0, TC);
    // noise (modes 0 / 1): the tensor, or drawn -- from rng (keyed per row where keys is set), under per-row schedules from keys at rt->draw
    const bool drawn = !ms && !f.noise;
    MC_REQUIRE(!f.keys || (f.keys->keys && f.keys->TC > 0 && (rows || seam ? f.keys->TC == TC : f.n % f.keys->TC == 0)),
               "sampler update (%s): row keys for rows of %d elements, %ld in all", form, f.keys ? f.keys->TC : 0, f.n);
    MC_REQUIRE(!drawn || rows || f.rng, "sampler update (%s): neither a noise tensor nor a Philox draw given", form);
    MC_REQUIRE(!drawn || !rows || (f.keys && f.rt->draw), "sampler update (%s): no noise tensor, and no seed table / draw numbers", form);
    // the history (mode 2)
    float* const hist = ms ? f.x0_hist : nullptr;
    MC_REQUIRE(!ms || hist, "sampler update (%s): mode 2 without a history buffer", form);
    MC_REQUIRE(!ms || (hist != f.x_t && hist != f.x_prev && hist != f.x0_out && hist != f.out_text && hist != f.out_none && (!f.edit || hist != f.edit->gt)),
               "sampler update (%s): the history buffer aliases another operand", form);
    EditTab et = f.edit ? *f.edit : EditTab();
    if (f.edit) {
        MC_REQUIRE(et.gt && et.keep, "sampler update (%s): no gt / keep table", form);
        if (drawn || f.mode != 1) et.gt_noise = nullptr;      // (both noises come from the rows' streams; modes 0 and 2 take no second one)
        MC_REQUIRE(f.mode != 1 || drawn || et.gt_noise, "sampler update (%s): mode 1 beside a noise tensor needs the kept region's noise tensor", form);
        et.kword = (uintptr_t)et.keep % 4 == 0 ? 1 : 0;
    }
    const PadOut po = f.pad ? *f.pad : PadOut();
    MC_REQUIRE(!po.xpad || (po.C > 0 && po.Cp >= po.C && (!seam || po.C == C)), "sampler update (%s): bad padded-copy shape", form);
    if (f.n <= 0) return MC_OK;
    // the vector rule: f32x4 loads / stores when every stream the form reads or writes is 16-byte aligned (torch / workspace allocations
    // are; out2 + B*T*C or noise + k*n need not be: C = 263 / 251 / 322 with an odd B*T) -- otherwise the element form of the same
    // kernel (same groups, same Philox counters)
    const bool vec = ((uintptr_t)f.x_t | (uintptr_t)f.out_text | (uintptr_t)f.out_none | (uintptr_t)f.x_prev | (uintptr_t)f.x0_out |
                      (uintptr_t)(ms ? hist : f.noise) | (uintptr_t)et.gt | (uintptr_t)et.gt_noise) % 16 == 0;
    int blocks = cdiv((f.n + 3) / 4, 256);
    if (blocks > 2048) blocks = 2048;
    const RngArgs ra = drawn && f.rng ? *f.rng : RngArgs();
    const RowKeys rk{drawn && f.keys ? f.keys->keys : nullptr, TC};
    const RowNoise rn{ra, f.keys ? *f.keys : RowKeys()};
    const bool row_noise = drawn && f.keys;            // (uniform entries: the rows' own streams at the call's draw)
    const float tc = f.c.text_coef, nc = f.c.none_coef;
#define MC_GO(K, ...) hipLaunchKernelGGL(K, dim3(blocks), dim3(256), 0, s, f.x_t, f.out_text, f.out_none, __VA_ARGS__)
    with_bool(vec, [&](auto vec_t) {
        constexpr bool V = decltype(vec_t)::value;
        with_bool(drawn, [&](auto drawn_t) {
            constexpr bool R = decltype(drawn_t)::value;
            if (f.seam_rows && f.edit) MC_GO((sampler_seam_edit_rows_k<R, V>), f.noise, hist, et, f.x_prev, f.x0_out, (uint32_t)f.n, tc, nc, f.rt->coefs, rk, f.rt->draw, *f.seam_rows, f.mode, po);
            else if (f.seam_rows) MC_GO((sampler_seam_rows_k<R, V>), f.noise, hist, f.x_prev, f.x0_out, (uint32_t)f.n, tc, nc, f.rt->coefs, rk, f.rt->draw, *f.seam_rows, ms ? 1 : 0, po);
            else if (f.seam && row_noise) MC_GO((sampler_seam_k<true, V, RowNoise>), f.noise, hist, f.x_prev, f.x0_out, f.n, f.c, *f.seam, rn, po);
            else if (f.seam) MC_GO((sampler_seam_k<R, V>), f.noise, hist, f.x_prev, f.x0_out, f.n, f.c, *f.seam, ra, po);
            else if (f.edit && ms) MC_GO((sampler_multistep_edit_rows_k<V>), hist, et, f.x_prev, f.x0_out, f.n, tc, nc, f.rt->coefs, TC, po);
            else if (f.edit) MC_GO((sampler_edit_rows_k<R, V>), f.noise, et, f.x_prev, f.x0_out, f.n, tc, nc, f.rt->coefs, rk, f.rt->draw, po);
            else if (rows && ms) MC_GO((sampler_multistep_rows_k<V>), hist, f.x_prev, f.x0_out, f.n, tc, nc, f.rt->coefs, TC, po);
            else if (rows) MC_GO((sampler_update_rows_k<R, V>), f.noise, f.x_prev, f.x0_out, f.n, tc, nc, f.rt->coefs, rk, f.rt->draw, po);
            else if (ms) MC_GO((sampler_multistep_k<V>), hist, f.x_prev, f.x0_out, f.n, f.c, f.table, f.step_ptr, po);
            else if (row_noise) MC_GO((sampler_update_k<true, V, RowNoise>), f.noise, f.x_prev, f.x0_out, f.n, f.c, f.table, f.step_ptr, rn, po);
            else MC_GO((sampler_update_k<R, V>), f.noise, f.x_prev, f.x0_out, f.n, f.c, f.table, f.step_ptr, ra, po);
        });
    });
#undef MC_GO
    MC_LAUNCH_CHECK();
    return MC_OK;
}


int mc_launch_axpby_rows(const float* x, const float* y, const RowTab& rt, int D, float* out, long n, hipStream_t s) {
    MC_REQUIRE(rt.coefs && rt.B > 0 && rt.T > 0 && D > 0, "axpby rows: no coefficient table");
    if (n <= 0) return MC_OK;
    int blocks = cdiv(n, 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(axpby_rows_k, dim3(blocks), dim3(256), 0, s, x, y, rt.coefs, D, rt.T, rt.B, out, n);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int mc_launch_axpby_pair_rows(const float* x0, const float* y0, float* out0, const float* x1, const float* y1, float* out1, const RowTab& rt,
                              int D, long n, hipStream_t s) {
    MC_REQUIRE(rt.coefs && rt.B > 0 && rt.T > 0 && D > 0, "axpby pair rows: no coefficient table");
    if (n <= 0) return MC_OK;
    int blocks = cdiv(n, 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(axpby_pair_rows_k, dim3(blocks, 2), dim3(256), 0, s, AxpbySet{x0, y0, out0}, AxpbySet{x1, y1, out1}, rt.coefs, D, rt.T, rt.B, n);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int mc_launch_philox_fill(float* out, uint32_t* bits, long n, RngArgs rng, hipStream_t s) {
    if (n <= 0) return MC_OK;
    int blocks = cdiv((n + 3) / 4, 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(philox_fill_k, dim3(blocks), dim3(256), 0, s, out, bits, n, rng);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int mc_launch_philox_rows_fill(float* out, int B, RowKeys rk, RngArgs rng, hipStream_t s) {
    MC_REQUIRE(out && rk.keys && rk.TC > 0 && B >= 0, "row draw: bad argument");
    const long n = (long)B * rk.TC;
    if (n == 0) return MC_OK;
    int blocks = cdiv((n + 3) / 4, 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(philox_rows_fill_k, dim3(blocks), dim3(256), 0, s, out, n, rk, rng, (uintptr_t)out % 16 == 0 ? 1 : 0);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int mc_launch_cfg_combine_tab(const float* x, const float* y, const SamplerCoefs* table, const int* step_ptr, float* out, long n,
                              hipStream_t s) {
    if (n <= 0) return MC_OK;
    int blocks = cdiv(n, 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(cfg_combine_tab_k, dim3(blocks), dim3(256), 0, s, x, y, table, step_ptr, out, n);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int mc_launch_axpby_pair(const float* x0, const float* y0, float* out0, const float* x1, const float* y1, float* out1, float a, float b,
                         const SamplerCoefs* table, const int* step_ptr, long n, hipStream_t s) {
    if (n <= 0) return MC_OK;
    int blocks = cdiv(n, 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(axpby_pair_k, dim3(blocks, 2), dim3(256), 0, s, AxpbySet{x0, y0, out0}, AxpbySet{x1, y1, out1}, a, b, table, step_ptr, n);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int mc_launch_spin(long ticks, hipStream_t s) {
    hipLaunchKernelGGL(spin_k, dim3(1), dim3(1), 0, s, ticks);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
int mc_launch_set_int(int* dst, int value, hipStream_t s) {
    hipLaunchKernelGGL(set_int_k, dim3(1), dim3(1), 0, s, dst, value);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int mc_launch_sampler_inpaint(const float* x_t, const float* out_text, const float* out_none, const float* noise,
                              InpaintArgs ip, float* x_prev, float* x0_out, long n, SamplerCoefs c, hipStream_t s) {
    MC_REQUIRE(ip.gt && ip.keep && ip.T > 0 && ip.C > 0, "inpaint: gt / keep mask / shape missing");
    MC_REQUIRE(c.mode == 0 || ip.gt_noise, "inpaint: DDIM needs the gt re-noising draw");
    MC_REQUIRE(ip.blend_len == 0 || ip.blend_w, "inpaint: blend weights missing");
    int blocks = cdiv(n, 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(sampler_inpaint_k, dim3(blocks), dim3(256), 0, s, x_t, out_text, out_none, noise, ip, x_prev,
                       x0_out, n, c);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int mc_launch_axpby(const float* x, const float* y, float a, float b, float* out, long n, hipStream_t s) {
    if (n <= 0) return MC_OK;
    int blocks = cdiv(n, 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(axpby_k, dim3(blocks), dim3(256), 0, s, x, y, a, b, out, n);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int mc_launch_pad_rows(const float* X, float* Y, long rows, int C, int Cp, hipStream_t s) {
    if (rows <= 0) return MC_OK;
    int blocks = cdiv(rows * Cp, 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(pad_rows_k, dim3(blocks), dim3(256), 0, s, X, Y, rows, C, Cp);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int mc_launch_pad_rows_seeded(float* X, float* Y, long rows, int C, int Cp, const SeedArgs& sd, hipStream_t s) {
    if (rows <= 0) return MC_OK;
    MC_REQUIRE(sd.T >= 1 && sd.pre_len >= 0 && sd.pre_len <= sd.T && sd.num_transl >= 0 && sd.num_transl <= 8, "bad seed arguments");
    MC_REQUIRE(sd.pre_len == 0 || (sd.pre && sd.pre_noise), "pre_seq seeding without pre_seq / noise");
    int blocks = cdiv(rows * Cp, 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(pad_rows_seeded_k, dim3(blocks), dim3(256), 0, s, X, Y, rows, C, Cp, sd);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int mc_launch_splitk_reduce(const float* part, int S, long M, int N, const float* bias, const float* res, float* out,
                            hipStream_t s, const int* dyn_tiles) {
    MC_REQUIRE(N % 4 == 0 && S >= 1, "split-K reduce: N=%d S=%d", N, S);
    const long MN = M * N;
    if (MN <= 0) return MC_OK;
    int blocks = cdiv(MN / 4, 256);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(splitk_reduce_k, dim3(blocks), dim3(256), 0, s, part, S, MN, N, bias, res, out, dyn_tiles);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
