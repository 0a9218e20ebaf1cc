// Audio onset detection of the speech-to-gesture test on the device: what librosa 0.10.1's onset.onset_detect computes with its
// defaults, the call of the reference's alignment.load_audio (mogen/datasets/EMAGE_2024/utils/metric.py:64-76).  The algorithm is
// stated once, in float64, in tests/onset_ref.py; n_fft is 2048 here.
//   frames    frame f, sample k = y[f hop + k - 1024], zero outside the clip (center=True, constant padding), F = 1 + N / hop
//   spectrum  C[f][c] = sum_k frame[f][k] T[k][c]: T [2048][2050] holds the window times cos (column 2b) and -sin (column 2b + 1)
//   power     P[f][b] = C[f][2b]^2 + C[f][2b+1]^2, 1025 bins;  mel M = P W^T;  S = 10 log10(max(1e-10, M))
//   envelope  env[j] = mean over the mel rows of max(0, S'[j-lag+1] - S'[j-lag]), S' = max(S, max(S) - 80), lag = 1 + 1024 / hop;
//             env[j] = 0 for j < lag
//   pick      normalise to [0, 1]; n is an onset iff env[n] is the maximum of [n - pre_max, n + post_max), env[n] >= the mean of
//             [n - pre_avg, n + post_avg) + delta, env[n] > 0 and n > the last onset + wait (windows truncated at the array's ends)
// onset_melpow_k is the hot part, an implicit GEMM on the exact fp32 MFMA.  It is run TRANSPOSED, D[c][f] = sum_k T[k][c] frame[f][k]:
// the 32x32 result has its column on the lane and its rows in the 16 registers (row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)), so
// with the table as the MFMA's first operand the re and im columns 2b, 2b+1 of a bin are the registers 2p, 2p+1 of ONE lane and
// the power needs no lane movement; with the frames as the first operand they would sit in neighbouring lanes.  One workgroup
// takes FT = 32 frames x 128 table columns (one 32x32 tile per wave); the frames are never materialised: the workgroup stages the
// one span of 31 hop + 2048 samples they share into LDS (4 floats of padding per 512, so the 32 frames of a 16-byte fragment
// read land in different banks at hop 512) and each lane reads its fragments from it.  The sum over k runs as four chains (the
// four quarters of the frame) in four accumulators, added at the end: a shorter fmaf chain rounds less.
// onset_mel_k projects through the work buffer (P is written bin-major, so both kernels touch it coalesced) over each mel row's
// non-zero bins only (onset_melrange_k finds them; adding the zeros would change nothing), takes the dB in fp64 and leaves one
// maximum per workgroup.  onset_flux_k reduces those maxima (no atomics; a maximum does not depend on the order anyway), clamps
// on the fly and sums the 128 rows in order, in fp64.  onset_pick_k is one workgroup: min / max, the two windows per frame, then
// one wave walks the candidates 64 at a time (ballot) for the left-to-right `wait` rule.  Two runs give the same bits.
#include "mc_common.h"
#include "../../include/motioncraft_amd.h"
#include <float.h>
#include <math.h>

namespace {

constexpr int NFFT = MC_ONSET_N_FFT, NBIN = NFFT / 2 + 1, NCOL = 2 * NBIN;
constexpr int FT = 32;                       // frames per workgroup of onset_melpow_k (the row tile)
constexpr int CT = 128;                      // table columns per workgroup: one 32-wide MFMA tile per wave
constexpr int MAX_HOP = MC_ONSET_MAX_HOP, MAX_MELS = MC_ONSET_MAX_MELS, MAX_FRAMES = 1 << 20, MAX_WINDOW = 1 << 16;
constexpr int SPAN = (FT - 1) * MAX_HOP + NFFT;
__host__ __device__ constexpr int lds_at(int p) { return p + 4 * (p >> 9); }
constexpr int SPAN_LDS = lds_at(SPAN - 1) + 1;
constexpr int MEL_SPLIT = 8;                 // onset_mel_k: workgroups per 64 frames, 16 mel rows each

__global__ __launch_bounds__(256) void onset_melpow_k(const float* __restrict__ y, long n, const float* __restrict__ T, int hop, int F, int fstride,
                                                      float* __restrict__ Pt) {
    __shared__ __attribute__((aligned(16))) float span[SPAN_LDS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int f0 = blockIdx.x * FT;
    const long s0 = (long)f0 * hop - NFFT / 2;
    const int len = (FT - 1) * hop + NFFT;
    for (int i = tid; i < len; i += 256) {
        const long s = s0 + i;
        span[lds_at(i)] = (s >= 0 && s < n) ? y[s] : 0.f;
    }
    __syncthreads();
    const int c0 = blockIdx.y * CT + w * 32;
    // Known cost: 2050 = 16 x 128 + 2, so a 17th column block exists for the Nyquist bin alone; it stages the span again and its
    // wave 0 runs a whole tile for one value per frame, about 6 % of the DFT work.  (That bin is sum_k (-1)^k w[k] y[k] and could
    // be a reduction of its own.)
    if (c0 >= NCOL) return;                                          // the last column block holds 2 columns: waves 1..3 have none
    const int r = lane & 31, h = lane >> 5;
    const float* tp = T + min(c0 + r, NCOL - 1);                     // a column past the table reads the last one; its result is dropped
    const int a0 = r * hop + 4 * h;                                  // this lane's frame, its half of each 8-sample step
    f32x16 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[q][i] = 0.f;
    // one step = 8 samples of each quarter q: lane half h carries samples 4h .. 4h+3 of the 8 in its fragment (the MFMA's two k
    // slots are whatever both operands agree on).  The operands of step s+1 are requested before the 16 MFMAs of step s.
    f32x4 an[4], tn[4];
    auto load = [&](int k0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = q * (NFFT / 4) + k0;
            an[q] = *reinterpret_cast<const f32x4*>(&span[lds_at(a0 + k)]);
            const float* t = tp + (long)(k + 4 * h) * NCOL;
            tn[q] = f32x4{t[0], t[NCOL], t[2 * NCOL], t[3 * NCOL]};
        }
    };
    load(0);
    for (int k0 = 0; k0 < NFFT / 4; k0 += 8) {
        f32x4 ac[4], tc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) ac[q] = an[q], tc[q] = tn[q];
        if (k0 + 8 < NFFT / 4) load(k0 + 8);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(tc[q][i], ac[q][i], acc[q], 0, 0, 0);
    }
    const int f = f0 + r;
    if (f >= F) return;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const float re = (acc[0][2 * p] + acc[1][2 * p]) + (acc[2][2 * p] + acc[3][2 * p]);
        const float im = (acc[0][2 * p + 1] + acc[1][2 * p + 1]) + (acc[2][2 * p + 1] + acc[3][2 * p + 1]);
        const int bin = (c0 + 2 * (p & 1) + 8 * (p >> 1) + 4 * h) >> 1;      // register 2p is row 2 (p & 1) + 8 (p >> 1) + 4 h of the tile
        if (bin < NBIN) Pt[(long)bin * fstride + f] = re * re + im * im;
    }
}

// [lo, hi) of each mel row's non-zero weights (lo = hi = 0 for an empty row)
__global__ __launch_bounds__(64) void onset_melrange_k(const float* __restrict__ W, int* __restrict__ ranges) {
    const float* wr = W + (long)blockIdx.x * NBIN;
    int lo = NBIN, hi = 0;
    for (int b = threadIdx.x; b < NBIN; b += 64)
        if (wr[b] != 0.f) lo = min(lo, b), hi = max(hi, b + 1);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lo = min(lo, __shfl_xor(lo, o, 64)), hi = max(hi, __shfl_xor(hi, o, 64));
    if (threadIdx.x == 0) ranges[2 * blockIdx.x] = hi ? lo : 0, ranges[2 * blockIdx.x + 1] = hi;
}

__device__ __forceinline__ float wave_max_f32(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// lane = frame; workgroup y of the MEL_SPLIT takes the rows 32 i + 4 y + wave (a low row has a few bins, a high one some fifty)
__global__ __launch_bounds__(256) void onset_mel_k(const float* __restrict__ Pt, int fstride, int F, const float* __restrict__ W,
                                                   const int* __restrict__ ranges, int n_mels, float* __restrict__ Sdb, float* __restrict__ blockmax) {
    __shared__ float sh[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int f = blockIdx.x * 64 + lane, fc = min(f, F - 1);
    float mx = -INFINITY;
    for (int m = 4 * blockIdx.y + w; m < n_mels; m += 4 * MEL_SPLIT) {
        const int lo = ranges[2 * m], hi = ranges[2 * m + 1];
        const float* wr = W + (long)m * NBIN;
        float acc = 0.f;
        for (int b = lo; b < hi; ++b) acc = fmaf(wr[b], Pt[(long)b * fstride + fc], acc);
        const float s = (float)(10.0 * log10((double)fmaxf(acc, 1e-10f)));
        if (f < F) {
            Sdb[(long)m * fstride + f] = s;
            mx = fmaxf(mx, s);
        }
    }
    mx = wave_max_f32(mx);
    if (lane == 0) sh[w] = mx;
    __syncthreads();
    if (tid == 0) blockmax[blockIdx.y * gridDim.x + blockIdx.x] = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

__global__ __launch_bounds__(256) void onset_flux_k(const float* __restrict__ Sdb, int fstride, int F, int n_mels, const float* __restrict__ blockmax,
                                                    int n_max, int lag, float* __restrict__ env) {
    __shared__ float sh[4];
    const int tid = threadIdx.x;
    float mx = -INFINITY;
    for (int i = tid; i < n_max; i += 256) mx = fmaxf(mx, blockmax[i]);
    mx = wave_max_f32(mx);
    if ((tid & 63) == 0) sh[tid >> 6] = mx;
    __syncthreads();
    const double floor_db = (double)fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3])) - 80.0;
    const int j = blockIdx.x * 256 + tid;
    if (j >= F) return;
    if (j < lag) {
        env[j] = 0.f;
        return;
    }
    const float* s = Sdb + (j - lag);
    double acc = 0.0;
    for (int m = 0; m < n_mels; ++m) {
        const double a = fmax((double)s[(long)m * fstride], floor_db), b = fmax((double)s[(long)m * fstride + 1], floor_db);
        acc += fmax(0.0, b - a);
    }
    env[j] = (float)(acc / (double)n_mels);
}

__global__ __launch_bounds__(256) void onset_pick_k(const float* __restrict__ env, int F, int pre_max, int post_max, int pre_avg, int post_avg,
                                                    double delta, int wait, int normalize, uint8_t* __restrict__ mask, int* __restrict__ count) {
    __shared__ double smin[4], smax[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double mn = INFINITY, mx = -INFINITY;
    for (int i = tid; i < F; i += 256) mn = fmin(mn, (double)env[i]), mx = fmax(mx, (double)env[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mn = fmin(mn, __shfl_xor(mn, o, 64)), mx = fmax(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) smin[w] = mn, smax[w] = mx;
    __syncthreads();
    mn = fmin(fmin(smin[0], smin[1]), fmin(smin[2], smin[3]));
    mx = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
    // env -= min; env /= max + tiny, in fp64; an all-zero envelope has no onsets (onset_detect returns before the peak pick)
    const bool live = !(normalize && mn == 0.0 && mx == 0.0);
    const double sub = normalize ? mn : 0.0, div = normalize ? (mx - mn) + DBL_MIN : 1.0;
    auto x = [&](int i) { return ((double)env[i] - sub) / div; };
    for (int n = tid; n < F; n += 256) {
        const double v = x(n);
        bool c = live && v > 0.0;
        if (c) {
            const int hi = (int)min((long)F, (long)n + post_max);
            for (int i = max(0, n - pre_max); i < hi; ++i) c = c && v >= x(i);
        }
        if (c) {
            const int lo = max(0, n - pre_avg), hi = (int)min((long)F, (long)n + post_avg);
            double s = 0.0;
            for (int i = lo; i < hi; ++i) s += x(i);
            c = v >= s / (double)(hi - lo) + delta;
        }
        mask[n] = c;
    }
    __syncthreads();                                                 // the candidates of all four waves are visible to wave 0
    if (w != 0) return;
    long last = -1 - (long)wait;
    int total = 0;
    for (int i0 = 0; i0 < F; i0 += 64) {
        const int n = i0 + lane;
        unsigned long long bits = __ballot(n < F && mask[n] != 0), keep = 0;
        if (wait > 0) {
            while (bits) {                                           // wave-uniform: every lane walks the same candidates
                const int b = __ffsll((long long)bits) - 1;
                bits &= bits - 1;
                if (i0 + b > last + wait) keep |= 1ull << b, last = i0 + b;
            }
        } else {
            keep = bits;
        }
        if (n < F) mask[n] = (keep >> lane) & 1;
        total += __popcll(keep);
    }
    if (lane == 0) *count = total;
}

struct Work {
    int F, fstride, n_max;
    int64_t pt, sdb, ranges, blockmax, bytes;          // byte offsets
};

bool work_layout(int64_t n_samples, int n_fft, int hop, int n_mels, Work& k) {
    if (n_samples < 1 || n_fft != NFFT || hop < 4 || hop > MAX_HOP || hop % 4 || n_mels < 1 || n_mels > MAX_MELS) return false;
    const int64_t F = 1 + n_samples / hop;
    if (F > MAX_FRAMES) return false;
    k.F = (int)F;
    k.fstride = cdiv(F, 64) * 64;
    k.n_max = cdiv(F, 64) * MEL_SPLIT;
    k.pt = 0;
    k.sdb = k.pt + (int64_t)NBIN * k.fstride * 4;
    k.ranges = k.sdb + (int64_t)n_mels * k.fstride * 4;
    k.blockmax = k.ranges + (int64_t)2 * n_mels * 4;
    k.bytes = (k.blockmax + (int64_t)k.n_max * 4 + 15) / 16 * 16;
    return true;
}

}  // namespace

extern "C" {

int64_t mc_onset_work_bytes(int64_t n_samples, int32_t n_fft, int32_t hop, int32_t n_mels) {
    Work k;
    return work_layout(n_samples, n_fft, hop, n_mels, k) ? k.bytes : -1;
}

int mc_onset_strength(const float* wave_dev, int64_t n_samples, const float* dft_dev, const float* mel_dev, int32_t n_fft, int32_t hop,
                      int32_t n_mels, void* work_dev, int64_t work_bytes, float* env_out_dev, void* stream) {
    MC_REQUIRE(wave_dev && dft_dev && mel_dev && work_dev && env_out_dev, "onset strength: null argument");
    Work k;
    MC_REQUIRE(work_layout(n_samples, n_fft, hop, n_mels, k),
               "onset strength: %ld samples (at least 1, at most %d frames), n_fft=%d (%d), hop=%d (a multiple of 4 in 4..%d), n_mels=%d (1..%d)",
               (long)n_samples, MAX_FRAMES, n_fft, NFFT, hop, MAX_HOP, n_mels, MAX_MELS);
    MC_REQUIRE(((uintptr_t)work_dev & 15) == 0 && work_bytes >= k.bytes,
               "onset strength: the workspace must be 16-byte aligned and hold %ld bytes (mc_onset_work_bytes), got %ld", (long)k.bytes, (long)work_bytes);
    char* base = (char*)work_dev;
    float* Pt = (float*)(base + k.pt);
    float* Sdb = (float*)(base + k.sdb);
    int* ranges = (int*)(base + k.ranges);
    float* blockmax = (float*)(base + k.blockmax);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(cdiv(k.F, FT), cdiv(NCOL, CT));
    hipLaunchKernelGGL(onset_melpow_k, grid, dim3(256), 0, s, wave_dev, (long)n_samples, dft_dev, hop, k.F, k.fstride, Pt);
    MC_LAUNCH_CHECK();
    MC_LEDGER("onset_melpow_k", grid, 2.0 * k.F * NCOL * NFFT);
    hipLaunchKernelGGL(onset_melrange_k, dim3(n_mels), dim3(64), 0, s, mel_dev, ranges);
    MC_LAUNCH_CHECK();
    hipLaunchKernelGGL(onset_mel_k, dim3(cdiv(k.F, 64), MEL_SPLIT), dim3(256), 0, s, Pt, k.fstride, k.F, mel_dev, ranges, n_mels, Sdb, blockmax);
    MC_LAUNCH_CHECK();
    hipLaunchKernelGGL(onset_flux_k, dim3(cdiv(k.F, 256)), dim3(256), 0, s, Sdb, k.fstride, k.F, n_mels, blockmax, k.n_max, 1 + NFFT / (2 * hop), env_out_dev);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int mc_onset_pick(const float* env_dev, int32_t n_frames, int32_t pre_max, int32_t post_max, int32_t pre_avg, int32_t post_avg, double delta,
                  int32_t wait, int32_t normalize, uint8_t* mask_out_dev, int32_t* count_out_dev, void* stream) {
    MC_REQUIRE(env_dev && mask_out_dev && count_out_dev, "onset pick: null argument");
    MC_REQUIRE(n_frames >= 1 && n_frames <= MAX_FRAMES, "onset pick: %d frames (1..%d)", n_frames, MAX_FRAMES);
    MC_REQUIRE(pre_max >= 0 && pre_avg >= 0 && post_max >= 1 && post_avg >= 1 && wait >= 0 && pre_max <= MAX_WINDOW && post_max <= MAX_WINDOW &&
                   pre_avg <= MAX_WINDOW && post_avg <= MAX_WINDOW && wait <= MAX_FRAMES,
               "onset pick: pre_max=%d, pre_avg=%d, wait=%d (>= 0), post_max=%d, post_avg=%d (>= 1), windows up to %d", pre_max, pre_avg, wait, post_max,
               post_avg, MAX_WINDOW);
    MC_REQUIRE(delta >= 0.0, "onset pick: delta=%g (>= 0)", delta);
    hipLaunchKernelGGL(onset_pick_k, dim3(1), dim3(256), 0, (hipStream_t)stream, env_dev, n_frames, pre_max, post_max, pre_avg, post_avg, delta, wait,
                       normalize != 0, mask_out_dev, count_out_dev);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

}  // extern "C"
