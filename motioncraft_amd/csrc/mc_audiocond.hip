// The audio condition of the speech-to-gesture configs on the device: the [samples, 2] array `onset+amplitude` that the reference's
// data loader builds on the host (mogen/datasets/EMAGE_2024/dataloaders/beat_motionx.py:398-412) and the WavEncoder reads.  The
// semantics are stated once, in numpy, in tests/audio_cond_ref.py.
//   column 0  out[i][0] = max |wave[s .. s + window - 1]|, s = min(i, n - window): the rolling maximum over the FULL windows only;
//             the last window's value is repeated over the final window - 1 samples (np.pad with constant_values = envelope[-1]),
//             it is NOT a window that shrinks towards the end of the clip
//   column 1  out[i][1] = 1 if i < n_frames and onset_mask[i], else 0.  Reference quirk, kept: onset_mask is indexed by onset FRAME
//             (hop 512, what onset_detect(units='frames') returns) and the reference writes those frame indices into the SAMPLE-indexed
//             array (onset_array[audio_onset_f] = 1.0), so the ones sit in the first n_frames samples and nowhere near the onsets' times
// The kernel is memory bound (4 B read, 8 B written per sample) and passes over HBM once.  A workgroup produces TILE samples: it stages
// |wave| of the tile plus the window - 1 samples behind it in LDS, then builds the doubling table
//   m_0 = |wave|,  m_k[i] = max(m_{k-1}[i], m_{k-1}[i + 2^(k-1)])        (m_k[i] = the maximum of the 2^k samples from i on)
// level by level between two LDS buffers, four entries per thread and step, and reads a window of any length as two overlapping
// power-of-two windows: out = max(m_p[l], m_p[l + window - 2^p]), p = floor(log2 window).  The work per sample grows with log2 of the
// window, not with the window.  A maximum of |fp32| values is exact in any order: the output equals the restatement bit for bit, and
// two runs give the same bits (no atomics, no workspace).
#include "mc_common.h"
#include "../../include/motioncraft_amd.h"

namespace {

constexpr int TILE = MC_AUDIO_COND_TILE;     // output samples per workgroup
constexpr int MAX_WINDOW = MC_AUDIO_COND_MAX_WINDOW;
constexpr int SPAN = TILE + MAX_WINDOW - 1;  // staged samples at most
// a level is written four entries at a time up to the next multiple of 4 and reads up to 8 entries past the one it starts at; both
// buffers are defined over that whole range (zeros behind the samples, and zeros in the second buffer until a level writes it), so
// the entries a level computes past its last useful one are maxima of defined values that nothing reads for a result
constexpr int SPAN_LDS = (SPAN + 3) / 4 * 4 + 8;

__global__ __launch_bounds__(256) void audio_condition_k(const float* __restrict__ wave, long n, int window, const uint8_t* __restrict__ onset_mask,
                                                         int n_frames, float2* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float buf[2][SPAN_LDS];
    const int tid = threadIdx.x;
    const long t0 = (long)blockIdx.x * TILE;
    const long last = n - window;                                    // the start of the last full window
    const long s0 = min(t0, last);                                   // a tile in the tail starts its span at the last full window
    const int len = (int)min((long)(TILE + window - 1), n - s0);     // staged samples: buf[.][j] = |wave[s0 + j]|
    const int len4 = (len + 3) & ~3;
    const float* src = wave + s0;
    if (((uintptr_t)src & 15) == 0) {
        for (int j = 4 * tid; j < len4 + 8; j += 4 * 256) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (j + 3 < len) {
                v = *reinterpret_cast<const f32x4*>(src + j);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (j + e < len) v[e] = src[j + e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fabsf(v[e]);
            *reinterpret_cast<f32x4*>(&buf[0][j]) = v;
            *reinterpret_cast<f32x4*>(&buf[1][j]) = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    } else {                                                         // a span that does not start on 16 bytes: the tail tiles, a sliced clip
        for (int j = tid; j < len4 + 8; j += 256) buf[0][j] = j < len ? fabsf(src[j]) : 0.f, buf[1][j] = 0.f;
    }
    __syncthreads();
    int cur = 0;
    for (int o = 1; 2 * o <= window; o *= 2) {                       // m_k from m_{k-1}, o = 2^(k-1); entries from len - 2 o + 1 on are not used
        const float* m = buf[cur];
        float* d = buf[cur ^ 1];
        const int valid4 = (len - 2 * o + 1 + 3) & ~3;
        for (int i = 4 * tid; i < valid4; i += 4 * 256) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(m + i);
            f32x4 b;
            if (o >= 4) {
                b = *reinterpret_cast<const f32x4*>(m + i + o);
            } else {                                                 // o = 1, 2: the shifted vector straddles two aligned ones
                const f32x4 c = *reinterpret_cast<const f32x4*>(m + i + 4);
                b = o == 1 ? f32x4{a[1], a[2], a[3], c[0]} : f32x4{a[2], a[3], c[0], c[1]};
            }
            f32x4 r;
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = fmaxf(a[e], b[e]);
            *reinterpret_cast<f32x4*>(d + i) = r;
        }
        __syncthreads();
        cur ^= 1;
    }
    const float* m = buf[cur];
    const int second = window - (1 << (31 - __clz(window)));         // window - 2^p
    const int cnt = (int)min((long)TILE, n - t0);
    for (int i = tid; i < cnt; i += 256) {
        const long g = t0 + i;
        const int l = (int)(min(g, last) - s0);
        const float onset = (g < n_frames && onset_mask && onset_mask[g]) ? 1.f : 0.f;
        out[g] = make_float2(fmaxf(m[l], m[l + second]), onset);
    }
}

}  // namespace

extern "C" int mc_audio_condition(const float* wave_dev, int64_t n_samples, int32_t window, const uint8_t* onset_mask_dev, int32_t n_frames,
                                  float* out_dev, void* stream) {
    MC_REQUIRE(wave_dev && out_dev, "audio condition: null argument");
    MC_REQUIRE(window >= 1 && window <= MAX_WINDOW, "audio condition: window=%d (1..%d)", window, MAX_WINDOW);
    MC_REQUIRE(n_samples >= window, "audio condition: %ld samples hold no full window of %d", (long)n_samples, window);
    MC_REQUIRE(n_frames >= 0 && n_frames <= n_samples, "audio condition: %d onset frames index into %ld samples", n_frames, (long)n_samples);
    MC_REQUIRE(((uintptr_t)wave_dev & 3) == 0 && ((uintptr_t)out_dev & 7) == 0, "audio condition: wave must be 4-byte and out 8-byte aligned");
    const int64_t tiles = (n_samples + TILE - 1) / TILE;
    MC_REQUIRE(tiles <= 0x7fffffff, "audio condition: %ld samples are more than one launch takes", (long)n_samples);
    hipLaunchKernelGGL(audio_condition_k, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, wave_dev, (long)n_samples, window, onset_mask_dev,
                       n_frames, (float2*)out_dev);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
