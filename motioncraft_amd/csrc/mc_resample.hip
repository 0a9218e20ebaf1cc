// From the bytes of a PCM wav file to the waveform the S2G front reads, on the device: decode + mono mix (mc_pcm_decode) and rational
// resampling (mc_resample_poly).  The reference does this on the host with librosa.load + librosa.resample
// (mogen/datasets/EMAGE_2024/dataloaders/beat_sep_lower.py:392-393, tools/s2g_test.py:416-417); the resampler here is librosa's
// res_type='polyphase', i.e. scipy.signal.resample_poly with zero padding, NOT its default soxr_hq.  The semantics are stated once, in
// numpy, in tests/resample_ref.py:
//   y[m] = fp32( sum over k of x[k] * taps[half + m*down - k*up] ),  0 <= k < n_in,  0 <= half + m*down - k*up < n_taps
// with taps the filter already multiplied by `up`, half = (n_taps - 1) / 2.  Writing q = half + m*down = qd*up + p, output m reads
// only the taps of its phase p: taps[p + j*up], j = qd - k.  The host lays the filter out phase-major and reversed,
//   table[p][i] = taps[p + (L - 1 - i)*up] (0 past the filter's end),  L = ceil(n_taps / up),
// so that a thread walks its inputs in ascending k and its taps in ascending i, both contiguous.
// A workgroup produces TILE consecutive outputs, one thread per output and pass.  The inputs any of them reads are one contiguous
// span of at most (TILE - 1)*down/up + n_taps/up + 2 samples: it is staged in LDS once (32-bit reads: no alignment is asked of x) and
// each sample is then read by about n_taps/down threads.  The taps are read through global memory: the table (70 KB for 441/320,
// 102 KB for 640/441) stays in L2.  Staging them in LDS would be warranted if a chain took longer than the upload of the clip it
// processes; measured (tools/resample_time.py, profiles/resample_time.txt, DESIGN.md: 60 s of 44.1 kHz stereo) decode + resample
// take 84 us and the detour through 22 050 Hz 113 us against 270 us for the copy of the same bytes, so they are not staged.  Products and the sum are fp64 (fma), in ascending k whatever the tiling, rounded to fp32
// once; no atomics, no workspace, one launch: two runs give the same bits.  Every sample index is 64-bit.
#include "mc_common.h"
#include "../../include/motioncraft_amd.h"

namespace {

constexpr int TILE = MC_RESAMPLE_TILE;       // outputs per workgroup
constexpr long MAX_SPAN_BYTES = 64 << 10;    // the dynamic LDS a launch gets without asking for more

__global__ __launch_bounds__(256) void resample_poly_k(const float* __restrict__ x, long n_in, long up, long down, const double* __restrict__ table,
                                                       long n_taps, long L, float* __restrict__ y, long n_out) {
    extern __shared__ __attribute__((aligned(16))) float xs[];       // xs[j] = x[ks0 + j]
    const int tid = threadIdx.x;
    const long half = (n_taps - 1) / 2;
    const long m0 = (long)blockIdx.x * TILE;
    const long m1 = min(m0 + TILE, n_out) - 1;
    // the first input of output m0 and the last input of output m1: k*up >= q - (n_taps - 1) and k*up <= q
    const long first = m0 * down - half;
    const long ks0 = first <= 0 ? 0 : (first + up - 1) / up;
    const long ks1 = min(n_in - 1, (half + m1 * down) / up);
    for (long j = tid; j <= ks1 - ks0; j += 256) xs[j] = x[ks0 + j];
    __syncthreads();
    for (long m = m0 + tid; m <= m1; m += 256) {
        const long q = half + m * down;
        const long qd = q / up;
        const long p = q - qd * up;
        double acc = 0.0;
        if (p < n_taps) {                                            // a phase past a filter shorter than `up` has no taps
            const long jmax = (n_taps - 1 - p) / up;                 // taps[p + j*up] exists for j = qd - k in 0..jmax
            const long k_lo = max(0L, qd - jmax), k_hi = min(n_in - 1, qd);
            const long tb = p * L + (L - 1 - qd);                    // table[tb + k] = taps[p + (qd - k)*up], 0 <= qd - k <= jmax < L
            for (long k = k_lo; k <= k_hi; ++k) acc = fma((double)xs[k - ks0], table[tb + k], acc);
        }
        y[m] = (float)acc;
    }
}

__device__ __forceinline__ int32_t pcm_value(const uint8_t* p, int sample_bytes) {
    switch (sample_bytes) {
        case 1: return (int32_t)p[0] - 128;
        case 2: return (int16_t)(uint16_t)(p[0] | (p[1] << 8));
        case 3: return (int32_t)(((uint32_t)p[0] << 8) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 24)) >> 8;
        default: return (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
    }
}

__global__ __launch_bounds__(256) void pcm_decode_k(const uint8_t* __restrict__ pcm, long n_frames, int channels, int sample_bytes, int mono,
                                                    double scale, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_frames) return;
    const uint8_t* p = pcm + i * channels * sample_bytes;
    double v = (double)pcm_value(p, sample_bytes);
    if (mono) {
        for (int c = 1; c < channels; ++c) v += (double)pcm_value(p + c * sample_bytes, sample_bytes);   // integers below 2^53: exact
        v /= (double)channels;
    }
    out[i] = (float)(v * scale);                                     // scale is a power of two: the product is exact
}

long gcd_of(long a, long b) {
    while (b) {
        const long r = a % b;
        a = b, b = r;
    }
    return a;
}

}  // namespace

extern "C" int64_t mc_resample_out_len(int64_t n_in, int32_t up, int32_t down) {
    if (n_in < 0 || up < 1 || down < 1) return -1;
    const __int128 n = ((__int128)n_in * up + down - 1) / down;
    return n > (__int128)INT64_MAX / 2 / down ? -1 : (int64_t)n;      // n_out * down + half stays inside int64 in the kernel
}

extern "C" int mc_resample_poly(const float* x_dev, int64_t n_in, int32_t up, int32_t down, const double* taps_dev, int32_t n_taps, float* y_dev,
                                int64_t n_out, void* stream) {
    MC_REQUIRE(x_dev && taps_dev && y_dev, "resample: null argument");
    MC_REQUIRE(n_in >= 1 && up >= 1 && down >= 1, "resample: n_in=%ld up=%d down=%d (all >= 1)", (long)n_in, up, down);
    MC_REQUIRE(gcd_of(up, down) == 1, "resample: up=%d and down=%d share a factor; reduce the ratio first", up, down);
    MC_REQUIRE(n_taps >= 1 && n_taps % 2 == 1, "resample: n_taps=%d must be odd (a filter centred on a sample)", n_taps);
    const int64_t want = mc_resample_out_len(n_in, up, down);
    MC_REQUIRE(want >= 1 && n_out == want, "resample: n_out=%ld, but %ld samples at %d/%d give %ld", (long)n_out, (long)n_in, up, down, (long)want);
    MC_REQUIRE(((uintptr_t)x_dev & 3) == 0 && ((uintptr_t)y_dev & 3) == 0 && ((uintptr_t)taps_dev & 7) == 0,
               "resample: x and y must be 4-byte and taps 8-byte aligned");
    const long span = ((long)(TILE - 1) * down + n_taps - 1) / up + 2;
    MC_REQUIRE(span * 4 <= MAX_SPAN_BYTES, "resample: a tile of %d outputs at %d/%d with %d taps reads %ld inputs, more than the %ld the LDS stage holds; "
               "resample in two steps", TILE, up, down, n_taps, span, MAX_SPAN_BYTES / 4);
    const int64_t tiles = (n_out + TILE - 1) / TILE;
    MC_REQUIRE(tiles <= 0x7fffffff, "resample: %ld outputs are more than one launch takes", (long)n_out);
    const long L = ((long)n_taps + up - 1) / up;
    hipLaunchKernelGGL(resample_poly_k, dim3((unsigned)tiles), dim3(256), (size_t)(span * 4 + 15) / 16 * 16, (hipStream_t)stream, x_dev, (long)n_in,
                       (long)up, (long)down, taps_dev, (long)n_taps, L, y_dev, (long)n_out);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

extern "C" int mc_pcm_decode(const uint8_t* pcm_dev, int64_t n_frames, int32_t channels, int32_t sample_bytes, int32_t mono, float* out_dev,
                             void* stream) {
    MC_REQUIRE(pcm_dev && out_dev, "pcm decode: null argument");
    MC_REQUIRE(n_frames >= 1, "pcm decode: n_frames=%ld", (long)n_frames);
    MC_REQUIRE(channels >= 1 && channels <= 1024, "pcm decode: channels=%d (1..1024)", channels);
    MC_REQUIRE(sample_bytes >= 1 && sample_bytes <= 4, "pcm decode: %d-byte samples (1: unsigned, 2..4: signed little-endian)", sample_bytes);
    MC_REQUIRE(((uintptr_t)out_dev & 3) == 0, "pcm decode: out must be 4-byte aligned");
    const int64_t blocks = (n_frames + 255) / 256;
    MC_REQUIRE(blocks <= 0x7fffffff, "pcm decode: %ld frames are more than one launch takes", (long)n_frames);
    hipLaunchKernelGGL(pcm_decode_k, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, pcm_dev, (long)n_frames, channels, sample_bytes,
                       mono != 0, 1.0 / (double)(1ull << (8 * sample_bytes - 1)), out_dev);
    MC_LAUNCH_CHECK();
    return MC_OK;
}
