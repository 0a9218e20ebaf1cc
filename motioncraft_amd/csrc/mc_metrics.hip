// Beat alignment of the speech-to-gesture test on the device: alignment.load_pose + alignment.calculate_align of the reference's
// mogen/datasets/EMAGE_2024/utils/metric.py:78-127,199-242, fed the 55 joints of mc_smplx_joints (tools/s2g_test.py:406,418-422).
//   speed[f][j] = |d joints[f][j] / dt| / mean_vel[j]: forward / central / backward differences, fp32 like numpy on fp32 joints
//                 (dt = 1 / pose_fps rounded to fp32, sqrt((x x + y y) + z z) without fused multiply-adds), then the division
//                 by mean_vel in its own precision;
//   beat mask     slice s = speed[t_start:t_end][j]: i is a beat iff s[i] < s[clip(i +- k, 0, n - 1)] for k = 1..order
//                 (scipy's argrelextrema(np.less, mode='clip')) and speed[i][j] > threshold -- i is slice-relative but looked up
//                 in the UNSLICED array, as metric.py:113-123 does;
//   score         mean over the upper-body joints of mean over onsets of exp(-d^2 / (2 sigma^2)), d = distance from the onset
//                 to the joint's nearest beat time i / pose_fps (0 for a joint without beats).
// beat_mask_k: one workgroup per (tile of TF slice frames, joint); the tile's speeds with a halo of `order` frames on each side sit
// in LDS (clipped at the fill, so the comparison loop reads straight).  align_k: one workgroup per upper-body joint compacts the
// joint's beats in order (wave ballots + an LDS prefix over the four waves), runs one binary search per onset over the sorted beat
// list and reduces the terms in a fixed order (wave shuffles, then the four waves): no floating-point atomics, so two runs give the same bits.
#include "mc_common.h"
#include "../../include/motioncraft_amd.h"
#include <math.h>

namespace {

constexpr int TF = 256;                      // slice frames per workgroup of beat_mask_k
constexpr int MAX_ORDER = MC_BEAT_MAX_ORDER, MAX_UPPER = MC_BEAT_MAX_UPPER;

struct SpeedArgs {
    const float* joints;                     // [T, nj, 3]
    const double* mean_vel;                  // [nj]
    int T, nj, mv_f32;
    float dt, dt2;                           // 1 / pose_fps and 2 / pose_fps, rounded to fp32
};

// speed of joint j at frame f of the whole sequence (T >= 2); the fp32 value widened when mean_vel is fp32
__device__ __forceinline__ double speed_at(const SpeedArgs& a, int f, int j) {
#pragma clang fp contract(off)
    const bool edge = f == 0 || f == a.T - 1;
    const float* hi = a.joints + ((long)min(f + 1, a.T - 1) * a.nj + j) * 3;
    const float* lo = a.joints + ((long)max(f - 1, 0) * a.nj + j) * 3;
    const float d = edge ? a.dt : a.dt2;
    const float vx = (hi[0] - lo[0]) / d, vy = (hi[1] - lo[1]) / d, vz = (hi[2] - lo[2]) / d;
    const float s = sqrtf((vx * vx + vy * vy) + vz * vz);
    return a.mv_f32 ? (double)(s / (float)a.mean_vel[j]) : (double)s / a.mean_vel[j];
}

__global__ __launch_bounds__(256) void beat_mask_k(SpeedArgs a, int t_start, int n, int order, double threshold, uint8_t* __restrict__ mask) {
    __shared__ double s[TF + 2 * MAX_ORDER];
    const int tid = threadIdx.x, j = blockIdx.y, i0 = blockIdx.x * TF;
    for (int e = tid; e < TF + 2 * order; e += 256) s[e] = speed_at(a, t_start + min(max(i0 - order + e, 0), n - 1), j);
    __syncthreads();
    const int i = i0 + tid;
    if (i >= n) return;
    const double c = s[order + tid];
    bool beat = true;
    for (int k = 1; k <= order; ++k) beat = beat && c < s[order + tid - k] && c < s[order + tid + k];
    mask[(long)j * n + i] = beat && speed_at(a, i, j) > threshold;
}

struct UpperBody { int joint[MAX_UPPER]; };

__global__ __launch_bounds__(256) void align_k(const uint8_t* __restrict__ mask, int n, UpperBody ub, const double* __restrict__ onsets, int n_on,
                                               double pose_fps, double two_sigma2, int* __restrict__ beats, double* __restrict__ per_joint) {
    __shared__ int wave_cnt[4];
    __shared__ double sh[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint8_t* m = mask + (long)ub.joint[blockIdx.x] * n;
    int* bt = beats + (long)blockIdx.x * n;
    int nb = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        const bool b = i < n && m[i] != 0;
        const unsigned long long bal = __ballot(b);
        if (lane == 0) wave_cnt[w] = __popcll(bal);
        __syncthreads();
        int off = nb;
        for (int q = 0; q < w; ++q) off += wave_cnt[q];
        if (b) bt[off + __popcll(bal & ((1ull << lane) - 1ull))] = i;
        nb += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        __syncthreads();
    }
    double acc = 0.0;
    if (nb > 0)
        for (int o = tid; o < n_on; o += 256) {
            const double t = onsets[o];
            int lo = 0, hi = nb;                     // first beat at or after the onset
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if ((double)bt[mid] / pose_fps < t) lo = mid + 1; else hi = mid;
            }
            double d = INFINITY;
            if (lo < nb) d = fabs((double)bt[lo] / pose_fps - t);
            if (lo > 0) d = fmin(d, fabs((double)bt[lo - 1] / pose_fps - t));
            acc += exp(-(d * d) / two_sigma2);
        }
    acc = block_sum_f64(acc, sh);
    if (tid == 0) per_joint[blockIdx.x] = acc / (double)n_on;
}

__global__ __launch_bounds__(64) void align_mean_k(const double* __restrict__ per_joint, int nu, double* __restrict__ score) {
    double v = 0.0;
    for (int i = threadIdx.x; i < nu; i += 64) v += per_joint[i];
    v = wave_sum_f64(v);
    if (threadIdx.x == 0) *score = v / (double)nu;
}

}  // namespace

extern "C" {

int mc_beat_mask(const float* joints_dev, int32_t n_frames, int32_t num_joints, const double* mean_vel_dev, int32_t mean_vel_fp32,
                 int32_t t_start, int32_t t_end, double pose_fps, int32_t order, double threshold, uint8_t* mask_out_dev, void* stream) {
    MC_REQUIRE(joints_dev && mean_vel_dev && mask_out_dev, "beat mask: null argument");
    MC_REQUIRE(n_frames >= 2 && num_joints >= 1 && num_joints <= 65535, "beat mask: %d frames of %d joints (at least 2 frames, 1..65535 joints)",
               n_frames, num_joints);
    MC_REQUIRE(0 <= t_start && t_start < t_end && t_end <= n_frames, "beat mask: the slice [%d, %d) is empty or leaves the %d frames", t_start, t_end,
               n_frames);
    MC_REQUIRE(order >= 1 && order <= MAX_ORDER && pose_fps > 0.0, "beat mask: order=%d (1..%d), pose_fps=%g (> 0)", order, MAX_ORDER, pose_fps);
    SpeedArgs a;
    a.joints = joints_dev; a.mean_vel = mean_vel_dev; a.T = n_frames; a.nj = num_joints; a.mv_f32 = mean_vel_fp32 != 0;
    const double dt = 1.0 / pose_fps;
    a.dt = (float)dt; a.dt2 = (float)(2 * dt);
    const int n = t_end - t_start;
    // an fp32 speed is compared with the threshold rounded to fp32 (numpy keeps the Python scalar weak); widening both is exact
    const double thr = a.mv_f32 ? (double)(float)threshold : threshold;
    hipLaunchKernelGGL(beat_mask_k, dim3(cdiv(n, TF), num_joints), dim3(256), 0, (hipStream_t)stream, a, t_start, n, order, thr, mask_out_dev);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int64_t mc_beat_align_work_bytes(int32_t n_slice, int32_t n_upper) {
    if (n_slice < 1 || n_upper < 1 || n_upper > MAX_UPPER) return -1;
    return (int64_t)n_upper * (sizeof(double) + (int64_t)n_slice * sizeof(int));
}

int mc_beat_align(const uint8_t* mask_dev, int32_t num_joints, int32_t n_slice, const int32_t* upper_body_host, int32_t n_upper,
                  const double* onsets_dev, int32_t n_onsets, double pose_fps, double sigma, void* work_dev, int64_t work_bytes,
                  double* score_out_dev, void* stream) {
    MC_REQUIRE(mask_dev && upper_body_host && onsets_dev && work_dev && score_out_dev, "beat alignment: null argument");
    MC_REQUIRE(num_joints >= 1 && n_slice >= 1 && n_upper >= 1 && n_upper <= MAX_UPPER, "beat alignment: %d joints, %d frames, %d upper-body joints (1..%d)",
               num_joints, n_slice, n_upper, MAX_UPPER);
    MC_REQUIRE(n_onsets >= 1, "beat alignment: no onsets (the score is a mean over them)");
    MC_REQUIRE(pose_fps > 0.0 && sigma > 0.0, "beat alignment: pose_fps=%g, sigma=%g (both > 0)", pose_fps, sigma);
    MC_REQUIRE(((uintptr_t)work_dev & 7) == 0 && work_bytes >= mc_beat_align_work_bytes(n_slice, n_upper),
               "beat alignment: the workspace must be 8-byte aligned and hold %ld bytes (mc_beat_align_work_bytes), got %ld",
               (long)mc_beat_align_work_bytes(n_slice, n_upper), (long)work_bytes);
    UpperBody ub;
    for (int i = 0; i < n_upper; ++i) {
        MC_REQUIRE(upper_body_host[i] >= 0 && upper_body_host[i] < num_joints, "beat alignment: upper-body joint %d is not one of the %d joints",
                   upper_body_host[i], num_joints);
        ub.joint[i] = upper_body_host[i];
    }
    for (int i = n_upper; i < MAX_UPPER; ++i) ub.joint[i] = 0;
    double* per_joint = (double*)work_dev;
    int* beats = (int*)(per_joint + n_upper);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(align_k, dim3(n_upper), dim3(256), 0, s, mask_dev, n_slice, ub, onsets_dev, n_onsets, pose_fps, 2 * (sigma * sigma), beats, per_joint);
    MC_LAUNCH_CHECK();
    hipLaunchKernelGGL(align_mean_k, dim3(1), dim3(64), 0, s, per_joint, n_upper, score_out_dev);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

}  // extern "C"
