// Result post-processing of the 322-d SMPL-X motion vector, on the device:
//   de-normalise (pred * std + mean)                                    tools/visualize.py:217-220
//   re-pack 322 -> poses[165] (body 0:66, jaw 66:69 <- 156:159, hands 75:165 <- 66:156),
//                  expressions[100] <- 209:309, trans[3] <- 309:312        tools/visualize.py:236-243, s2g_test.py:289-297
//   Gaussian temporal filter per channel, scipy.ndimage.gaussian_filter(mode="nearest") semantics
//   (taps = normalised exp(-x^2 / 2 sigma^2), radius int(4 sigma + .5), edge frames replicated)
//                                                                       tools/visualize.py:39-44,244-246
// One thread per (sample, frame, output channel); the whole [T,322] slab of a sample is a few hundred KB and
// stays in L2, so the 2r+1 strided taps are cache hits: HBM traffic = one read of pred + one write of the outputs.
#include "mc_common.h"
#include "mc_kernels.h"

namespace {

constexpr int NPOSE = 165, NEXPR = 100, NTRANS = 3, NOUT = NPOSE + NEXPR + NTRANS;

struct PostArgs {
    const float* pred;        // [B][T][322] normalised
    const int* lengths;       // [B] valid frames (filter support is clamped to [0, len))
    const int* rows;          // stitched mode (B == 1, T == stitched frames): frame t reads row rows[t] of pred [*, 322]
    const double* mean;       // [322]
    const double* stdv;       // [322]
    const double* taps;       // 4 tables of MAXTAP doubles: centre at [radius[g]]
    int radius[4];            // per group: body+jaw, hands, trans, expr;  -1 = not filtered
    int stats_f32;            // de-normalise in fp32 (two roundings, numpy float32 * float32 + float32)
    int B, T, C;
    double* poses;            // [B][T][165]
    double* expr;             // [B][T][100]
    double* trans;            // [B][T][3]
};

constexpr int MAXTAP = 129;

// numpy evaluates pred * std + mean as two ufunc passes (two roundings): keep the compiler from fusing them into
// one FMA (hipcc contracts by default, and HIP's __fmul_rn / __fadd_rn are plain operators).
template <typename F>
__device__ __forceinline__ F mul_then_add(F p, F s, F m) {
#pragma clang fp contract(off)
    const F q = p * s;
    return q + m;
}

__global__ __launch_bounds__(256) void smplx_post_k(PostArgs a) {
    const long total = (long)a.B * a.T * NOUT;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int j = (int)(i % NOUT);
        const int t = (int)((i / NOUT) % a.T);
        const int b = (int)(i / ((long)NOUT * a.T));
        int src, grp;
        double* out;
        if (j < NPOSE) {
            out = a.poses + ((long)b * a.T + t) * NPOSE + j;
            if (j < 66) { src = j; grp = 0; }
            else if (j < 69) { src = 156 + (j - 66); grp = 0; }
            else if (j < 75) { src = -1; grp = 0; }                       // eye poses: not generated
            else { src = 66 + (j - 75); grp = 1; }
        } else if (j < NPOSE + NEXPR) {
            out = a.expr + ((long)b * a.T + t) * NEXPR + (j - NPOSE);
            src = 209 + (j - NPOSE); grp = 3;
        } else {
            out = a.trans + ((long)b * a.T + t) * NTRANS + (j - NPOSE - NEXPR);
            src = 309 + (j - NPOSE - NEXPR); grp = 2;
        }
        const int len = a.lengths ? a.lengths[b] : a.T;
        if (src < 0 || t >= len) { *out = 0.0; continue; }
        const float* col = a.pred + (long)b * a.T * a.C + src;      // (stitched mode: B == 1 -> b == 0)
        const double m = a.mean[src], s = a.stdv[src];
        const float mf = (float)m, sf = (float)s;
        auto denorm = [&](int tt) -> double {
            const float p = col[(long)(a.rows ? a.rows[tt] : tt) * a.C];
            if (a.stats_f32) return (double)mul_then_add<float>(p, sf, mf);
            return mul_then_add<double>((double)p, s, m);
        };
        const int r = a.radius[grp];
        if (r < 0) { *out = denorm(t); continue; }
        const double* w = a.taps + grp * MAXTAP;
        double acc = denorm(t) * w[r];
        for (int k = 1; k <= r; ++k) {
            const int lo = t - k < 0 ? 0 : t - k, hi = t + k > len - 1 ? len - 1 : t + k;
            acc += (denorm(lo) + denorm(hi)) * w[r + k];
        }
        *out = acc;
    }
}

// ---- HumanML3D / KIT features -> joint positions (recover_from_ric + the tool's temporal filter) ------------------
//   data = float(pred * std + mean)                                     tools/visualize.py:47,220
//   ang[t] = sum_{s<t} data[s,0];  q[t] = (cos ang, 0, sin ang, 0)       mogen/utils/plot_utils.py:69-78
//   r_pos[t].xz = sum_{s<=t} qrot(qinv(q[s]), (data[s-1,1], 0, data[s-1,2]));  r_pos[t].y = data[t,3]     :80-88
//   joint j >= 1: qrot(qinv(q[t]), data[t, 4+3(j-1) : 4+3j]) + r_pos[t].xz;  joint 0 = r_pos[t]            :91-104
//   every (joint, axis) track filtered over time like the SMPL-X channels tools/visualize.py:31-37,48
// Two phases.  The scan phase is one 256-thread workgroup per sequence: it walks the frames in chunks of 256 and
// leaves the per-frame root state (cos, sin, x, z) in LDS (one sample) or in a workspace (the stitched sequence, any
// length).  The filter phase is one thread per (frame, joint): it re-derives the unfiltered joint of each tap from
// pred (L2 hits) and the root state, so no [n, 3J] intermediate is stored.  After the fp32 rounding of `data`
// everything is fp64 with one rounding at the store: the result does not depend on the scan order.
constexpr int T2M_MAXT = 1024;                 // frames of one sample whose root state is held in LDS (32 KB)

struct JointArgs {
    const float* pred;        // [B][T][C] normalised
    const int* lengths;       // [B] or null (= T)
    const int* rows;          // stitched: frame t reads row rows[t] of pred [*, C]
    const double* mean;       // [C]
    const double* stdv;       // [C]
    const double* taps;       // MAXTAP doubles, centre at [radius]
    int radius;               // -1 = not filtered
    int stats_f32;
    int B, T, C, J;
    double* root;             // stitched: workspace [T][4]
    float* out;               // [B][T][J][3]
};

// one sequence of `n` frames as the phases see it
struct JointSeq {
    const float* pred;        // row 0 of the sequence
    const int* rows;
    int n, C, stats_f32;
    const double* mean;
    const double* stdv;
    __device__ __forceinline__ double at(int t, int ch) const {           // data[t, ch], rounded to fp32 like the tool does
        const float p = pred[(long)(rows ? rows[t] : t) * C + ch];
        const double m = mean[ch], s = stdv[ch];
        if (stats_f32) return (double)mul_then_add<float>(p, (float)s, (float)m);
        return (double)(float)mul_then_add<double>((double)p, s, m);
    }
};

// inclusive prefix sum over the 256 threads of the workgroup; `total` = the sum of all 256
__device__ __forceinline__ double block_scan_256(double v, double* buf, double& total) {
    const int i = threadIdx.x;
    buf[i] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const double add = i >= d ? buf[i - d] : 0.0;
        __syncthreads();
        v += add;
        buf[i] = v;
        __syncthreads();
    }
    total = buf[255];
    __syncthreads();
    return v;
}

// rotation of (x, ., z) by the conjugate of q = (c, 0, s, 0):  v + 2 (c (u x v) + u x (u x v)),  u = (0, -s, 0)
__device__ __forceinline__ void yaw_rotate(double c, double s, double x, double z, double& ox, double& oz) {
    const double k = 1.0 - 2.0 * s * s, m = 2.0 * c * s;
    ox = k * x - m * z;
    oz = k * z + m * x;
}

// scan phase: root[t] = (cos ang[t], sin ang[t], r_pos[t].x, r_pos[t].z) for t < n; the whole workgroup calls it
__device__ void t2m_root_scan(const JointSeq& q, double* root, double* buf) {
    double c_ang = 0.0, c_x = 0.0, c_z = 0.0, tot;
    for (int base = 0; base < q.n; base += 256) {
        const int t = base + (int)threadIdx.x;
        const bool prev = t >= 1 && t < q.n;                              // frame t adds the velocities of frame t - 1
        const double ang = c_ang + block_scan_256(prev ? q.at(t - 1, 0) : 0.0, buf, tot);
        c_ang += tot;
        double sn, cs, vx = 0.0, vz = 0.0;
        sincos(ang, &sn, &cs);
        if (prev) yaw_rotate(cs, sn, q.at(t - 1, 1), q.at(t - 1, 2), vx, vz);
        const double x = c_x + block_scan_256(vx, buf, tot);
        c_x += tot;
        const double z = c_z + block_scan_256(vz, buf, tot);
        c_z += tot;
        if (t < q.n) {
            root[4 * t + 0] = cs; root[4 * t + 1] = sn; root[4 * t + 2] = x; root[4 * t + 3] = z;
        }
    }
}

// filter phase, one (frame t, joint j): the three filtered coordinates
__device__ __forceinline__ void t2m_filtered_joint(const JointSeq& q, const double* root, const double* taps, int r,
                                                   int t, int j, float* out3) {
    auto joint = [&](int tt, double& x, double& y, double& z) {
        const double* rt = root + 4 * tt;
        if (j == 0) { x = rt[2]; y = q.at(tt, 3); z = rt[3]; return; }
        const int ch = 4 + 3 * (j - 1);
        yaw_rotate(rt[0], rt[1], q.at(tt, ch), q.at(tt, ch + 2), x, z);
        x += rt[2]; y = q.at(tt, ch + 1); z += rt[3];
    };
    double x, y, z;
    joint(t, x, y, z);
    if (r >= 0) {
        x *= taps[r]; y *= taps[r]; z *= taps[r];
        for (int k = 1; k <= r; ++k) {
            const int lo = t - k < 0 ? 0 : t - k, hi = t + k > q.n - 1 ? q.n - 1 : t + k;
            double xa, ya, za, xb, yb, zb;
            joint(lo, xa, ya, za);
            joint(hi, xb, yb, zb);
            const double w = taps[r + k];
            x += (xa + xb) * w; y += (ya + yb) * w; z += (za + zb) * w;
        }
    }
    out3[0] = (float)x; out3[1] = (float)y; out3[2] = (float)z;
}

// per sample: workgroup (b, slice) scans sample b into LDS, then filters every gridDim.y-th group of 256 (frame, joint) pairs
__global__ __launch_bounds__(256) void t2m_joints_k(JointArgs a) {
    __shared__ double root[4 * T2M_MAXT];
    __shared__ double buf[256];
    const int b = blockIdx.x;
    int len = a.lengths ? a.lengths[b] : a.T;
    len = len < 0 ? 0 : (len > a.T ? a.T : len);
    const JointSeq q{a.pred + (long)b * a.T * a.C, nullptr, len, a.C, a.stats_f32, a.mean, a.stdv};
    t2m_root_scan(q, root, buf);
    __syncthreads();
    float* out = a.out + (long)b * a.T * a.J * 3;
    for (int i = blockIdx.y * 256 + threadIdx.x; i < a.T * a.J; i += gridDim.y * 256) {
        const int t = i / a.J, j = i % a.J;
        if (t < len) t2m_filtered_joint(q, root, a.taps, a.radius, t, j, out + 3L * i);
        else out[3L * i] = out[3L * i + 1] = out[3L * i + 2] = 0.f;
    }
}

// stitched sequence (a.T frames through a.rows): root state to the workspace, one workgroup ...
__global__ __launch_bounds__(256) void t2m_root_scan_k(JointArgs a) {
    __shared__ double buf[256];
    const JointSeq q{a.pred, a.rows, a.T, a.C, a.stats_f32, a.mean, a.stdv};
    t2m_root_scan(q, a.root, buf);
}

// ... then the filter over all (frame, joint) pairs
__global__ __launch_bounds__(256) void t2m_joints_filter_k(JointArgs a) {
    const JointSeq q{a.pred, a.rows, a.T, a.C, a.stats_f32, a.mean, a.stdv};
    const long total = (long)a.T * a.J;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256)
        t2m_filtered_joint(q, a.root, a.taps, a.radius, (int)(i / a.J), (int)(i % a.J), a.out + 3 * i);
}

}  // namespace

int mc_launch_t2m_joints(const float* pred, const int* lengths, const int* rows, const double* mean, const double* stdv,
                         const double* taps, int radius, int stats_f32, int B, int T, int C, int J, double* root_work,
                         float* joints, hipStream_t s) {
    MC_REQUIRE(J >= 2, "joint recovery: joints_num=%d (at least the root and one joint)", J);
    MC_REQUIRE(C == 4 + 9 * (J - 1) + 3 * J + 4, "joint recovery: input_feats=%d is not the %d-joint layout (4 + 9 (J-1) + 3 J + 4 = %d)",
               C, J, 4 + 9 * (J - 1) + 3 * J + 4);
    MC_REQUIRE(radius < (MAXTAP + 1) / 2, "joint recovery: filter radius %d too large", radius);
    MC_REQUIRE(B >= 0 && T >= 0, "joint recovery: negative size");
    JointArgs a;
    a.pred = pred; a.lengths = lengths; a.rows = rows; a.mean = mean; a.stdv = stdv; a.taps = taps;
    a.radius = radius < 0 ? -1 : radius; a.stats_f32 = stats_f32; a.B = B; a.T = T; a.C = C; a.J = J;
    a.root = root_work; a.out = joints;
    if ((long)B * T == 0) return MC_OK;
    if (rows) {
        MC_REQUIRE(B == 1 && !lengths && root_work, "joint recovery: the stitched mode takes one sequence of `T` mapped frames and a workspace");
        hipLaunchKernelGGL(t2m_root_scan_k, dim3(1), dim3(256), 0, s, a);
        MC_LAUNCH_CHECK();
        int blocks = cdiv((long)T * J, 256);
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(t2m_joints_filter_k, dim3(blocks), dim3(256), 0, s, a);
    } else {
        MC_REQUIRE(T <= T2M_MAXT, "joint recovery: T=%d frames per sample (at most %d; longer sequences go through the stitched form)", T, T2M_MAXT);
        int slices = cdiv((long)T * J, 1024);                           // ~4 (frame, joint) pairs per thread
        if (slices > 16) slices = 16;
        hipLaunchKernelGGL(t2m_joints_k, dim3(B, slices), dim3(256), 0, s, a);
    }
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int mc_launch_smplx_post(const float* pred, const int* lengths, const int* rows, const double* mean, const double* stdv,
                         const double* taps, const int* radius, int stats_f32, int B, int T, int C,
                         double* poses, double* expr, double* trans, hipStream_t s) {
    MC_REQUIRE(C == 322, "smplx post-processing: input_feats=%d (the SMPL-X layout is 322-d)", C);
    MC_REQUIRE(!rows || (B == 1 && !lengths), "smplx post-processing: the stitched mode takes one sequence of `T` mapped frames");
    PostArgs a;
    a.pred = pred; a.lengths = lengths; a.rows = rows; a.mean = mean; a.stdv = stdv; a.taps = taps;
    for (int g = 0; g < 4; ++g) {
        MC_REQUIRE(radius[g] < (MAXTAP + 1) / 2, "smplx post-processing: filter radius %d too large", radius[g]);
        a.radius[g] = radius[g];
    }
    a.stats_f32 = stats_f32; a.B = B; a.T = T; a.C = C;
    a.poses = poses; a.expr = expr; a.trans = trans;
    const long total = (long)B * T * NOUT;
    if (total <= 0) return MC_OK;
    int blocks = cdiv(total, 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(smplx_post_k, dim3(blocks), dim3(256), 0, s, a);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int mc_smplx_post_maxtap() { return MAXTAP; }
