// SMPL-X body model on the device: linear blend skinning as published (Loper et al. 2015; Pavlakos et al. 2019), i.e. what
// the `smplx` package's lbs() computes for the 55 kinematic joints and the vertices.  The reference creates that model in
// tools/s2g_test.py:76-85 and tools/visualize.py:71-86 and runs it per frame in tools/s2g_test.py:364-404; its joints feed
// L1div and the beat alignment (:406, :414-422), its face vertices the l2 / lvel errors (:407-412), its mesh plot_t2m_smplx.
// Per frame, theta [55,3] in the order mc_postprocess_smplx emits (global 0:3, body 3:66, jaw 66:69, eyes 69:75, hands 75:165):
//   R_j      = I + sin(a) K + (1 - cos a) K^2,  a = |theta_j + 1e-8|,  K = skew(theta_j / a)        (the package's batch_rodrigues)
//   v_shaped = v_template + shapedirs [beta; psi]          J = J_regressor v_shaped
//   v_posed  = v_shaped + posedirs^T vec(R_1..54 - I)
//   G_0 = [R_0 | J_0],  G_j = G_parent [R_j | J_j - J_parent],  A_j = G_j [I | -J_j]
//   joints_j = G_j[:3,3] + transl          verts_v = (sum_j W[v,j] A_j) [v_posed_v; 1] + transl
// finalize folds the regressor into J0 = J_regressor v_template and Jdirs = J_regressor shapedirs (fp64), so the joints never
// touch a vertex: joints_k is one kernel, fp64 inside with one rounding at the fp32 store (four frames per workgroup, one wave
// per frame in the level-ordered tree walk, transforms in LDS).  The vertices are fp32 like the package: feat_k writes the rows
// [psi | vec(R - I) | beta], the blend shapes are one launch of the fp32 MFMA GEMM (mc_gemm.hip) against the K-contiguous
// weight [expr_dirs | posedirs | shapedirs] laid out at finalize, and skin_k blends the frame's 55 A_j (LDS) with the
// per-vertex nonzero skin weights (ELL, in registers across the frames of a workgroup) and stores through LDS in 16-byte pieces.
// mc_smplx_vertex_errors runs that vertex path for two pose sets chunk by chunk and keeps only the two sums behind the face l2 /
// lvel errors (tools/s2g_test.py:407-412): vert_err_k leaves one fp64 partial per frame and sum, vert_err_sum_k adds them in one
// fixed order over the frames, so the sums do not depend on the chunk size either.
#include "mc_common.h"
#include "mc_gemm.h"
#include "mc_options.h"
#include "mc_params.h"
#include "../../include/motioncraft_amd.h"
#include <algorithm>
#include <string>
#include <vector>

namespace {

constexpr int NJ = 55, NJ3 = NJ * 3, NPF = 9 * (NJ - 1);
constexpr int JA = NJ * 12 + 4;              // floats per frame of the skinning transforms: 55 x [R | t] rows, then transl + pad
constexpr int MAXC = 400;                    // betas + expression coefficients
constexpr int FPB = 4;                       // frames per workgroup of joints_k (one wave each)
constexpr int VT = 256, SKF = 8;             // skin_k: vertices per workgroup, frames per workgroup

// sin(a) K + (1 - cos a) K^2 = R - I (no cancellation), a = |theta + 1e-8|, K = skew(theta / a)
__device__ __forceinline__ void rodrigues_minus_i(double tx, double ty, double tz, double (&m)[9]) {
    const double ex = tx + 1e-8, ey = ty + 1e-8, ez = tz + 1e-8;
    const double a = sqrt(ex * ex + ey * ey + ez * ez);
    const double x = tx / a, y = ty / a, z = tz / a;
    double s, c;
    sincos(a, &s, &c);
    const double u = 1.0 - c;
    m[0] = -u * (y * y + z * z); m[1] = u * x * y - s * z;    m[2] = u * x * z + s * y;
    m[3] = u * x * y + s * z;    m[4] = -u * (x * x + z * z); m[5] = u * y * z - s * x;
    m[6] = u * x * z - s * y;    m[7] = u * y * z + s * x;    m[8] = -u * (x * x + y * y);
}

struct JointsArgs {
    const double *poses, *expr, *trans, *betas;       // [n,165], [n,ne] | null, [n,3] | null, [nb] | [n,nb]
    int betas_per_frame, n, nb, ne;
    const double *J0, *JdirsT;                        // [165], [nb + ne][165]
    const int *parents, *level;
    int nlevels;
    float *joints, *A;                                // [n,55,3] | null, [n,JA] | null
};

__global__ __launch_bounds__(256) void joints_k(JointsArgs a) {
    __shared__ double coef[FPB][MAXC];
    __shared__ double Jl[FPB][NJ3];
    __shared__ double G[FPB][NJ][12];
    const int tid = threadIdx.x, Kc = a.nb + a.ne;
    const long f0 = (long)blockIdx.x * FPB;
    for (int i = tid; i < FPB * Kc; i += 256) {
        const int w = i / Kc, k = i % Kc;
        const long fr = min(f0 + w, (long)a.n - 1);
        coef[w][k] = k < a.nb ? a.betas[(a.betas_per_frame ? fr * a.nb : 0) + k] : (a.expr ? a.expr[fr * a.ne + (k - a.nb)] : 0.0);
    }
    __syncthreads();
    if (tid < NJ3) {
        double acc[FPB];
#pragma unroll
        for (int w = 0; w < FPB; ++w) acc[w] = a.J0[tid];
        for (int k = 0; k < Kc; ++k) {
            const double d = a.JdirsT[(long)k * NJ3 + tid];
#pragma unroll
            for (int w = 0; w < FPB; ++w) acc[w] += d * coef[w][k];
        }
#pragma unroll
        for (int w = 0; w < FPB; ++w) Jl[w][tid] = acc[w];
    }
    __syncthreads();
    const int w = tid >> 6, j = min(tid & 63, NJ - 1);
    const bool own = (tid & 63) < NJ;
    const long f = f0 + w, fr = min(f, (long)a.n - 1);
    double R[9];
    rodrigues_minus_i(a.poses[fr * NJ3 + 3 * j], a.poses[fr * NJ3 + 3 * j + 1], a.poses[fr * NJ3 + 3 * j + 2], R);
    R[0] += 1.0; R[4] += 1.0; R[8] += 1.0;
    const int lv = a.level[j], p = j ? a.parents[j] : 0;
    const double jx = Jl[w][3 * j], jy = Jl[w][3 * j + 1], jz = Jl[w][3 * j + 2];
    for (int l = 0; l < a.nlevels; ++l) {
        if (own && lv == l) {
            double* g = G[w][j];
            if (l == 0) {
#pragma unroll
                for (int r = 0; r < 3; ++r) { g[4 * r] = R[3 * r]; g[4 * r + 1] = R[3 * r + 1]; g[4 * r + 2] = R[3 * r + 2]; }
                g[3] = jx; g[7] = jy; g[11] = jz;
            } else {
                const double* q = G[w][p];
                const double tx = jx - Jl[w][3 * p], ty = jy - Jl[w][3 * p + 1], tz = jz - Jl[w][3 * p + 2];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const double q0 = q[4 * r], q1 = q[4 * r + 1], q2 = q[4 * r + 2];
                    g[4 * r] = q0 * R[0] + q1 * R[3] + q2 * R[6];
                    g[4 * r + 1] = q0 * R[1] + q1 * R[4] + q2 * R[7];
                    g[4 * r + 2] = q0 * R[2] + q1 * R[5] + q2 * R[8];
                    g[4 * r + 3] = q0 * tx + q1 * ty + q2 * tz + q[4 * r + 3];
                }
            }
        }
        __syncthreads();
    }
    if (!own || f >= a.n) return;
    const double* g = G[w][j];
    double t[3] = {0.0, 0.0, 0.0};
    if (a.trans) { t[0] = a.trans[f * 3]; t[1] = a.trans[f * 3 + 1]; t[2] = a.trans[f * 3 + 2]; }
    if (a.joints) {
        float* o = a.joints + (f * NJ + j) * 3;
        o[0] = (float)(g[3] + t[0]); o[1] = (float)(g[7] + t[1]); o[2] = (float)(g[11] + t[2]);
    }
    if (a.A) {
        float* o = a.A + f * JA + j * 12;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            o[4 * r] = (float)g[4 * r]; o[4 * r + 1] = (float)g[4 * r + 1]; o[4 * r + 2] = (float)g[4 * r + 2];
            o[4 * r + 3] = (float)(g[4 * r + 3] - (g[4 * r] * jx + g[4 * r + 1] * jy + g[4 * r + 2] * jz));
        }
        if (j == 0) {
            float* e = a.A + f * JA + NJ * 12;
            e[0] = (float)t[0]; e[1] = (float)t[1]; e[2] = (float)t[2]; e[3] = 0.f;
        }
    }
}

// one workgroup per frame: feat[f] = [psi (ne) | vec(R_1..54 - I) (486) | 0 .. Kp | beta (nb, per-frame form only) | 0 .. ld]
__global__ __launch_bounds__(256) void feat_k(const double* __restrict__ poses, const double* __restrict__ expr,
                                              const double* __restrict__ betas, int ne, int nb, int Kp, int ld, float* __restrict__ feat) {
    const long f = blockIdx.x;
    const int tid = threadIdx.x;
    float* row = feat + f * ld;
    if (tid < NJ - 1) {
        double m[9];
        const double* th = poses + f * NJ3 + 3 * (tid + 1);
        rodrigues_minus_i(th[0], th[1], th[2], m);
#pragma unroll
        for (int e = 0; e < 9; ++e) row[ne + 9 * tid + e] = (float)m[e];
    }
    for (int k = tid; k < ld; k += 256) {
        if (k < ne) row[k] = expr ? (float)expr[f * ne + k] : 0.f;
        else if (k >= ne + NPF && k < Kp) row[k] = 0.f;
        else if (k >= Kp) row[k] = (betas && k - Kp < nb) ? (float)betas[f * nb + (k - Kp)] : 0.f;
    }
}

// per-call betas: bias[r] = v_template[r] + sum_k W[r][Kp + k] beta[k]
__global__ __launch_bounds__(256) void shape_bias_k(const float* __restrict__ vt, const float* __restrict__ W, long ldw, int Kp, int nb,
                                                    const double* __restrict__ betas, int rows, float* __restrict__ bias) {
    __shared__ float sb[MAXC];
    for (int k = threadIdx.x; k < nb; k += 256) sb[k] = (float)betas[k];
    __syncthreads();
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const float* w = W + (long)r * ldw + Kp;
    float acc = vt[r];
    for (int k = 0; k < nb; ++k) acc = fmaf(w[k], sb[k], acc);
    bias[r] = acc;
}

// verts[f][v] = (sum_k w_k A[j_k]) [vp[f][v]; 1] + transl for VT vertices x SKF frames per workgroup; ELL [nz][V] (padding: w = 0).
// NZ = 4 / 8 / 16: the vertex's ELL entries stay in registers across the frames; NZ = 0: any width `nz` (up to all 55 joints),
// entries re-read per frame (cache hits after the first)
template <int NZ>
__global__ __launch_bounds__(256) void skin_k(const float* __restrict__ vp, long ldv, const float* __restrict__ A, const int* __restrict__ ell_j,
                                              const float* __restrict__ ell_w, int nz, int V, int n, long f_base, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float sA[JA];
    __shared__ __attribute__((aligned(16))) float sv[3 * VT];
    const int tid = threadIdx.x, v0 = blockIdx.x * VT, nv = min(VT, V - v0), cnt = 3 * nv;
    const int v = v0 + min(tid, nv - 1);
    int jj[NZ > 0 ? NZ : 1];
    float ww[NZ > 0 ? NZ : 1];
#pragma unroll
    for (int k = 0; k < NZ; ++k) { jj[k] = ell_j[(long)k * V + v] * 12; ww[k] = ell_w[(long)k * V + v]; }
    for (int fi = 0; fi < SKF; ++fi) {
        const long f = (long)blockIdx.y * SKF + fi;
        if (f >= n) break;
        for (int i = tid; i < JA; i += 256) sA[i] = A[f * JA + i];
        for (int i = tid; i < 3 * VT; i += 256) sv[i] = vp[f * ldv + 3 * v0 + min(i, cnt - 1)];
        __syncthreads();
        const float x = sv[3 * tid], y = sv[3 * tid + 1], z = sv[3 * tid + 2];
        float T[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) T[e] = 0.f;
        auto blend = [&](int j12, float w) {
            const f32x4* a4 = reinterpret_cast<const f32x4*>(sA + j12);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const f32x4 q = a4[r];
                T[4 * r] = fmaf(w, q[0], T[4 * r]); T[4 * r + 1] = fmaf(w, q[1], T[4 * r + 1]);
                T[4 * r + 2] = fmaf(w, q[2], T[4 * r + 2]); T[4 * r + 3] = fmaf(w, q[3], T[4 * r + 3]);
            }
        };
        if constexpr (NZ > 0) {
#pragma unroll
            for (int k = 0; k < NZ; ++k) blend(jj[k], ww[k]);
        } else {
            for (int k = 0; k < nz; ++k) blend(ell_j[(long)k * V + v] * 12, ell_w[(long)k * V + v]);
        }
        const float ox = fmaf(T[0], x, fmaf(T[1], y, fmaf(T[2], z, T[3]))) + sA[NJ * 12];
        const float oy = fmaf(T[4], x, fmaf(T[5], y, fmaf(T[6], z, T[7]))) + sA[NJ * 12 + 1];
        const float oz = fmaf(T[8], x, fmaf(T[9], y, fmaf(T[10], z, T[11]))) + sA[NJ * 12 + 2];
        __syncthreads();
        sv[3 * tid] = ox; sv[3 * tid + 1] = oy; sv[3 * tid + 2] = oz;
        __syncthreads();
        // the tile's cnt floats start at float offset g0 of `out` (16-byte aligned base; frame f of this launch is frame f_base + f of `out`): scalar head, 16-byte body, scalar tail
        const long g0 = ((f_base + f) * V + v0) * 3;
        const int head = min(cnt, (int)((4 - (g0 & 3)) & 3)), nvec = (cnt - head) >> 2, tail = cnt - head - 4 * nvec;
        if (tid < head) out[g0 + tid] = sv[tid];
        for (int i = tid; i < nvec; i += 256) {
            const float* s = sv + head + 4 * i;
            const f32x4 q = {s[0], s[1], s[2], s[3]};
            *reinterpret_cast<f32x4*>(out + g0 + head + 4 * i) = q;
        }
        if (tid < tail) out[g0 + head + 4 * nvec + tid] = sv[head + 4 * nvec + tid];
        __syncthreads();
    }
}

// face errors of tools/s2g_test.py:409-410, one workgroup per frame f of a chunk: l2[f] = sum (a - b)^2 and, from the second
// frame of the run on, lvel[f] = sum |(a[f] - b[f-1]) - (b[f] - b[f-1])|; fp32 element operations, fp64 sums in a fixed order.
// `vb` holds the previous frame's b in its row 0 (row f + 1 = frame f of the chunk); frame f of the chunk is frame f_base + f of the run
__global__ __launch_bounds__(256) void vert_err_k(const float* __restrict__ va, const float* __restrict__ vb, long E, long f_base,
                                                  double* __restrict__ l2, double* __restrict__ lvel) {
    __shared__ double sh[4];
    const long f = blockIdx.x;
    const float *a = va + f * E, *b = vb + (f + 1) * E, *bp = vb + f * E;
    const bool vel = f_base + f > 0;
    double s2 = 0.0, sv = 0.0;
    for (long i = threadIdx.x; i < E; i += 256) {
        const float x = a[i], y = b[i], d = x - y;
        s2 += (double)(d * d);
        if (vel) {
            const float p = bp[i];
            sv += (double)fabsf((x - p) - (y - p));
        }
    }
    s2 = block_sum_f64(s2, sh);
    sv = block_sum_f64(sv, sh);
    if (threadIdx.x == 0) { l2[f_base + f] = s2; lvel[f_base + f] = sv; }
}

// the per-frame partials in one fixed order over the frames: sums[0] = sum l2, sums[1] = sum lvel
__global__ __launch_bounds__(256) void vert_err_sum_k(const double* __restrict__ l2, const double* __restrict__ lvel, int n, double* __restrict__ sums) {
    __shared__ double sh[4];
    double s2 = 0.0, sv = 0.0;
    for (int f = threadIdx.x; f < n; f += 256) { s2 += l2[f]; sv += lvel[f]; }
    s2 = block_sum_f64(s2, sh);
    sv = block_sum_f64(sv, sh);
    if (threadIdx.x == 0) { sums[0] = s2; sums[1] = sv; }
}

int round_up(long a, int m) { return (int)((a + m - 1) / m * m); }

}  // namespace

struct mc_smplx {
    mc_smplx_config cfg;
    ParamStore params{"SMPL-X body model"};
    int V = 0, nb = 0, ne = 0, N4 = 0, Kp = 0, Kfull = 0, NZ = 0, nlevels = 0;
    const double *J0 = nullptr, *JdirsT = nullptr;
    const int *parents = nullptr, *level = nullptr, *ell_j = nullptr;
    const float *ell_w = nullptr, *W = nullptr, *vt4 = nullptr;
    bool finalized = false;
};

namespace {

template <typename T>
int upload_derived(ParamStore& ps, const std::vector<T>& host, const T** out) {
    float* d = nullptr;
    if (int r = ps.derived((host.size() * sizeof(T) + sizeof(float) - 1) / sizeof(float), &d)) return r;
    MC_HIP(hipMemcpy(d, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = reinterpret_cast<const T*>(d);
    return MC_OK;
}

int fetch(const ParamStore& ps, const char* name, int64_t numel, std::vector<float>& host) {
    const float* d = nullptr;
    if (int r = ps.get(name, numel, &d)) return r;
    host.resize((size_t)numel);
    MC_HIP(hipMemcpy(host.data(), d, (size_t)numel * sizeof(float), hipMemcpyDeviceToHost));
    return MC_OK;
}

int launch_joints(const mc_smplx* m, const double* poses, const double* expr, const double* trans, const double* betas, int per_frame, int n,
                  float* joints, float* A, hipStream_t s) {
    JointsArgs a;
    a.poses = poses; a.expr = expr; a.trans = trans; a.betas = betas; a.betas_per_frame = per_frame; a.n = n; a.nb = m->nb; a.ne = m->ne;
    a.J0 = m->J0; a.JdirsT = m->JdirsT; a.parents = m->parents; a.level = m->level; a.nlevels = m->nlevels; a.joints = joints; a.A = A;
    hipLaunchKernelGGL(joints_k, dim3(cdiv(n, FPB)), dim3(256), 0, s, a);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int check_frames(const mc_smplx* m, const void* poses, const void* betas, int n) {
    MC_REQUIRE(m && poses && betas && n >= 0, "SMPL-X body model: bad argument");
    MC_REQUIRE(m->finalized, "SMPL-X body model not finalized");
    return MC_OK;
}

long round_up4(long a) { return (a + 3) / 4 * 4; }

struct VertScratch { float *bias, *feat, *A, *vp; };                     // [N4] (per-call betas), [chunk,Kc], [chunk,JA], [chunk,N4]
struct FrameOperands { const double *poses, *expr, *trans, *betas; };   // a call's inputs from one frame on

FrameOperands frames_from(const mc_smplx* m, const double* poses, const double* expr, const double* trans, const double* betas, int per_frame, long c0) {
    return {poses + c0 * NJ3, expr ? expr + c0 * m->ne : nullptr, trans ? trans + c0 * 3 : nullptr, per_frame ? betas + c0 * m->nb : betas};
}

int launch_shape_bias(const mc_smplx* m, const double* betas, float* bias, hipStream_t s) {
    hipLaunchKernelGGL(shape_bias_k, dim3(cdiv(m->N4, 256)), dim3(256), 0, s, m->vt4, m->W, (long)m->Kfull, m->Kp, m->nb, betas, m->N4, bias);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

// the vertices of nc frames (one chunk: its scratch fits `w`) -> frames f_base .. f_base + nc of `verts_out` (16-byte aligned base)
int vertices_chunk(const mc_smplx* m, const McOptions* o, const FrameOperands& x, int per_frame, int nc, const VertScratch& w, float* joints_out,
                   float* verts_out, long f_base, hipStream_t s) {
    const int Kc = per_frame ? m->Kfull : m->Kp, N4 = m->N4, V = m->V;
    int r;
    if ((r = launch_joints(m, x.poses, x.expr, x.trans, x.betas, per_frame, nc, joints_out, w.A, s))) return r;
    hipLaunchKernelGGL(feat_k, dim3(nc), dim3(256), 0, s, x.poses, x.expr, per_frame ? x.betas : nullptr, m->ne, m->nb, m->Kp, Kc, w.feat);
    MC_LAUNCH_CHECK();
    GemmArgs g;                                  // v_posed = feat W^T + (v_template [+ shapedirs beta])
    g.A = w.feat; g.lda = Kc; g.W = m->W; g.ldw = m->Kfull; g.bias = per_frame ? m->vt4 : w.bias;
    g.C = w.vp; g.ldc = N4; g.M = nc; g.N = N4; g.K = Kc;
    // one kernel whatever the chunk's row count: a chunked call accumulates every element in the same order as an unchunked one
    g.tune = (int)o->gemm_tune & ~kTuneDma;
    if ((r = mc_launch_gemm(GM_PLAIN, g, 1, 0, s))) return r;
    const dim3 grid(cdiv(V, VT), cdiv(nc, SKF));
    if (m->NZ == 4) hipLaunchKernelGGL(skin_k<4>, grid, dim3(256), 0, s, w.vp, (long)N4, w.A, m->ell_j, m->ell_w, m->NZ, V, nc, f_base, verts_out);
    else if (m->NZ == 8) hipLaunchKernelGGL(skin_k<8>, grid, dim3(256), 0, s, w.vp, (long)N4, w.A, m->ell_j, m->ell_w, m->NZ, V, nc, f_base, verts_out);
    else if (m->NZ == 16) hipLaunchKernelGGL(skin_k<16>, grid, dim3(256), 0, s, w.vp, (long)N4, w.A, m->ell_j, m->ell_w, m->NZ, V, nc, f_base, verts_out);
    else hipLaunchKernelGGL(skin_k<0>, grid, dim3(256), 0, s, w.vp, (long)N4, w.A, m->ell_j, m->ell_w, m->NZ, V, nc, f_base, verts_out);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

}  // namespace

extern "C" {

int mc_smplx_create(const mc_smplx_config* cfg, mc_smplx** out) {
    MC_REQUIRE(cfg && out, "null argument");
    MC_REQUIRE(cfg->num_joints == NJ && cfg->num_pose_feats == NPF, "SMPL-X body model: %d joints / %d pose features (the model has %d / %d)",
               cfg->num_joints, cfg->num_pose_feats, NJ, NPF);
    MC_REQUIRE(cfg->num_vertices >= 1 && cfg->num_betas >= 1 && cfg->num_betas <= 300 && cfg->num_expr >= 1 && cfg->num_expr <= 100,
               "SMPL-X body model: num_vertices=%d num_betas=%d (1..300) num_expr=%d (1..100)", cfg->num_vertices, cfg->num_betas, cfg->num_expr);
    mc_smplx* m = new mc_smplx();
    m->cfg = *cfg;
    m->V = cfg->num_vertices; m->nb = cfg->num_betas; m->ne = cfg->num_expr;
    m->N4 = round_up(3L * m->V, 4);
    m->Kp = round_up(m->ne + NPF, 32);               // whole k-tiles of the GEMM in both forms
    m->Kfull = m->Kp + round_up(m->nb, 32);
    *out = m;
    return MC_OK;
}

void mc_smplx_destroy(mc_smplx* m) { delete m; }

int mc_smplx_set_param(mc_smplx* m, const char* name, const float* host, int64_t numel) {
    MC_REQUIRE(m && name && host && numel > 0, "bad argument");
    const int r = m->params.set(name, host, numel);
    if (r == MC_OK) m->finalized = false;
    return r;
}

int mc_smplx_finalize(mc_smplx* m) {
    MC_REQUIRE(m, "null body model");
    m->finalized = false;
    ParamStore& ps = m->params;
    ps.clear_derived();
    const int V = m->V, nb = m->nb, ne = m->ne;
    const long R3 = 3L * V;
    std::vector<float> vt, sd, ed, pd, jr, wt, par;
    int r;
    if ((r = fetch(ps, "v_template", R3, vt)) || (r = fetch(ps, "shapedirs", R3 * nb, sd)) || (r = fetch(ps, "expr_dirs", R3 * ne, ed)) ||
        (r = fetch(ps, "posedirs", R3 * NPF, pd)) || (r = fetch(ps, "J_regressor", (int64_t)NJ * V, jr)) ||
        (r = fetch(ps, "weights", (int64_t)V * NJ, wt)) || (r = fetch(ps, "parents", NJ, par)))
        return r;
    // the tree: every joint after the root hangs below an earlier one
    std::vector<int> parents(NJ, 0), level(NJ, 0);
    int nlevels = 1;
    for (int j = 1; j < NJ; ++j) {
        const int p = (int)par[j];
        MC_REQUIRE((float)p == par[j] && p >= 0 && p < j, "SMPL-X body model: parents[%d] = %g (the tree must be topologically ordered: 0 <= parent < joint)",
                   j, (double)par[j]);
        parents[j] = p;
        level[j] = level[p] + 1;
        nlevels = std::max(nlevels, level[j] + 1);
    }
    // J = J_regressor (v_template + shapedirs [beta; psi]) = J0 + Jdirs [beta; psi], folded in fp64
    const int Kc = nb + ne;
    std::vector<double> J0(NJ3, 0.0), JdT((size_t)Kc * NJ3, 0.0);
    for (int j = 0; j < NJ; ++j)
        for (int v = 0; v < V; ++v) {
            const double w = jr[(size_t)j * V + v];
            if (w == 0.0) continue;
            for (int c = 0; c < 3; ++c) {
                const size_t row = 3 * (size_t)v + c;
                J0[3 * j + c] += w * vt[row];
                for (int k = 0; k < nb; ++k) JdT[(size_t)k * NJ3 + 3 * j + c] += w * sd[row * nb + k];
                for (int k = 0; k < ne; ++k) JdT[(size_t)(nb + k) * NJ3 + 3 * j + c] += w * ed[row * ne + k];
            }
        }
    // skin weights: the nonzeros of each vertex (dropping exact zeros is exact)
    int maxnz = 0;
    for (int v = 0; v < V; ++v) {
        int c = 0;
        for (int j = 0; j < NJ; ++j) c += wt[(size_t)v * NJ + j] != 0.f;
        maxnz = std::max(maxnz, c);
    }
    const int NZ = maxnz <= 4 ? 4 : (maxnz <= 8 ? 8 : (maxnz <= 16 ? 16 : maxnz));      // ELL width: 4 / 8 / 16 take the register kernels
    std::vector<int> ej((size_t)NZ * V, 0);
    std::vector<float> ew((size_t)NZ * V, 0.f);
    for (int v = 0; v < V; ++v) {
        int c = 0;
        for (int j = 0; j < NJ; ++j)
            if (wt[(size_t)v * NJ + j] != 0.f) { ej[(size_t)c * V + v] = j; ew[(size_t)c * V + v] = wt[(size_t)v * NJ + j]; ++c; }
    }
    // blend-shape weight, K-contiguous: row r = [expr_dirs[r] | posedirs[r] | 0 .. Kp | shapedirs[r] | 0 .. Kfull]; rows 3V .. N4 are zero
    std::vector<float> W((size_t)m->N4 * m->Kfull, 0.f), vt4((size_t)m->N4, 0.f);
    for (long row = 0; row < R3; ++row) {
        float* w = W.data() + (size_t)row * m->Kfull;
        std::copy(ed.begin() + row * ne, ed.begin() + (row + 1) * ne, w);
        std::copy(pd.begin() + row * NPF, pd.begin() + (row + 1) * NPF, w + ne);
        std::copy(sd.begin() + row * nb, sd.begin() + (row + 1) * nb, w + m->Kp);
        vt4[row] = vt[row];
    }
    if ((r = upload_derived(ps, J0, &m->J0)) || (r = upload_derived(ps, JdT, &m->JdirsT)) || (r = upload_derived(ps, parents, &m->parents)) ||
        (r = upload_derived(ps, level, &m->level)) || (r = upload_derived(ps, ej, &m->ell_j)) || (r = upload_derived(ps, ew, &m->ell_w)) ||
        (r = upload_derived(ps, W, &m->W)) || (r = upload_derived(ps, vt4, &m->vt4)))
        return r;
    m->NZ = NZ;
    m->nlevels = nlevels;
    m->finalized = true;
    return MC_OK;
}

int mc_smplx_joints(mc_smplx* m, const double* poses, const double* expr, const double* trans, const double* betas, int32_t betas_per_frame,
                    int32_t n, float* joints_out, void* stream) {
    if (int r = check_frames(m, poses, betas, n)) return r;
    MC_REQUIRE(joints_out, "SMPL-X body model: null output");
    if (n == 0) return MC_OK;
    return launch_joints(m, poses, expr, trans, betas, betas_per_frame, n, joints_out, nullptr, (hipStream_t)stream);
}

int64_t mc_smplx_work_bytes(const mc_smplx* m, int32_t n_frames, int32_t betas_per_frame) {
    if (!m || n_frames < 0) return -1;
    const int Kc = betas_per_frame ? m->Kfull : m->Kp;
    return (int64_t)sizeof(float) * ((betas_per_frame ? 0 : m->N4) + (int64_t)n_frames * (Kc + JA + m->N4));
}

int mc_smplx_vertices(mc_smplx* m, const double* poses, const double* expr, const double* trans, const double* betas, int32_t betas_per_frame,
                      int32_t n, void* work, int64_t work_bytes, float* verts_out, float* joints_out, void* stream) {
    if (int r = check_frames(m, poses, betas, n)) return r;
    MC_REQUIRE(verts_out && work && ((uintptr_t)verts_out & 15) == 0 && ((uintptr_t)work & 15) == 0,
               "SMPL-X body model: the vertex output and the workspace must be 16-byte aligned device buffers");
    if (n == 0) return MC_OK;
    hipStream_t s = (hipStream_t)stream;
    const int Kc = betas_per_frame ? m->Kfull : m->Kp, N4 = m->N4;
    const long one = mc_smplx_work_bytes(m, 1, betas_per_frame), fixed = mc_smplx_work_bytes(m, 0, betas_per_frame);
    MC_REQUIRE(work_bytes >= one, "SMPL-X body model: the workspace holds %ld bytes, one frame needs %ld (mc_smplx_work_bytes)", (long)work_bytes, one);
    const int chunk = (int)std::min<long>((work_bytes - fixed) / (one - fixed), std::min<long>(n, 65535L * SKF));
    VertScratch w;
    w.bias = (float*)work;
    w.feat = w.bias + (betas_per_frame ? 0 : N4);
    w.A = w.feat + (long)chunk * Kc;
    w.vp = w.A + (long)chunk * JA;
    const McOptions* o = mc_process_options();
    if (!o) return MC_ERR_ARG;
    int r;
    if (!betas_per_frame && (r = launch_shape_bias(m, betas, w.bias, s))) return r;
    for (int c0 = 0; c0 < n; c0 += chunk) {
        const FrameOperands x = frames_from(m, poses, expr, trans, betas, betas_per_frame, c0);
        if ((r = vertices_chunk(m, o, x, betas_per_frame, std::min(chunk, n - c0), w, joints_out ? joints_out + (long)c0 * NJ3 : nullptr, verts_out, c0, s)))
            return r;
    }
    return MC_OK;
}

int64_t mc_smplx_vertex_errors_work_bytes(const mc_smplx* m, int32_t chunk_frames, int32_t n_frames, int32_t betas_per_frame) {
    if (!m || chunk_frames < 0 || n_frames < 0) return -1;
    const long E = 3L * m->V, c = chunk_frames;
    // per-frame partials of the two sums, the vertex path's scratch, a's vertices, b's vertices behind the previous frame's
    return (int64_t)2 * sizeof(double) * n_frames + mc_smplx_work_bytes(m, chunk_frames, betas_per_frame) +
           (int64_t)sizeof(float) * (round_up4(c * E) + round_up4((c + 1) * E));
}

int mc_smplx_vertex_errors(mc_smplx* m, const double* poses_a, const double* expr_a, const double* trans_a, const double* poses_b,
                           const double* expr_b, const double* trans_b, const double* betas, int32_t betas_per_frame, int32_t n, void* work,
                           int64_t work_bytes, double* sums_out, void* stream) {
    if (int r = check_frames(m, poses_a, betas, n)) return r;
    MC_REQUIRE(poses_b && sums_out && work && ((uintptr_t)work & 15) == 0,
               "SMPL-X vertex errors: null pose set or output, or a workspace that is not a 16-byte aligned device buffer");
    hipStream_t s = (hipStream_t)stream;
    const int Kc = betas_per_frame ? m->Kfull : m->Kp, N4 = m->N4;
    const long E = 3L * m->V, one = mc_smplx_vertex_errors_work_bytes(m, 1, n, betas_per_frame);
    MC_REQUIRE(work_bytes >= one, "SMPL-X vertex errors: the workspace holds %ld bytes, %d frames one at a time need %ld (mc_smplx_vertex_errors_work_bytes)",
               (long)work_bytes, n, one);
    int chunk = 1, top = (int)std::min<long>(std::max(n, 1), 65535L * SKF);          // the most frames per chunk that fit
    while (chunk < top) {
        const int mid = chunk + (top - chunk + 1) / 2;
        if (mc_smplx_vertex_errors_work_bytes(m, mid, n, betas_per_frame) <= work_bytes) chunk = mid; else top = mid - 1;
    }
    double* l2 = (double*)work;
    double* lvel = l2 + n;
    VertScratch w;
    w.bias = (float*)(lvel + n);
    w.feat = w.bias + (betas_per_frame ? 0 : N4);
    w.A = w.feat + (long)chunk * Kc;
    w.vp = w.A + (long)chunk * JA;
    float* va = w.vp + (long)chunk * N4;
    float* vb = va + round_up4(chunk * E);
    const McOptions* o = mc_process_options();
    if (!o) return MC_ERR_ARG;
    int r;
    if (n > 0 && !betas_per_frame && (r = launch_shape_bias(m, betas, w.bias, s))) return r;
    for (int c0 = 0; c0 < n; c0 += chunk) {
        const int nc = std::min(chunk, n - c0);
        // both vertex sets of the chunk at frame 0 of their buffers (b behind row 0, the last b frame of the chunk before)
        if ((r = vertices_chunk(m, o, frames_from(m, poses_a, expr_a, trans_a, betas, betas_per_frame, c0), betas_per_frame, nc, w, nullptr, va, 0, s)) ||
            (r = vertices_chunk(m, o, frames_from(m, poses_b, expr_b, trans_b, betas, betas_per_frame, c0), betas_per_frame, nc, w, nullptr, vb, 1, s)))
            return r;
        hipLaunchKernelGGL(vert_err_k, dim3(nc), dim3(256), 0, s, va, vb, E, (long)c0, l2, lvel);
        MC_LAUNCH_CHECK();
        if (c0 + nc < n) MC_HIP(hipMemcpyAsync(vb, vb + (long)nc * E, E * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    hipLaunchKernelGGL(vert_err_sum_k, dim3(1), dim3(256), 0, s, l2, lvel, n, sums_out);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

}  // extern "C"
