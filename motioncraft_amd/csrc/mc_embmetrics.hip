// The quality metrics of mogen/core/evaluation/utils.py reduced from embedding tables on the device, in fp64.
//
// Frechet distance without a covariance or a matrix root.  With A_c [n, d], B_c [m, d] the column-centred tables,
//     Tr sqrt(C1 C2) = || A_c B_c^T ||_* / sqrt((n - 1)(m - 1)),      Tr C1 = || A_c ||_F^2 / (n - 1),
// and the nuclear norm is the sum of the singular values of a small matrix K = F1^T F2 built from one factor per table:
//     n >= d:  A_c = U S V^T,  F = V S   [d, d]  (one-sided Jacobi on A_c with an appended identity block that accumulates V)
//     n <  d:  A_c = Q G^T,    F = G     [d, n]  (one-sided Jacobi on A_c^T: its columns, the centred rows, made orthogonal)
// so the decompositions run over min(n, d) columns, and a third Jacobi run on K ends in its singular values as column norms.
//
// One-sided Jacobi (Hestenes): a round-robin schedule pairs all columns in m - 1 rounds (m = c rounded up to even, the odd one
// out sits a round out against the bye); the pairs of a round are disjoint, so one launch runs them in parallel, one workgroup per
// pair: alpha = |a_p|^2, beta = |a_q|^2, gamma = a_p . a_q over the r data rows, skipped when |gamma| <= tol sqrt(alpha) sqrt(beta)
// or when either squared norm is at or below floor2 (2^-1000 of the largest squared column norm at the start: zero columns, the
// normal case for a rank-deficient table, never reach a division), else the plane rotation with tan = sign(z) / (|z| + sqrt(1 + z^2)),
// z = (beta - alpha) / (2 gamma) over all rows, the identity block included.  Rounds are separated by kernel boundaries; after each
// sweep the host reads one int32, the number of pairs rotated, and stops at zero or at the sweep cap (an error).  Every sum is a
// per-thread strided sum followed by the fixed wave / workgroup tree of mc_common.h, the counter is an integer: two runs give the
// same bits.
#include "mc_common.h"
#include <float.h>
#include <math.h>

namespace {

constexpr int MAX_DIM = MC_EMB_MAX_DIM, MAX_ROWS = MC_EMB_MAX_ROWS, MAX_BATCH = MC_EMB_MAX_BATCH, MAX_TOPK = MC_EMB_MAX_TOPK;

__device__ __forceinline__ double ld_tab(const void* t, long i, int f64) { return f64 ? ((const double*)t)[i] : (double)((const float*)t)[i]; }

// ---- 1. column statistics ---------------------------------------------------------------------------------------------------
// 256 threads = 4 waves x 64 columns: lane = column (coalesced rows), wave w sums rows w, w + 4, ...; the four partial sums are
// added as ((s0 + s1) + s2) + s3.  mean_out [d] (scaled), cen_out[i * cen_rs + j * cen_cs] = (x - mean) * scale, z_out [n, d].
__global__ __launch_bounds__(256) void colstats_k(const void* __restrict__ tab, int f64, int n, int d, double scale, double* __restrict__ mean_out,
                                                  double* __restrict__ cen_out, long cen_rs, long cen_cs, double* __restrict__ z_out) {
    __shared__ double sh[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, j = blockIdx.x * 64 + lane;
    const bool live = j < d;
    double s = 0.0;
    if (live) for (int i = w; i < n; i += 4) s += ld_tab(tab, (long)i * d + j, f64);
    sh[w][lane] = s;
    __syncthreads();
    const double mean = (((sh[0][lane] + sh[1][lane]) + sh[2][lane]) + sh[3][lane]) / (double)n;
    __syncthreads();
    double sd = 1.0;
    if (z_out) {
        double v = 0.0;
        if (live) for (int i = w; i < n; i += 4) { const double c = ld_tab(tab, (long)i * d + j, f64) - mean; v = fma(c, c, v); }
        sh[w][lane] = v;
        __syncthreads();
        sd = sqrt((((sh[0][lane] + sh[1][lane]) + sh[2][lane]) + sh[3][lane]) / (double)n);
        if (sd == 0.0) sd = 1e-8;
    }
    if (!live) return;
    if (w == 0 && mean_out) mean_out[j] = mean * scale;
    for (int i = w; i < n; i += 4) {
        const double c = ld_tab(tab, (long)i * d + j, f64) - mean;
        if (cen_out) cen_out[i * cen_rs + j * cen_cs] = c * scale;
        if (z_out) z_out[(long)i * d + j] = c / sd;
    }
}

// ---- 2. one-sided Jacobi -----------------------------------------------------------------------------------------------------
// squared norms of the first r rows of each column of W [ld, c] (column-major); sqrt_out: the norms themselves
__global__ __launch_bounds__(256) void colnorm_k(const double* __restrict__ W, int r, long ld, double* __restrict__ out, int sqrt_out) {
    __shared__ double sh[4];
    const double* a = W + blockIdx.x * ld;
    double s = 0.0;
    for (int i = threadIdx.x; i < r; i += 256) s = fma(a[i], a[i], s);
    s = block_sum_f64(s, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = sqrt_out ? sqrt(s) : s;
}

// floor2 = 2^-1000 of the largest of c squared norms; *trace = their sum in index order; the identity block under W (with_v)
__global__ __launch_bounds__(256) void jacobi_init_k(const double* __restrict__ norm2, int c, double* __restrict__ floor2, double* __restrict__ trace,
                                                     double* __restrict__ W, int r, long ld, int with_v) {
    if (with_v)
        for (long e = threadIdx.x; e < (long)c * c; e += 256) W[(e / c) * ld + r + e % c] = (e / c == e % c) ? 1.0 : 0.0;
    if (threadIdx.x == 0) {
        double mx = 0.0, tr = 0.0;
        for (int j = 0; j < c; ++j) { mx = fmax(mx, norm2[j]); tr += norm2[j]; }
        *floor2 = ldexp(mx, -1000);
        if (trace) *trace = tr;
    }
}

// the pair of slot `i` in round `k` of the round-robin over m (even) players: player m - 1 stays, the others rotate
__host__ __device__ inline void rr_pair(int m, int k, int i, int* p, int* q) {
    const int a = i == 0 ? m - 1 : (k + i) % (m - 1), b = i == 0 ? k : (k - i + (m - 1)) % (m - 1);
    *p = a < b ? a : b;
    *q = a < b ? b : a;
}

__global__ __launch_bounds__(256) void jacobi_round_k(double* __restrict__ W, int r, int rtot, long ld, int c, int m, int round, double tol,
                                                      const double* __restrict__ floor2, int* __restrict__ rotated) {
    __shared__ double sh[3][4];
    int p, q;
    rr_pair(m, round, blockIdx.x, &p, &q);
    if (q >= c) return;                                         // the bye
    double* ap = W + p * ld;
    double* aq = W + q * ld;
    double al = 0.0, be = 0.0, ga = 0.0;
    for (int i = threadIdx.x; i < r; i += 256) {
        const double x = ap[i], y = aq[i];
        al = fma(x, x, al); be = fma(y, y, be); ga = fma(x, y, ga);
    }
    al = wave_sum_f64(al); be = wave_sum_f64(be); ga = wave_sum_f64(ga);
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = al; sh[1][threadIdx.x >> 6] = be; sh[2][threadIdx.x >> 6] = ga; }
    __syncthreads();
    al = ((sh[0][0] + sh[0][1]) + sh[0][2]) + sh[0][3];
    be = ((sh[1][0] + sh[1][1]) + sh[1][2]) + sh[1][3];
    ga = ((sh[2][0] + sh[2][1]) + sh[2][2]) + sh[2][3];
    const double fl = *floor2;
    if (al <= fl || be <= fl || !(fabs(ga) > tol * (sqrt(al) * sqrt(be)))) return;       // uniform over the workgroup
    const double z = (be - al) / (2.0 * ga);
    const double t = (z >= 0.0 ? 1.0 : -1.0) / (fabs(z) + sqrt(1.0 + z * z));
    const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
    for (int i = threadIdx.x; i < rtot; i += 256) {
        const double x = ap[i], y = aq[i];
        ap[i] = cs * x - sn * y;
        aq[i] = sn * x + cs * y;
    }
    if (threadIdx.x == 0) atomicAdd(rotated, 1);
}

// ---- 3. K = diag(s1) F1^T F2 diag(s2) * scale: 16 x 16 output tiles, the inner dimension in LDS chunks of 16 ---------------------
// F1 [len, k1] and F2 [len, k2] column-major with leading dimensions ld1 / ld2; K [k1, k2] column-major; s1 / s2 may be null (ones)
__global__ __launch_bounds__(256) void kform_k(const double* __restrict__ F1, long ld1, const double* __restrict__ s1, int k1, const double* __restrict__ F2,
                                               long ld2, const double* __restrict__ s2, int k2, int len, double scale, double* __restrict__ K) {
    __shared__ double t1[16][17], t2[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int i0 = blockIdx.x * 16, j0 = blockIdx.y * 16;
    double acc = 0.0;
    for (int e0 = 0; e0 < len; e0 += 16) {
        // t1[col][e], t2[col][e]: thread (tx = e, ty = col) reads down a column, 16 consecutive doubles per column
        t1[ty][tx] = (i0 + ty < k1 && e0 + tx < len) ? F1[(i0 + ty) * ld1 + e0 + tx] : 0.0;
        t2[ty][tx] = (j0 + ty < k2 && e0 + tx < len) ? F2[(j0 + ty) * ld2 + e0 + tx] : 0.0;
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 16; ++e) acc = fma(t1[tx][e], t2[ty][e], acc);
        __syncthreads();
    }
    const int i = i0 + tx, j = j0 + ty;
    if (i < k1 && j < k2) K[i + (long)j * k1] = ((s1 ? s1[i] : 1.0) * (s2 ? s2[j] : 1.0)) * acc * scale;
}

__global__ void frechet_final_k(const double* __restrict__ mu1, const double* __restrict__ mu2, int d, const double* __restrict__ tr1,
                                const double* __restrict__ tr2, const double* __restrict__ sv, int nsv, int n, int m, double* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double dm = 0.0, nuc = 0.0;
    for (int j = 0; j < d; ++j) { const double t = mu1[j] - mu2[j]; dm = fma(t, t, dm); }
    for (int j = 0; j < nsv; ++j) nuc += sv[j];
    *out = dm + *tr1 / (double)(n - 1) + *tr2 / (double)(m - 1) - 2.0 * nuc / sqrt((double)(n - 1) * (double)(m - 1));
}

// ---- 4. retrieval: one workgroup per batch of nb <= 64 rows -------------------------------------------------------------------------
__global__ __launch_bounds__(256) void retrieval_k(const void* __restrict__ text, const void* __restrict__ motion, int f64, int n_total, int d, int batch,
                                                   int top_k, int* __restrict__ counts, double* __restrict__ match_sum) {
    __shared__ double dist[MAX_BATCH * MAX_BATCH];
    const int b0 = blockIdx.x * batch, nb = min(batch, n_total - b0);
    for (int e = threadIdx.x; e < nb * nb; e += 256) {
        const long ti = (long)(b0 + e / nb) * d, mj = (long)(b0 + e % nb) * d;
        double s = 0.0;
        for (int k = 0; k < d; ++k) { const double t = ld_tab(text, ti + k, f64) - ld_tab(motion, mj + k, f64); s = fma(t, t, s); }
        dist[e] = sqrt(s);
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;
    const int i = threadIdx.x;
    int rank = MAX_BATCH;
    if (i < nb) {
        const double own = dist[i * nb + i];
        rank = 0;
        for (int j = 0; j < nb; ++j) rank += (dist[i * nb + j] < own) || (j < i && dist[i * nb + j] == own);
    }
    for (int k = 1; k <= top_k; ++k) {
        const unsigned long long hit = __ballot(i < nb && rank < k);
        if (i == 0) counts[blockIdx.x * top_k + k - 1] = __popcll(hit);
    }
    if (match_sum && i == 0) {
        double s = 0.0;
        for (int r = 0; r < nb; ++r) s += dist[r * nb + r];
        match_sum[blockIdx.x] = s;
    }
}

// ---- 5. gathered pair distances: mean over groups x pairs of |((a[g, f] * es) - (a[g, s] * es)) * ns| --------------------------------
__global__ __launch_bounds__(256) void pair_distance_k(const void* __restrict__ tab, int f64, int groups, int rows, int d, const int* __restrict__ first,
                                                       const int* __restrict__ second, int n_pairs, double es, double ns, double* __restrict__ out) {
    __shared__ double sh[4];
    const long total = (long)groups * n_pairs;
    double acc = 0.0;
    for (long e = threadIdx.x; e < total; e += 256) {
        const int g = (int)(e / n_pairs), p = (int)(e % n_pairs);
        const int f = min(max(first[p], 0), rows - 1), s = min(max(second[p], 0), rows - 1);        // an index out of range never leaves the table
        const long fo = ((long)g * rows + f) * d, so = ((long)g * rows + s) * d;
        double q = 0.0;
        for (int k = 0; k < d; ++k) { const double t = (ld_tab(tab, fo + k, f64) * es - ld_tab(tab, so + k, f64) * es) * ns; q = fma(t, t, q); }
        acc += sqrt(q);
    }
    acc = block_sum_f64(acc, sh);
    if (threadIdx.x == 0) *out = acc / (double)total;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
bool on_device(const void* p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}
#define MC_REQUIRE_DEV(p, what) MC_REQUIRE(on_device(p), "%s: %s must be a device pointer", what, #p)

bool dims_ok(int64_t n, int64_t d) { return n >= 2 && n <= MAX_ROWS && d >= 1 && d <= MAX_DIM; }

struct Side {                        // one table of the Frechet distance inside the workspace
    int n, d, tall, k;               // k = min(n, d) columns of the factor
    int r, rtot;                     // Jacobi: data rows, rows with the identity block
    double *mean, *W, *norm2, *sig, *trace;
    const double* F() const { return tall ? W + r : W; }          // factor column j at F() + j * rtot, d long
};

long side_doubles(int n, int d) { return (n >= d ? ((long)n + d) * d : (long)d * n) + d /*mean*/ + 2L * (n >= d ? d : n) /*norm2, sig*/ + 1 /*trace*/; }

double* carve(Side& s, int n, int d, double* w) {
    s.n = n; s.d = d; s.tall = n >= d; s.k = s.tall ? d : n;
    s.r = s.tall ? n : d; s.rtot = s.tall ? n + d : d;
    s.mean = w; w += d;
    s.W = w; w += (long)s.rtot * s.k;
    s.norm2 = w; w += s.k;
    s.sig = w; w += s.k;
    s.trace = w; w += 1;
    return w;
}

// Jacobi on W [rtot, c] column-major (r data rows): norm2 = scratch [c].  info[0] = sweeps, info[1] = round launches.
int jacobi(double* W, int r, int rtot, int c, int with_v, double* norm2, double* trace, double* floor2, int* rotated, int max_sweeps, int* info,
           hipStream_t s, const char* what) {
    hipLaunchKernelGGL(colnorm_k, dim3(c), dim3(256), 0, s, W, r, (long)rtot, norm2, 0);
    MC_LAUNCH_CHECK();
    hipLaunchKernelGGL(jacobi_init_k, dim3(1), dim3(256), 0, s, norm2, c, floor2, trace, W, r, (long)rtot, with_v);
    MC_LAUNCH_CHECK();
    info[0] = info[1] = 0;
    if (c < 2) return MC_OK;
    const int m = c + (c & 1);
    const double tol = DBL_EPSILON * sqrt((double)r);
    for (int sweep = 0; sweep < max_sweeps; ++sweep) {
        MC_HIP(hipMemsetAsync(rotated, 0, sizeof(int), s));
        for (int k = 0; k < m - 1; ++k) {
            hipLaunchKernelGGL(jacobi_round_k, dim3(m / 2), dim3(256), 0, s, W, r, rtot, (long)rtot, c, m, k, tol, floor2, rotated);
            MC_LAUNCH_CHECK();
        }
        int left = -1;
        MC_HIP(hipMemcpyAsync(&left, rotated, sizeof(int), hipMemcpyDeviceToHost, s));
        MC_HIP(hipStreamSynchronize(s));
        info[0] = sweep + 1; info[1] += m - 1;
        if (left == 0) return MC_OK;
    }
    mc_set_error("%s: the one-sided Jacobi iteration on %d columns of %d rows still rotated pairs in sweep %d (the cap; MC_EMB_MAX_SWEEPS = %d)", what, c, r,
                 max_sweeps, MC_EMB_MAX_SWEEPS);
    return MC_ERR_NOCONV;
}

int centre(const void* tab, int f64, const Side& sd, double scale, hipStream_t s) {
    // tall: W[j * rtot + i]; short: the transpose, W[i * d + j]
    hipLaunchKernelGGL(colstats_k, dim3(cdiv(sd.d, 64)), dim3(256), 0, s, tab, f64, sd.n, sd.d, scale, sd.mean, sd.W, sd.tall ? 1L : (long)sd.d,
                       sd.tall ? (long)sd.rtot : 1L, (double*)nullptr);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

}  // namespace

extern "C" {

int64_t mc_emb_frechet_work_bytes(int32_t n, int32_t m, int32_t d) {
    if (!dims_ok(n, d) || !dims_ok(m, d)) return -1;
    const long k1 = n >= d ? d : n, k2 = m >= d ? d : m;
    return (int64_t)sizeof(double) * (side_doubles(n, d) + side_doubles(m, d) + k1 * k2 + (k1 < k2 ? k1 : k2) /*K and its norms*/ + 2 /*floor2, counter*/);
}

int mc_emb_frechet(const void* gt_dev, int32_t n, const void* pred_dev, int32_t m, int32_t d, int32_t table_fp64, double emb_scale, int32_t max_sweeps,
                   void* work_dev, int64_t work_bytes, double* fid_out_dev, int32_t* info_host, void* stream) {
    MC_REQUIRE(gt_dev && pred_dev && work_dev && fid_out_dev, "frechet distance: null argument");
    MC_REQUIRE(dims_ok(n, d) && dims_ok(m, d), "frechet distance: tables [%d, %d] and [%d, %d] (2..%d rows, 1..%d columns)", n, d, m, d, MAX_ROWS, MAX_DIM);
    MC_REQUIRE(max_sweeps >= 0 && max_sweeps <= MC_EMB_MAX_SWEEPS, "frechet distance: max_sweeps=%d (0 = the cap, 1..%d)", max_sweeps, MC_EMB_MAX_SWEEPS);
    MC_REQUIRE(((uintptr_t)work_dev & 7) == 0 && work_bytes >= mc_emb_frechet_work_bytes(n, m, d),
               "frechet distance: the workspace must be 8-byte aligned and hold %ld bytes (mc_emb_frechet_work_bytes), got %ld",
               (long)mc_emb_frechet_work_bytes(n, m, d), (long)work_bytes);
    MC_REQUIRE_DEV(gt_dev, "frechet distance"); MC_REQUIRE_DEV(pred_dev, "frechet distance");
    MC_REQUIRE_DEV(work_dev, "frechet distance"); MC_REQUIRE_DEV(fid_out_dev, "frechet distance");
    const int cap = max_sweeps ? max_sweeps : MC_EMB_MAX_SWEEPS;
    hipStream_t s = (hipStream_t)stream;
    Side a, b;
    double* w = carve(a, n, d, (double*)work_dev);
    w = carve(b, m, d, w);
    // K [kr, kc] with kc <= kr: the side with fewer factor columns gives K's columns
    const Side& rowside = a.k >= b.k ? a : b;
    const Side& colside = a.k >= b.k ? b : a;
    const int kr = rowside.k, kc = colside.k;
    double* K = w; w += (long)kr * kc;
    double* knorm = w; w += kc;
    double* floor2 = w; w += 1;
    int* rotated = (int*)w;
    int info[6] = {0, 0, 0, 0, 0, 0};
    int rc = MC_OK;
    const void* tabs[2] = {gt_dev, pred_dev};
    Side* sides[2] = {&a, &b};
    for (int t = 0; t < 2 && rc == MC_OK; ++t) {
        Side& sd = *sides[t];
        rc = centre(tabs[t], table_fp64 != 0, sd, emb_scale, s);
        if (rc == MC_OK) rc = jacobi(sd.W, sd.r, sd.rtot, sd.k, sd.tall, sd.norm2, sd.trace, floor2, rotated, cap, info + 2 * t, s, "frechet distance");
        if (rc == MC_OK && sd.tall) {
            hipLaunchKernelGGL(colnorm_k, dim3(sd.k), dim3(256), 0, s, sd.W, sd.r, (long)sd.rtot, sd.sig, 1);
            MC_LAUNCH_CHECK();
        }
    }
    if (rc == MC_OK) {
        hipLaunchKernelGGL(kform_k, dim3(cdiv(kr, 16), cdiv(kc, 16)), dim3(256), 0, s, rowside.F(), (long)rowside.rtot, rowside.tall ? rowside.sig : nullptr, kr,
                           colside.F(), (long)colside.rtot, colside.tall ? colside.sig : nullptr, kc, d, 1.0, K);
        MC_LAUNCH_CHECK();
        rc = jacobi(K, kr, kr, kc, 0, knorm, nullptr, floor2, rotated, cap, info + 4, s, "frechet distance");
    }
    if (info_host) for (int i = 0; i < 6; ++i) info_host[i] = info[i];
    if (rc != MC_OK) return rc;
    hipLaunchKernelGGL(colnorm_k, dim3(kc), dim3(256), 0, s, K, kr, (long)kr, knorm, 1);
    MC_LAUNCH_CHECK();
    hipLaunchKernelGGL(frechet_final_k, dim3(1), dim3(64), 0, s, a.mean, b.mean, d, a.trace, b.trace, knorm, kc, n, m, fid_out_dev);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int64_t mc_emb_statistics_work_bytes(int32_t n, int32_t d) {
    if (!dims_ok(n, d)) return -1;
    return (int64_t)sizeof(double) * n * d;
}

int mc_emb_statistics(const void* table_dev, int32_t n, int32_t d, int32_t table_fp64, double emb_scale, void* work_dev, int64_t work_bytes,
                      double* mean_out_dev, double* cov_out_dev, void* stream) {
    MC_REQUIRE(table_dev && work_dev && mean_out_dev && cov_out_dev, "activation statistics: null argument");
    MC_REQUIRE(dims_ok(n, d), "activation statistics: table [%d, %d] (2..%d rows, 1..%d columns)", n, d, MAX_ROWS, MAX_DIM);
    MC_REQUIRE(((uintptr_t)work_dev & 7) == 0 && work_bytes >= mc_emb_statistics_work_bytes(n, d),
               "activation statistics: the workspace must be 8-byte aligned and hold %ld bytes (mc_emb_statistics_work_bytes), got %ld",
               (long)mc_emb_statistics_work_bytes(n, d), (long)work_bytes);
    MC_REQUIRE_DEV(table_dev, "activation statistics"); MC_REQUIRE_DEV(work_dev, "activation statistics");
    MC_REQUIRE_DEV(mean_out_dev, "activation statistics"); MC_REQUIRE_DEV(cov_out_dev, "activation statistics");
    hipStream_t s = (hipStream_t)stream;
    double* W = (double*)work_dev;
    hipLaunchKernelGGL(colstats_k, dim3(cdiv(d, 64)), dim3(256), 0, s, table_dev, table_fp64 != 0, n, d, emb_scale, mean_out_dev, W, 1L, (long)n, (double*)nullptr);
    MC_LAUNCH_CHECK();
    hipLaunchKernelGGL(kform_k, dim3(cdiv(d, 16), cdiv(d, 16)), dim3(256), 0, s, W, (long)n, (const double*)nullptr, d, W, (long)n, (const double*)nullptr, d, n,
                       1.0 / (double)(n - 1), cov_out_dev);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int mc_emb_zscore(const void* table_dev, int32_t n, int32_t d, int32_t table_fp64, double* out_dev, void* stream) {
    MC_REQUIRE(table_dev && out_dev, "z-score: null argument");
    MC_REQUIRE(n >= 1 && n <= MAX_ROWS && d >= 1 && d <= MAX_DIM, "z-score: table [%d, %d] (1..%d rows, 1..%d columns)", n, d, MAX_ROWS, MAX_DIM);
    MC_REQUIRE_DEV(table_dev, "z-score"); MC_REQUIRE_DEV(out_dev, "z-score");
    hipLaunchKernelGGL(colstats_k, dim3(cdiv(d, 64)), dim3(256), 0, (hipStream_t)stream, table_dev, table_fp64 != 0, n, d, 1.0, (double*)nullptr, (double*)nullptr,
                       0L, 0L, out_dev);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int mc_emb_retrieval(const void* text_dev, const void* motion_dev, int32_t n, int32_t d, int32_t table_fp64, int32_t batch, int32_t top_k,
                     int32_t* counts_out_dev, double* match_sum_out_dev, void* stream) {
    MC_REQUIRE(text_dev && motion_dev && counts_out_dev, "retrieval: null argument");
    MC_REQUIRE(n >= 1 && n <= MAX_ROWS && d >= 1 && d <= MAX_DIM, "retrieval: tables [%d, %d] (1..%d rows, 1..%d columns)", n, d, MAX_ROWS, MAX_DIM);
    MC_REQUIRE(batch >= 1 && batch <= MAX_BATCH && top_k >= 1 && top_k <= MAX_TOPK, "retrieval: batch=%d (1..%d), top_k=%d (1..%d)", batch, MAX_BATCH, top_k,
               MAX_TOPK);
    MC_REQUIRE_DEV(text_dev, "retrieval"); MC_REQUIRE_DEV(motion_dev, "retrieval"); MC_REQUIRE_DEV(counts_out_dev, "retrieval");
    if (match_sum_out_dev) MC_REQUIRE_DEV(match_sum_out_dev, "retrieval");
    hipLaunchKernelGGL(retrieval_k, dim3(cdiv(n, batch)), dim3(256), 0, (hipStream_t)stream, text_dev, motion_dev, table_fp64 != 0, n, d, batch, top_k,
                       counts_out_dev, match_sum_out_dev);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

int mc_emb_pair_distance(const void* table_dev, int32_t groups, int32_t rows, int32_t d, int32_t table_fp64, const int32_t* first_dev,
                         const int32_t* second_dev, int32_t n_pairs, double emb_scale, double norm_scale, double* mean_out_dev, void* stream) {
    MC_REQUIRE(table_dev && first_dev && second_dev && mean_out_dev, "pair distance: null argument");
    MC_REQUIRE(groups >= 1 && rows >= 1 && (int64_t)groups * rows <= MAX_ROWS && d >= 1 && d <= MAX_DIM,
               "pair distance: table [%d, %d, %d] (up to %d rows in all, 1..%d columns)", groups, rows, d, MAX_ROWS, MAX_DIM);
    MC_REQUIRE(n_pairs >= 1 && n_pairs <= MAX_ROWS, "pair distance: %d pairs (1..%d)", n_pairs, MAX_ROWS);
    MC_REQUIRE_DEV(table_dev, "pair distance"); MC_REQUIRE_DEV(first_dev, "pair distance"); MC_REQUIRE_DEV(second_dev, "pair distance");
    MC_REQUIRE_DEV(mean_out_dev, "pair distance");
    hipLaunchKernelGGL(pair_distance_k, dim3(1), dim3(256), 0, (hipStream_t)stream, table_dev, table_fp64 != 0, groups, rows, d, first_dev, second_dev, n_pairs,
                       emb_scale, norm_scale, mean_out_dev);
    MC_LAUNCH_CHECK();
    return MC_OK;
}

}  // extern "C"
