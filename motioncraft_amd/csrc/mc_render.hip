// Orthographic rasteriser for the SMPL-X mesh: fp32 vertices [n,V,3] as mc_smplx_vertices leaves them -> uint8 frames [n,H,W,3],
// the last step of the reference's tools (mogen/datasets/EMAGE_2024/utils/fast_render.py:13-81, called from
// other_tools.py:695-765), which runs pyrender + osmesa in eight host processes.  Geometry is restated exactly in numpy in
// tests/raster_ref.py; the colours are this project's own shading model, not pyrender's.
//
// Three launches per chunk of frames, all on one stream:
//   project_k  one thread per (frame, vertex): screen position snapped to 8 sub-pixel bits, the distance along the view direction,
//              and the smooth normal: the sum of the face cross products over the vertex's adjacency list IN LIST ORDER (area
//              weighted, fp32, no atomics), normalised.
//   raster_k   one thread per (frame, triangle): exact int64 edge functions at the pixel centres of the clamped bounding box, top-left
//              fill rule, fp32 depth, and a 64-bit integer atomicMin of (depth bits << 32 | face id) into the visibility buffer.
//              Positive floats order like their bit patterns, so the minimum is the nearest sample whatever the arrival order, and
//              equal depths go to the lower face id.  A plain read of the key comes first: keys only fall during this phase, so a stale
//              value can only cause an atomic that changes nothing, never suppress one that would.  A triangle whose box holds more
//              than `large_threshold` pixels is appended to a list instead (an integer atomicAdd on one counter; the order of the list
//              cannot change a minimum) and
//   raster_large_k walks each listed triangle with `large_slices` waves, interleaved by groups of 64 pixels, lanes striding the box.
//   shade_k    one thread per 4 pixels of the flat [n*H*W] pixel array (12 bytes = three dword stores; a quad that straddles the
//              chunk's first or last pixel is written byte by byte): reads the key, recomputes the exact barycentrics of the winning
//              face, interpolates and normalises the vertex normals, shades, writes depth / face when asked, and puts the key back
//              to all-ones.  Thread 0 zeroes the list counter.  So a work buffer that was clean before a call is clean after it.
// Nothing depends on the chunk size, and two runs give the same bits.
#include "mc_common.h"
#include "../../include/motioncraft_amd.h"
#include <algorithm>
#include <limits.h>
#include <math.h>
#include <new>
#include <vector>

namespace {

constexpr int GUARD = MC_RENDER_MAX_SIZE * 256;   // |snapped coordinate| <= 16384 px: differences < 2^24, products < 2^48
constexpr int OUTSIDE = INT_MIN;               // what project_k stores for a coordinate that is not finite or beyond the guard band
constexpr unsigned long long EMPTY = ~0ull;    // background key
constexpr int DEFAULT_LARGE = 1024;            // bounding-box pixels above which a triangle takes the wave path (the sweep)
constexpr int LARGE_BLOCKS = 1024;             // raster_large_k's fixed grid: 4096 waves stride the list
constexpr int DEFAULT_SLICES = 32;             // waves that share one listed triangle (the sweep)

struct Layout {                                // byte offsets into work_dev for a chunk capacity of c frames
    long counter, keys, list, screen, zcam, normal, total;
};
__host__ __device__ inline long up16(long b) { return (b + 15) / 16 * 16; }
Layout layout(long c, long W, long H, long V, long F) {
    Layout l;
    l.counter = 0;
    l.keys = 16;                               // the counter and the keys lead, so the clean region of a buffer does not move with c
    l.list = l.keys + up16(8 * c * H * W);
    l.screen = l.list + up16(4 * c * F);
    l.zcam = l.screen + up16(8 * c * V);
    l.normal = l.zcam + up16(4 * c * V);
    l.total = l.normal + up16(12 * c * V);
    return l;
}

struct Frame {                                 // what the kernels of one chunk share
    float A[12];
    float light[3], base[3];
    float ambient, gain, znear, zfar;
    int bg[3];
    int W, H, V, F, cull, large_threshold, large_slices;
};

__global__ __launch_bounds__(256) void project_k(const float* __restrict__ verts, long count, Frame fr, const int* __restrict__ faces,
                                                 const int* __restrict__ adj_start, const int* __restrict__ adj_faces, int2* __restrict__ screen,
                                                 float* __restrict__ zcam, float* __restrict__ normal, int2* __restrict__ screen_out,
                                                 float* __restrict__ zcam_out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;       // frame-in-chunk * V + vertex
    if (i >= count) return;
    const int v = (int)(i % fr.V);
    const float* fv = verts + (i - v) * 3;                     // this frame's vertices
    const float x = fv[3 * v], y = fv[3 * v + 1], z = fv[3 * v + 2];
    const float xs = fmaf(fr.A[0], x, fmaf(fr.A[1], y, fmaf(fr.A[2], z, fr.A[3])));
    const float ys = fmaf(fr.A[4], x, fmaf(fr.A[5], y, fmaf(fr.A[6], z, fr.A[7])));
    const float zc = fmaf(fr.A[8], x, fmaf(fr.A[9], y, fmaf(fr.A[10], z, fr.A[11])));
    const float fx = floorf(fmaf(256.f, xs, 0.5f)), fy = floorf(fmaf(256.f, ys, 0.5f));
    int2 s;
    s.x = fabsf(fx) <= (float)GUARD ? (int)fx : OUTSIDE;       // false for NaN
    s.y = fabsf(fy) <= (float)GUARD ? (int)fy : OUTSIDE;
    screen[i] = s;
    zcam[i] = zc;
    if (screen_out) screen_out[i] = s;
    if (zcam_out) zcam_out[i] = zc;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    for (int k = adj_start[v]; k < adj_start[v + 1]; ++k) {
        const int* f = faces + 3 * adj_faces[k];
        const float* p0 = fv + 3 * f[0];
        const float* p1 = fv + 3 * f[1];
        const float* p2 = fv + 3 * f[2];
        const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
        const float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
        nx += ay * bz - az * by;
        ny += az * bx - ax * bz;
        nz += ax * by - ay * bx;
    }
    const float l2 = nx * nx + ny * ny + nz * nz;
    const float inv = l2 > 0.f ? 1.f / sqrtf(l2) : 0.f;        // no faces, or faces that cancel: a zero normal
    normal[3 * i] = nx * inv, normal[3 * i + 1] = ny * inv, normal[3 * i + 2] = nz * inv;
}

// One triangle on the snapped grid.  Edge functions in units of 1/256 px, y down:
//   E_ab(P) = (bx - ax)(Py - ay) - (by - ay)(Px - ax);  w0 = E_12, w1 = E_20, w2 = E_01, area = w0 + w1 + w2 = E_01(v2).
// A triangle that is counter-clockwise with y up (front) has area < 0 here; `sign` turns its edge values positive inside.  An edge
// is top or left when, in the orientation that makes the inside positive, dy < 0, or dy == 0 and dx > 0; a sample on an edge belongs
// to the triangle only then: bias = 0 for such an edge and -1 otherwise, inside <=> sign * w + bias >= 0 for the three edges.
struct Tri {
    long x[3], y[3];
    long area, sign;
    long bias[3];
    float z0, dz1, dz2;
    int bx0, bx1, by0, by1;                    // clamped pixel box, inclusive
};

__device__ __forceinline__ long edge(long ax, long ay, long bx, long by, long px, long py) { return (bx - ax) * (py - ay) - (by - ay) * (px - ax); }
__device__ __forceinline__ long edge_bias(long ax, long ay, long bx, long by, long sign) {
    const long dx = (bx - ax) * sign, dy = (by - ay) * sign;
    return (dy < 0 || (dy == 0 && dx > 0)) ? 0 : -1;
}
__device__ __forceinline__ bool in_guard(int2 s) { return s.x >= -GUARD && s.x <= GUARD && s.y >= -GUARD && s.y <= GUARD; }

// false: the triangle produces no sample (bad vertex, zero area, culled, box off the viewport)
__device__ __forceinline__ bool tri_setup(Tri& t, const int* __restrict__ f, const int2* __restrict__ screen, const float* __restrict__ zcam,
                                          const Frame& fr) {
    const int2 s0 = screen[f[0]], s1 = screen[f[1]], s2 = screen[f[2]];
    const float z0 = zcam[f[0]], z1 = zcam[f[1]], z2 = zcam[f[2]];
    if (!(in_guard(s0) && in_guard(s1) && in_guard(s2))) return false;
    if (!(isfinite(z0) && isfinite(z1) && isfinite(z2))) return false;
    t.x[0] = s0.x, t.y[0] = s0.y, t.x[1] = s1.x, t.y[1] = s1.y, t.x[2] = s2.x, t.y[2] = s2.y;
    t.area = edge(t.x[0], t.y[0], t.x[1], t.y[1], t.x[2], t.y[2]);
    if (t.area == 0 || (t.area > 0 && fr.cull)) return false;
    t.sign = t.area > 0 ? 1 : -1;
    t.bias[0] = edge_bias(t.x[1], t.y[1], t.x[2], t.y[2], t.sign);
    t.bias[1] = edge_bias(t.x[2], t.y[2], t.x[0], t.y[0], t.sign);
    t.bias[2] = edge_bias(t.x[0], t.y[0], t.x[1], t.y[1], t.sign);
    t.z0 = z0, t.dz1 = z1 - z0, t.dz2 = z2 - z0;
    const long lox = min(t.x[0], min(t.x[1], t.x[2])), hix = max(t.x[0], max(t.x[1], t.x[2]));
    const long loy = min(t.y[0], min(t.y[1], t.y[2])), hiy = max(t.y[0], max(t.y[1], t.y[2]));
    // pixel centres 256 p + 128 inside [lo, hi]: p >= ceil((lo - 128) / 256), p <= floor((hi - 128) / 256); >> floors
    t.bx0 = (int)max((lox + 127) >> 8, 0L), t.bx1 = (int)min((hix - 128) >> 8, (long)fr.W - 1);
    t.by0 = (int)max((loy + 127) >> 8, 0L), t.by1 = (int)min((hiy - 128) >> 8, (long)fr.H - 1);
    return t.bx0 <= t.bx1 && t.by0 <= t.by1;
}

// the depth of the sample with edge values w1, w2, and its key into the visibility buffer when it lies in [znear, zfar]
__device__ __forceinline__ float sample_depth(const Tri& t, long w1, long w2) {
    const float b1 = (float)w1 / (float)t.area, b2 = (float)w2 / (float)t.area;
    return fmaf(b2, t.dz2, fmaf(b1, t.dz1, t.z0));
}
__device__ __forceinline__ void emit(unsigned long long* __restrict__ key, const Tri& t, long w1, long w2, int face, const Frame& fr) {
    const float z = sample_depth(t, w1, w2);
    if (!(z >= fr.znear && z <= fr.zfar)) return;
    const unsigned long long k = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)face;
    if (*key > k) atomicMin(key, k);
}

__global__ __launch_bounds__(256) void raster_k(long count, Frame fr, const int* __restrict__ faces, const int2* __restrict__ screen,
                                                const float* __restrict__ zcam, unsigned long long* __restrict__ keys, int* __restrict__ counter,
                                                unsigned* __restrict__ list) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;       // frame-in-chunk * F + face
    if (i >= count) return;
    const int face = (int)(i % fr.F);
    const long fl = i / fr.F;
    Tri t;
    if (!tri_setup(t, faces + 3 * face, screen + fl * fr.V, zcam + fl * fr.V, fr)) return;
    const long box = (long)(t.bx1 - t.bx0 + 1) * (t.by1 - t.by0 + 1);
    if (box > fr.large_threshold) {
        list[atomicAdd(counter, 1)] = (unsigned)i;
        return;
    }
    unsigned long long* fk = keys + fl * fr.H * fr.W;
    const long px0 = 256L * t.bx0 + 128;
    const long s0 = -256 * (t.y[2] - t.y[1]), s1 = -256 * (t.y[0] - t.y[2]), s2 = -256 * (t.y[1] - t.y[0]);   // per pixel step in x
    for (int y = t.by0; y <= t.by1; ++y) {
        const long py = 256L * y + 128;
        long w0 = edge(t.x[1], t.y[1], t.x[2], t.y[2], px0, py);
        long w1 = edge(t.x[2], t.y[2], t.x[0], t.y[0], px0, py);
        long w2 = edge(t.x[0], t.y[0], t.x[1], t.y[1], px0, py);
        for (int x = t.bx0; x <= t.bx1; ++x) {
            if (t.sign * w0 + t.bias[0] >= 0 && t.sign * w1 + t.bias[1] >= 0 && t.sign * w2 + t.bias[2] >= 0)
                emit(fk + (long)y * fr.W + x, t, w1, w2, face, fr);
            w0 += s0, w1 += s1, w2 += s2;
        }
    }
}

__global__ __launch_bounds__(256) void raster_large_k(Frame fr, const int* __restrict__ faces, const int2* __restrict__ screen,
                                                      const float* __restrict__ zcam, unsigned long long* __restrict__ keys,
                                                      const int* __restrict__ counter, const unsigned* __restrict__ list) {
    const int lane = threadIdx.x & 63;
    const long n = *counter;
    // fr.large_slices waves share a triangle, interleaved by groups of 64 pixels: one wave on a viewport-sized box is bound by the
    // latency of its own read-then-atomic chain
    for (long v = blockIdx.x * 4 + (threadIdx.x >> 6); v < n * fr.large_slices; v += (long)gridDim.x * 4) {
        const unsigned i = list[v / fr.large_slices];                              // < c * F <= INT_MAX
        const unsigned slice = (unsigned)(v % fr.large_slices);
        const unsigned fl = i / (unsigned)fr.F, face = i - fl * (unsigned)fr.F;
        Tri t;
        if (!tri_setup(t, faces + 3 * face, screen + (long)fl * fr.V, zcam + (long)fl * fr.V, fr)) continue;      // never: raster_k listed it
        unsigned long long* fk = keys + (long)fl * fr.H * fr.W;
        const unsigned bw = t.bx1 - t.bx0 + 1;
        const unsigned box = bw * (unsigned)(t.by1 - t.by0 + 1);                   // <= H * W <= 2^28
        for (unsigned p = 64u * slice + lane; p < box; p += 64u * fr.large_slices) {
            const unsigned row = p / bw;                                           // 32-bit: box pixels, not bytes
            const int x = t.bx0 + (int)(p - row * bw), y = t.by0 + (int)row;
            const long px = 256L * x + 128, py = 256L * y + 128;
            const long w0 = edge(t.x[1], t.y[1], t.x[2], t.y[2], px, py);
            const long w1 = edge(t.x[2], t.y[2], t.x[0], t.y[0], px, py);
            const long w2 = edge(t.x[0], t.y[0], t.x[1], t.y[1], px, py);
            if (t.sign * w0 + t.bias[0] >= 0 && t.sign * w1 + t.bias[1] >= 0 && t.sign * w2 + t.bias[2] >= 0)
                emit(fk + (long)y * fr.W + x, t, w1, w2, (int)face, fr);
        }
    }
}

// where a pixel of the chunk lies: frame in the chunk, column, row.  A thread divides once (32-bit: a chunk holds at most INT_MAX
// pixels) and steps from there.
struct Pos {
    int fl, x, y;
};
__device__ __forceinline__ Pos pos_of(unsigned lp, const Frame& fr) {
    const unsigned hw = (unsigned)fr.H * (unsigned)fr.W, fl = lp / hw, r = lp - fl * hw, y = r / (unsigned)fr.W;
    return {(int)fl, (int)(r - y * (unsigned)fr.W), (int)y};
}
__device__ __forceinline__ void pos_next(Pos& q, const Frame& fr) {
    if (++q.x == fr.W) {
        q.x = 0;
        if (++q.y == fr.H) q.y = 0, ++q.fl;
    }
}

// one pixel: key -> packed 0x00BBGGRR, the key reset, depth / face written when asked.  lp: pixel index inside the chunk, at q
__device__ __forceinline__ unsigned shade_pixel(long lp, long gp, Pos q, const Frame& fr, const int* __restrict__ faces, const int2* __restrict__ screen,
                                                const float* __restrict__ normal, unsigned long long* __restrict__ keys,
                                                int* __restrict__ face_out, float* __restrict__ depth_out) {
    const unsigned long long k = keys[lp];
    if (k == EMPTY) {
        if (face_out) face_out[gp] = -1;
        if (depth_out) depth_out[gp] = INFINITY;
        return (unsigned)fr.bg[0] | ((unsigned)fr.bg[1] << 8) | ((unsigned)fr.bg[2] << 16);
    }
    keys[lp] = EMPTY;
    const int face = (int)(unsigned)k;
    if (face_out) face_out[gp] = face;
    if (depth_out) depth_out[gp] = __uint_as_float((unsigned)(k >> 32));
    const long fl = q.fl;
    const long px = 256L * q.x + 128, py = 256L * q.y + 128;
    const int* f = faces + 3 * face;
    const int2* fs = screen + fl * fr.V;
    const int2 s0 = fs[f[0]], s1 = fs[f[1]], s2 = fs[f[2]];
    const long area = edge(s0.x, s0.y, s1.x, s1.y, s2.x, s2.y);
    const long w1 = edge(s2.x, s2.y, s0.x, s0.y, px, py), w2 = edge(s0.x, s0.y, s1.x, s1.y, px, py);
    const float b1 = (float)w1 / (float)area, b2 = (float)w2 / (float)area, b0 = 1.f - b1 - b2;
    const float* fn = normal + 3 * fl * fr.V;
    const float* n0 = fn + 3 * f[0];
    const float* n1 = fn + 3 * f[1];
    const float* n2 = fn + 3 * f[2];
    const float nx = b0 * n0[0] + b1 * n1[0] + b2 * n2[0];
    const float ny = b0 * n0[1] + b1 * n1[1] + b2 * n2[1];
    const float nz = b0 * n0[2] + b1 * n1[2] + b2 * n2[2];
    const float l2 = nx * nx + ny * ny + nz * nz;
    const float ndl = l2 > 0.f ? (nx * fr.light[0] + ny * fr.light[1] + nz * fr.light[2]) / sqrtf(l2) : 0.f;
    const float lit = fr.ambient + fr.gain * fmaxf(0.f, ndl);
    unsigned out = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) out |= (unsigned)(int)(fminf(1.f, fr.base[c] * lit) * 255.f + 0.5f) << (8 * c);
    return out;
}

// quad q holds the global pixels 4 q .. 4 q + 3 (bytes 12 q .. 12 q + 11 of rgb); the chunk holds the global pixels [g0, g1)
__global__ __launch_bounds__(256) void shade_k(long q0, long quads, long g0, long g1, Frame fr, const int* __restrict__ faces,
                                               const int2* __restrict__ screen, const float* __restrict__ normal, unsigned long long* __restrict__ keys,
                                               int* __restrict__ counter, uint8_t* __restrict__ rgb, int* __restrict__ face_out,
                                               float* __restrict__ depth_out) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t == 0) *counter = 0;
    if (t >= quads) return;
    const long p = 4 * (q0 + t);
    if (p >= g0 && p + 4 <= g1) {
        unsigned c[4];
        Pos q = pos_of((unsigned)(p - g0), fr);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c[j] = shade_pixel(p + j - g0, p + j, q, fr, faces, screen, normal, keys, face_out, depth_out);
            pos_next(q, fr);
        }
        unsigned* o = (unsigned*)(rgb + 3 * p);                // 12 q bytes from a 4-byte aligned base
        o[0] = c[0] | (c[1] << 24);
        o[1] = (c[1] >> 8) | (c[2] << 16);
        o[2] = (c[2] >> 16) | (c[3] << 8);
    } else {
        for (long g = max(p, g0); g < min(p + 4, g1); ++g) {
            const unsigned c = shade_pixel(g - g0, g, pos_of((unsigned)(g - g0), fr), fr, faces, screen, normal, keys, face_out, depth_out);
            rgb[3 * g] = (uint8_t)c, rgb[3 * g + 1] = (uint8_t)(c >> 8), rgb[3 * g + 2] = (uint8_t)(c >> 16);
        }
    }
}

}  // namespace

struct mc_render {
    int V = 0, F = 0;
    int* faces = nullptr;                      // [F,3]
    int* adj_start = nullptr;                  // [V+1]
    int* adj_faces = nullptr;                  // [adj_start[V]]
    ~mc_render() {
        (void)hipFree(faces);
        (void)hipFree(adj_start);
        (void)hipFree(adj_faces);
    }
};

static int upload_ints(int** dev, const int32_t* host, size_t n) {
    MC_HIP(hipMalloc((void**)dev, (n ? n : 1) * sizeof(int)));
    if (n) MC_HIP(hipMemcpy(*dev, host, n * sizeof(int), hipMemcpyHostToDevice));
    return MC_OK;
}

extern "C" int mc_render_create(const int32_t* faces_host, int32_t num_faces, int32_t num_vertices, const int32_t* adj_start_host,
                                const int32_t* adj_faces_host, mc_render** out) {
    MC_REQUIRE(faces_host && adj_start_host && adj_faces_host && out, "render: null argument");
    MC_REQUIRE(num_vertices >= 1 && num_faces >= 1 && num_vertices <= INT_MAX / 4 && num_faces <= INT_MAX / 4,
               "render: num_vertices=%d num_faces=%d (both in 1..%d: 32-bit element offsets)", num_vertices, num_faces, INT_MAX / 4);
    for (long i = 0; i < 3L * num_faces; ++i)
        MC_REQUIRE(faces_host[i] >= 0 && faces_host[i] < num_vertices, "render: faces[%ld][%ld] = %d is no vertex of %d", i / 3, i % 3,
                   faces_host[i], num_vertices);
    MC_REQUIRE(adj_start_host[0] == 0, "render: adj_start[0] = %d, expected 0", adj_start_host[0]);
    for (int v = 0; v < num_vertices; ++v)
        MC_REQUIRE(adj_start_host[v + 1] >= adj_start_host[v], "render: adj_start decreases at vertex %d", v);
    const long nnz = adj_start_host[num_vertices];
    MC_REQUIRE(nnz <= 3L * num_faces, "render: the adjacency holds %ld entries, more than 3 x %d faces", nnz, num_faces);
    for (int v = 0; v < num_vertices; ++v)
        for (int k = adj_start_host[v]; k < adj_start_host[v + 1]; ++k) {
            const int f = adj_faces_host[k];
            MC_REQUIRE(f >= 0 && f < num_faces, "render: adj_faces[%d] = %d is no face of %d", k, f, num_faces);
            MC_REQUIRE(faces_host[3 * f] == v || faces_host[3 * f + 1] == v || faces_host[3 * f + 2] == v,
                       "render: adj_faces[%d] = %d, but face %d does not hold vertex %d", k, f, f, v);
            MC_REQUIRE(k == adj_start_host[v] || adj_faces_host[k - 1] < f, "render: the faces of vertex %d are not in ascending order", v);
        }
    mc_render* r = new (std::nothrow) mc_render;
    MC_REQUIRE(r, "render: out of host memory");
    r->V = num_vertices, r->F = num_faces;
    int rc = upload_ints(&r->faces, faces_host, 3 * (size_t)num_faces);
    if (!rc) rc = upload_ints(&r->adj_start, adj_start_host, (size_t)num_vertices + 1);
    if (!rc) rc = upload_ints(&r->adj_faces, adj_faces_host, (size_t)nnz);
    if (rc) {
        delete r;
        return rc;
    }
    *out = r;
    return MC_OK;
}

extern "C" void mc_render_destroy(mc_render* r) { delete r; }

static bool size_ok(int32_t width, int32_t height) { return width >= 1 && height >= 1 && width <= MC_RENDER_MAX_SIZE && height <= MC_RENDER_MAX_SIZE; }

extern "C" int64_t mc_render_work_bytes(const mc_render* r, int32_t n_frames, int32_t width, int32_t height) {
    if (!r || n_frames < 1 || !size_ok(width, height)) return -1;
    return layout(n_frames, width, height, r->V, r->F).total;
}

extern "C" int mc_render_frames(mc_render* r, const float* verts_dev, int32_t n, const mc_render_params* p, void* work_dev, int64_t work_bytes,
                                int32_t work_clean, uint8_t* rgb_out_dev, int32_t* face_out_dev, float* depth_out_dev, int32_t* screen_out_dev,
                                float* zcam_out_dev, void* stream) {
    MC_REQUIRE(r && p && rgb_out_dev && work_dev && (verts_dev || n == 0), "render: null argument");
    MC_REQUIRE(n >= 0, "render: n=%d", n);
    MC_REQUIRE(size_ok(p->width, p->height), "render: width=%d height=%d (1..%d each, the guard band)", p->width, p->height, MC_RENDER_MAX_SIZE);
    MC_REQUIRE(p->znear > 0.f && p->zfar >= p->znear && isfinite(p->zfar), "render: znear=%g zfar=%g (0 < znear <= zfar < inf: depth keys order as "
               "integers only for positive floats)", (double)p->znear, (double)p->zfar);
    for (int c = 0; c < 3; ++c)
        MC_REQUIRE(p->background[c] >= 0 && p->background[c] <= 255 && p->base[c] >= 0.f && p->base[c] <= 1.f,
                   "render: background must be 0..255 and base 0..1 per channel");
    MC_REQUIRE(p->large_threshold >= 0, "render: large_threshold=%d (0 = default)", p->large_threshold);
    MC_REQUIRE(p->large_slices >= 0 && p->large_slices <= MC_RENDER_MAX_SLICES, "render: large_slices=%d (0 = default, at most %d)", p->large_slices, MC_RENDER_MAX_SLICES);
    MC_REQUIRE(((uintptr_t)work_dev & 15) == 0 && ((uintptr_t)rgb_out_dev & 3) == 0 && ((uintptr_t)verts_dev & 3) == 0,
               "render: work must be 16-byte, rgb_out and verts 4-byte aligned");
    const long W = p->width, H = p->height, V = r->V, F = r->F;
    const long one = layout(1, W, H, V, F).total;
    MC_REQUIRE(work_bytes >= one, "render: work_bytes=%ld, one %ldx%ld frame needs %ld", (long)work_bytes, W, H, one);
    long cap = 1;                              // the frames work_dev holds: the largest c with layout(c).total <= work_bytes
    for (long hi = work_bytes / (8 * H * W + 4 * F + 24 * V); cap < hi;) {
        const long mid = (cap + hi + 1) / 2;
        if (layout(mid, W, H, V, F).total <= work_bytes) cap = mid;
        else hi = mid - 1;
    }
    cap = std::min(cap, (long)INT_MAX / std::max(std::max(F, V), H * W));      // what one launch and a 32-bit list entry index
    const Layout l = layout(cap, W, H, V, F);
    char* w = (char*)work_dev;
    hipStream_t s = (hipStream_t)stream;
    int* counter = (int*)(w + l.counter);
    unsigned long long* keys = (unsigned long long*)(w + l.keys);
    if (!work_clean) {
        MC_HIP(hipMemsetAsync(counter, 0, 16, s));
        MC_HIP(hipMemsetAsync(keys, 0xFF, (size_t)(8 * cap * H * W), s));
    }
    Frame fr;
    for (int i = 0; i < 12; ++i) fr.A[i] = p->screen[i];
    for (int i = 0; i < 3; ++i) fr.light[i] = p->light[i], fr.base[i] = p->base[i], fr.bg[i] = p->background[i];
    fr.ambient = p->ambient, fr.gain = p->gain, fr.znear = p->znear, fr.zfar = p->zfar;
    fr.W = (int)W, fr.H = (int)H, fr.V = (int)V, fr.F = (int)F, fr.cull = p->cull_backfaces != 0;
    fr.large_threshold = p->large_threshold ? p->large_threshold : DEFAULT_LARGE;
    fr.large_slices = p->large_slices ? p->large_slices : DEFAULT_SLICES;
    unsigned* list = (unsigned*)(w + l.list);
    int2* screen = (int2*)(w + l.screen);
    float* zcam = (float*)(w + l.zcam);
    float* normal = (float*)(w + l.normal);
    for (long f0 = 0; f0 < n; f0 += cap) {
        const long c = std::min(cap, (long)n - f0);
        hipLaunchKernelGGL(project_k, dim3(cdiv(c * V, 256)), dim3(256), 0, s, verts_dev + f0 * V * 3, c * V, fr, r->faces, r->adj_start, r->adj_faces,
                           screen, zcam, normal, screen_out_dev ? (int2*)screen_out_dev + f0 * V : nullptr, zcam_out_dev ? zcam_out_dev + f0 * V : nullptr);
        MC_LAUNCH_CHECK();
        hipLaunchKernelGGL(raster_k, dim3(cdiv(c * F, 256)), dim3(256), 0, s, c * F, fr, r->faces, screen, zcam, keys, counter, list);
        MC_LAUNCH_CHECK();
        hipLaunchKernelGGL(raster_large_k, dim3(LARGE_BLOCKS), dim3(256), 0, s, fr, r->faces, screen, zcam, keys, counter, list);
        MC_LAUNCH_CHECK();
        const long g0 = f0 * H * W, g1 = (f0 + c) * H * W, q0 = g0 / 4, quads = (g1 + 3) / 4 - q0;
        hipLaunchKernelGGL(shade_k, dim3(cdiv(quads, 256)), dim3(256), 0, s, q0, quads, g0, g1, fr, r->faces, screen, normal, keys, counter,
                           rgb_out_dev, face_out_dev, depth_out_dev);
        MC_LAUNCH_CHECK();
    }
    return MC_OK;
}
