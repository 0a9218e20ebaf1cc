// Capsule rasteriser for skeleton animations: fp32 joints [n,J,3] as mc_postprocess_t2m_joints* leaves them -> uint8 frames [n,H,W,3],
// the picture the reference's text-to-motion tool ends with (plot_3d_motion of mogen/utils/plot_utils.py:107-204, called from
// tools/visualize.py:46-56), which draws every frame with matplotlib's mplot3d on the host.  The scene and the rules are restated in
// numpy / Python integers in tests/skeleton_ref.py.  Not drawn: the title, anti-aliasing and mplot3d's projecting caps (every segment
// is a capsule with round caps, which gives round joins); pixel parity with matplotlib's Agg output is not claimed.
//
// THE SCENE.  The rows of `joints` are split into sequences by seq_start.  Per sequence, MINS and MAXS are the fp32 minimum and
// maximum per axis over all its frames and joints (non-finite values ignored; +inf / -inf when there is none), and traj[i] is the
// root joint's (x, z) at its frame i.  Frame i draws, in painter's order,
//   layer 1      the ground quad at y = 0 with the corners (MINS_x, MINS_z), (MINS_x, MAXS_z), (MAXS_x, MAXS_z), (MAXS_x, MINS_z) moved by
//                -traj[i]: the two triangles (0, 1, 2) and (0, 2, 3) of these corners;
//   layer 2      for i >= 2 only, the trail: the polyline through (traj[j] - traj[i], 0) for j = 0 .. i-1, i - 1 segments;
//   layer 3 + c  chain c: the polyline through (x - traj_x[i], y - MINS_y, z - traj_z[i]) of its joints.
// mplot3d has no depth buffer, later artists overwrite earlier ones: a pixel's layer is the MAXIMUM layer among the primitives that
// cover it, 0 on the background, and there is no depth test anywhere.  rgb = palette[layer].
//
// PROJECT.  Every point is p' = p - offset, one fp32 subtraction per axis, with offset = (traj_x[i], MINS_y, traj_z[i]) and p the
// joint, or (MINS|MAXS_x, MINS_y, MINS|MAXS_z) for a corner, or (traj_x[j], MINS_y, traj_z[j]) for a trail point (so y' is exactly 0
// for both).  With S the fp32 4x4 screen matrix, h_k = fmaf(S[k][0], x', fmaf(S[k][1], y', fmaf(S[k][2], z', S[k][3]))) for the rows
// k = 0, 1, 3 (row 2, the depth, is not used: nothing is depth tested), sx = h_0 / h_3 and sy = h_1 / h_3 in correctly rounded fp32
// division, snapped to 4 sub-pixel bits: X = floor(16 sx + 0.5), Y likewise, as int32, row 0 on top.  The point is invalid -- both
// coordinates INT32_MIN -- when a component of p', h_0, h_1 or h_3 is not finite, when h_3 <= 0, or when |X| or |Y| exceeds the guard
// band of 8192 px = 2^17 units.  A primitive with an invalid vertex is dropped; nothing else is.
//
// SEGMENT COVERAGE.  Pixel (x, y) has the centre P = (16 x + 8, 16 y + 8).  A line of width_px pixels has the radius
// R = max(12, floor(8 width_px + 0.5)) units, at most 512 (12 units exceed sqrt(2)/2 px, so a capsule always covers a connected run
// of pixels).  For the segment A -> B, with d = B - A, e = P - A, dd = d . d, t = e . d, all int64, exactly one rule applies:
//   t <= 0     covered iff e . e <= R^2
//   t >= dd    covered iff |P - B|^2 <= R^2
//   otherwise  covered iff cross^2 <= R^2 dd, cross = d_x e_y - d_y e_x.
// |d|, |e| < 2^19 per component, so dd, t and cross stay below 2^39 and R^2 dd below 2^56: |cross| >= 2^28 decides "not covered"
// without the product, and everything else fits int64.  A == B is a disc.
//
// PLANE TRIANGLES.  int64 edge functions and the top-left fill rule exactly as mc_render.hip defines them, at 16 units per pixel:
// E_ab(P) = (bx - ax)(Py - ay) - (by - ay)(Px - ax); w0 = E_12, w1 = E_20, w2 = E_01; a sample is covered when the three w have the sign
// of the area, or are 0 on an edge that is top or left in the orientation that makes the inside positive.  No culling; zero area is
// dropped.
//
// Three kinds of launch per chunk of frames, all on one stream, no atomics of any kind:
//   stats_k    one block per sequence that has a frame in the chunk: MINS / MAXS by a tree of fminf / fmaxf (exact and order-free),
//              written into the record of each of the sequence's frames in the chunk, with the sequence's first row.
//   project_k  one thread per (frame, point): J joints, 4 corners and max_trail trail points -- the trail moves with traj[i], so it is
//              projected again for every frame -- snapped into the work buffer (and the optional outputs).
//   gather_k   one block per (frame, tile of 64 x 16 pixels), 4 pixels in a row per thread.  The frame's primitives pass through LDS
//              256 at a time: a thread builds one, tests its box (grown by R) against the tile's pixel centres, and each wave packs
//              its survivors with a ballot; then every thread resolves its 4 pixels against the survivors and keeps the maximum
//              layer.  rgb and layer are written once, directly: no visibility buffer.
// A frame depends on its sequence and on nothing else, so the result does not depend on the chunking, and two runs give the same bits.
#include "mc_common.h"
#include "../../include/motioncraft_amd.h"
#include <algorithm>
#include <limits.h>
#include <math.h>
#include <new>
#include <vector>

namespace {

constexpr int GUARD = 1 << 17;                 // |snapped coordinate| <= 8192 px
constexpr int INVALID = INT_MIN;
constexpr int MIN_R = MC_SKELETON_MIN_RADIUS, MAX_R = MC_SKELETON_MAX_RADIUS;
constexpr int MAX_SIZE = MC_SKELETON_MAX_SIZE;
constexpr int TILE_W = 64, TILE_H = 16;        // 256 threads x 4 pixels in a row; 8.3 KB of LDS, so LDS never bounds the occupancy
constexpr int STAGE = 256;                     // primitives staged per pass: one per thread

struct Info {                                  // per frame of the chunk: its sequence's statistics and first row
    float mins[3], maxs[3];
    int seq_begin, pad;
};
static_assert(sizeof(Info) == 32, "Info is the 32-byte record of the work layout");

struct Screen {
    float S[16];
};
struct Prim {                                  // R >= 0: the capsule a -> b; R < 0: the triangle a, b, c
    int ax, ay, bx, by, cx, cy, R, layer;
};

// the radius of a line of width_px pixels, in units; 0 when width_px is no usable width
int radius_units(float width_px) {
    if (!(width_px > 0.f) || !isfinite(width_px)) return 0;
    const double r = floor(8.0 * (double)width_px + 0.5);
    if (r > MAX_R) return 0;
    return std::max(MIN_R, (int)r);
}

__global__ __launch_bounds__(256) void stats_k(const float* __restrict__ joints, long row0, long row1, int J, long f0, long f1,
                                               Info* __restrict__ info, float* __restrict__ stats_out) {
    __shared__ float lo[3][256], hi[3][256];
    const int t = threadIdx.x;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    const float* base = joints + row0 * J * 3;
    const long count = (row1 - row0) * J;                      // points of the sequence
    for (long i = t; i < count; i += 256)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = base[3 * i + a];
            if (isfinite(v)) mn[a] = fminf(mn[a], v), mx[a] = fmaxf(mx[a], v);
        }
#pragma unroll
    for (int a = 0; a < 3; ++a) lo[a][t] = mn[a], hi[a][t] = mx[a];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s)
#pragma unroll
            for (int a = 0; a < 3; ++a) lo[a][t] = fminf(lo[a][t], lo[a][t + s]), hi[a][t] = fmaxf(hi[a][t], hi[a][t + s]);
        __syncthreads();
    }
    if (t < 3 && stats_out) stats_out[t] = lo[t][0], stats_out[3 + t] = hi[t][0];
    for (long g = max(row0, f0) + t; g < min(row1, f1); g += 256) {
        Info in;
#pragma unroll
        for (int a = 0; a < 3; ++a) in.mins[a] = lo[a][0], in.maxs[a] = hi[a][0];
        in.seq_begin = (int)row0, in.pad = 0;
        info[g - f0] = in;
    }
}

__device__ __forceinline__ int2 project(const Screen& sc, float px, float py, float pz, float ox, float oy, float oz) {
    const float x = px - ox, y = py - oy, z = pz - oz;
    const float* S = sc.S;
    const float hx = fmaf(S[0], x, fmaf(S[1], y, fmaf(S[2], z, S[3])));
    const float hy = fmaf(S[4], x, fmaf(S[5], y, fmaf(S[6], z, S[7])));
    const float hw = fmaf(S[12], x, fmaf(S[13], y, fmaf(S[14], z, S[15])));
    const float sx = __fdiv_rn(hx, hw), sy = __fdiv_rn(hy, hw);
    const float fx = floorf(fmaf(16.f, sx, 0.5f)), fy = floorf(fmaf(16.f, sy, 0.5f));
    const bool ok = isfinite(x) && isfinite(y) && isfinite(z) && isfinite(hx) && isfinite(hy) && isfinite(hw) && hw > 0.f &&
                    fabsf(fx) <= (float)GUARD && fabsf(fy) <= (float)GUARD;        // false for NaN
    return ok ? make_int2((int)fx, (int)fy) : make_int2(INVALID, INVALID);
}

// points of one frame: [0, J) joints, [J, J + 4) the plane's corners, [J + 4, J + 4 + T) trail points
__global__ __launch_bounds__(256) void project_k(const float* __restrict__ joints, long f0, long count, int J, int T, Screen sc,
                                                 const Info* __restrict__ info, int2* __restrict__ pts, int2* __restrict__ screen_out,
                                                 int2* __restrict__ trail_out, float* __restrict__ traj_out) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= count) return;
    const int P = J + 4 + T;
    const long fl = idx / P, g = f0 + fl;
    const int k = (int)(idx - fl * P);
    const Info in = info[fl];
    const float* root = joints + g * J * 3;
    const float ox = root[0], oy = in.mins[1], oz = root[2];
    float px = 0.f, py = oy, pz = 0.f;
    bool live = true;
    if (k < J) {
        px = root[3 * k], py = root[3 * k + 1], pz = root[3 * k + 2];
        if (k == 0 && traj_out) traj_out[2 * g] = ox, traj_out[2 * g + 1] = oz;
    } else if (k < J + 4) {
        const int q = k - J;
        px = q < 2 ? in.mins[0] : in.maxs[0];
        pz = (q == 1 || q == 2) ? in.maxs[2] : in.mins[2];
    } else {
        const long i = g - in.seq_begin, j = k - J - 4;
        live = i >= 2 && j < i;
        if (live) {
            const float* r = joints + (in.seq_begin + j) * J * 3;
            px = r[0], pz = r[2];
        }
    }
    const int2 s = live ? project(sc, px, py, pz, ox, oy, oz) : make_int2(INVALID, INVALID);
    pts[idx] = s;
    if (k < J + 4) {
        if (screen_out) screen_out[g * (J + 4) + k] = s;
    } else if (trail_out) {
        trail_out[g * T + (k - J - 4)] = s;
    }
}

__device__ __forceinline__ long edge(long ax, long ay, long bx, long by, long px, long py) { return (bx - ax) * (py - ay) - (by - ay) * (px - ax); }
__device__ __forceinline__ long edge_bias(long ax, long ay, long bx, long by, long sign) {
    const long dx = (bx - ax) * sign, dy = (by - ay) * sign;
    return (dy < 0 || (dy == 0 && dx > 0)) ? 0 : -1;
}

__device__ __forceinline__ bool covers(const Prim& q, int px, int py) {
    if (q.R >= 0) {
        const long dx = q.bx - q.ax, dy = q.by - q.ay, ex = px - q.ax, ey = py - q.ay;
        const long dd = dx * dx + dy * dy, t = ex * dx + ey * dy, r2 = (long)q.R * q.R;
        if (t <= 0) return ex * ex + ey * ey <= r2;
        if (t >= dd) {
            const long fx = px - q.bx, fy = py - q.by;
            return fx * fx + fy * fy <= r2;
        }
        const long cr = dx * ey - dy * ex, a = cr < 0 ? -cr : cr;
        return a < (1L << 28) && a * a <= r2 * dd;
    }
    const long area = edge(q.ax, q.ay, q.bx, q.by, q.cx, q.cy);
    if (area == 0) return false;
    const long sign = area > 0 ? 1 : -1;
    const long w0 = edge(q.bx, q.by, q.cx, q.cy, px, py), w1 = edge(q.cx, q.cy, q.ax, q.ay, px, py), w2 = edge(q.ax, q.ay, q.bx, q.by, px, py);
    return sign * w0 + edge_bias(q.bx, q.by, q.cx, q.cy, sign) >= 0 && sign * w1 + edge_bias(q.cx, q.cy, q.ax, q.ay, sign) >= 0 &&
           sign * w2 + edge_bias(q.ax, q.ay, q.bx, q.by, sign) >= 0;
}

struct Dims {
    int W, H, J, T, nseg, tiles_x, tiles_y, trail_R;
};

__global__ __launch_bounds__(256) void gather_k(long f0, Dims d, const unsigned* __restrict__ palette, const Info* __restrict__ info,
                                                const int2* __restrict__ pts, const int4* __restrict__ segs, uint8_t* __restrict__ rgb,
                                                uint8_t* __restrict__ layer_out) {
    __shared__ Prim list[4][64];
    __shared__ int kept[4];
    __shared__ unsigned pal_s[MC_SKELETON_MAX_LAYERS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int tiles = d.tiles_x * d.tiles_y;
    const long fl = blockIdx.x / tiles, g = f0 + fl;
    const int tile = (int)(blockIdx.x - fl * tiles), ty = tile / d.tiles_x, tx = tile - ty * d.tiles_x;
    const int x0 = tx * TILE_W, y0 = ty * TILE_H, x1 = min(x0 + TILE_W, d.W) - 1, y1 = min(y0 + TILE_H, d.H) - 1;
    const int cx0 = 16 * x0 + 8, cx1 = 16 * x1 + 8, cy0 = 16 * y0 + 8, cy1 = 16 * y1 + 8;      // the tile's first and last pixel centres
    const int P = d.J + 4 + d.T;
    const int2* fp = pts + fl * P;
    const long i = g - info[fl].seq_begin;
    const int ntrail = i >= 2 ? (int)(i - 1) : 0;
    const int nprim = 2 + ntrail + d.nseg;
    const int row = y0 + (tid >> 4), col = x0 + 4 * (tid & 15);
    const int py = 16 * row + 8;
    int best[4] = {0, 0, 0, 0};
    if (tid < MC_SKELETON_MAX_LAYERS) pal_s[tid] = palette[tid];       // read after the barriers below: nprim >= 2
    for (int base = 0; base < nprim; base += STAGE) {
        const int q = base + tid;
        Prim pr;
        bool keep = false;
        if (q < nprim) {
            int2 a, b, c;
            if (q < 2) {
                a = fp[d.J], b = fp[d.J + 1 + q], c = fp[d.J + 2 + q];
                pr.R = -1, pr.layer = 1;
            } else if (q < 2 + ntrail) {
                a = fp[d.J + 4 + (q - 2)], b = fp[d.J + 4 + (q - 1)], c = b;
                pr.R = d.trail_R, pr.layer = 2;
            } else {
                const int4 s = segs[q - 2 - ntrail];
                a = fp[s.x], b = fp[s.y], c = b;
                pr.R = s.z, pr.layer = s.w;
            }
            pr.ax = a.x, pr.ay = a.y, pr.bx = b.x, pr.by = b.y, pr.cx = c.x, pr.cy = c.y;
            if (a.x != INVALID && b.x != INVALID && c.x != INVALID) {
                const int grow = max(pr.R, 0);
                keep = max(a.x, max(b.x, c.x)) + grow >= cx0 && min(a.x, min(b.x, c.x)) - grow <= cx1 &&
                       max(a.y, max(b.y, c.y)) + grow >= cy0 && min(a.y, min(b.y, c.y)) - grow <= cy1;
            }
        }
        const unsigned long long mask = __ballot(keep);
        if (keep) list[wave][__popcll(mask & ((1ull << lane) - 1))] = pr;
        if (lane == 0) kept[wave] = __popcll(mask);
        __syncthreads();
        for (int w = 0; w < 4; ++w)
            for (int k = 0; k < kept[w]; ++k) {
                const Prim pr2 = list[w][k];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (pr2.layer > best[j] && covers(pr2, 16 * (col + j) + 8, py)) best[j] = pr2.layer;
            }
        __syncthreads();
    }
    if (row >= d.H || col >= d.W) return;
    const long pix = (g * d.H + row) * d.W + col;
    unsigned c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = pal_s[best[j]];
    if ((d.W & 3) == 0) {                                      // col and pix are multiples of 4: 12 bytes = three dword stores
        unsigned* o = (unsigned*)(rgb + 3 * pix);
        o[0] = c[0] | (c[1] << 24);
        o[1] = (c[1] >> 8) | (c[2] << 16);
        o[2] = (c[2] >> 16) | (c[3] << 8);
        if (layer_out) *(unsigned*)(layer_out + pix) = (unsigned)best[0] | (best[1] << 8) | (best[2] << 16) | ((unsigned)best[3] << 24);
    } else {
        for (int j = 0; j < 4 && col + j < d.W; ++j) {
            uint8_t* o = rgb + 3 * (pix + j);
            o[0] = (uint8_t)c[j], o[1] = (uint8_t)(c[j] >> 8), o[2] = (uint8_t)(c[j] >> 16);
            if (layer_out) layer_out[pix + j] = (uint8_t)best[j];
        }
    }
}

}  // namespace

struct mc_skeleton {
    int J = 0, nseg = 0, trail_R = 0;
    int4* segs = nullptr;                      // [nseg]: joint a, joint b, R, layer
    unsigned* palette = nullptr;               // [MC_SKELETON_MAX_LAYERS] 0x00BBGGRR
    ~mc_skeleton() {
        (void)hipFree(segs);
        (void)hipFree(palette);
    }
};

extern "C" int mc_skeleton_create(const int32_t* chain_joints_host, const int32_t* chain_start_host, int32_t num_chains, int32_t num_joints,
                                  const float* chain_width_px_host, float trail_width_px, const uint8_t* palette_host, mc_skeleton** out) {
    MC_REQUIRE(chain_joints_host && chain_start_host && chain_width_px_host && palette_host && out, "skeleton: null argument");
    MC_REQUIRE(num_chains >= 1 && num_chains <= MC_SKELETON_MAX_LAYERS - 3, "skeleton: num_chains=%d (1..%d: layers are 3 + chain < %d)", num_chains,
               MC_SKELETON_MAX_LAYERS - 3, MC_SKELETON_MAX_LAYERS);
    MC_REQUIRE(num_joints >= 1 && num_joints <= 65536, "skeleton: num_joints=%d (1..65536)", num_joints);
    MC_REQUIRE(chain_start_host[0] == 0, "skeleton: chain_start[0] = %d, expected 0", chain_start_host[0]);
    const int trail_R = radius_units(trail_width_px);
    MC_REQUIRE(trail_R > 0, "skeleton: trail_width_px=%g (positive, at most %d px)", (double)trail_width_px, MAX_R / 8);
    std::vector<int4> segs;
    for (int c = 0; c < num_chains; ++c) {
        const int b = chain_start_host[c], e = chain_start_host[c + 1];
        MC_REQUIRE(e - b >= 2 && e - b <= 65536, "skeleton: chain %d holds %d joints (2..65536)", c, e - b);
        const int R = radius_units(chain_width_px_host[c]);
        MC_REQUIRE(R > 0, "skeleton: chain %d has width_px=%g (positive, at most %d px)", c, (double)chain_width_px_host[c], MAX_R / 8);
        for (int k = b; k < e; ++k)
            MC_REQUIRE(chain_joints_host[k] >= 0 && chain_joints_host[k] < num_joints, "skeleton: chain %d names joint %d of %d", c,
                       chain_joints_host[k], num_joints);
        for (int k = b; k + 1 < e; ++k) segs.push_back(make_int4(chain_joints_host[k], chain_joints_host[k + 1], R, 3 + c));
    }
    unsigned pal[MC_SKELETON_MAX_LAYERS] = {};
    for (int l = 0; l < 3 + num_chains; ++l)
        pal[l] = (unsigned)palette_host[3 * l] | ((unsigned)palette_host[3 * l + 1] << 8) | ((unsigned)palette_host[3 * l + 2] << 16);
    mc_skeleton* h = new (std::nothrow) mc_skeleton;
    MC_REQUIRE(h, "skeleton: out of host memory");
    h->J = num_joints, h->nseg = (int)segs.size(), h->trail_R = trail_R;
    auto upload = [&]() -> int {
        MC_HIP(hipMalloc((void**)&h->segs, segs.size() * sizeof(int4)));
        MC_HIP(hipMemcpy(h->segs, segs.data(), segs.size() * sizeof(int4), hipMemcpyHostToDevice));
        MC_HIP(hipMalloc((void**)&h->palette, sizeof(pal)));
        MC_HIP(hipMemcpy(h->palette, pal, sizeof(pal), hipMemcpyHostToDevice));
        return MC_OK;
    };
    if (const int rc = upload()) {
        delete h;
        return rc;
    }
    *out = h;
    return MC_OK;
}

extern "C" void mc_skeleton_destroy(mc_skeleton* h) { delete h; }

static bool skeleton_size_ok(int32_t width, int32_t height) { return width >= 1 && height >= 1 && width <= MAX_SIZE && height <= MAX_SIZE; }
// bytes one frame of the chunk takes: its record and its J + 4 + max_trail snapped points
static long frame_bytes(const mc_skeleton* h, long max_trail) { return (long)sizeof(Info) + 8 * (h->J + 4 + max_trail); }

extern "C" int64_t mc_skeleton_work_bytes(const mc_skeleton* h, int32_t n_frames, int32_t max_trail, int32_t width, int32_t height) {
    if (!h || n_frames < 1 || max_trail < 0 || !skeleton_size_ok(width, height)) return -1;
    return n_frames * frame_bytes(h, max_trail);
}

extern "C" int mc_skeleton_frames(mc_skeleton* h, const float* joints_dev, const int32_t* seq_start_host, int32_t num_seqs,
                                  const mc_skeleton_params* p, void* work_dev, int64_t work_bytes, uint8_t* rgb_out_dev, uint8_t* layer_out_dev,
                                  int32_t* screen_out_dev, int32_t* trail_screen_out_dev, float* stats_out_dev, float* traj_out_dev, void* stream) {
    MC_REQUIRE(h && seq_start_host && p, "skeleton: null argument");
    MC_REQUIRE(num_seqs >= 0, "skeleton: num_seqs=%d", num_seqs);
    MC_REQUIRE(seq_start_host[0] == 0, "skeleton: seq_start[0] = %d, expected 0", seq_start_host[0]);
    long longest = 0;
    for (int s = 0; s < num_seqs; ++s) {
        MC_REQUIRE(seq_start_host[s + 1] >= seq_start_host[s], "skeleton: seq_start decreases at sequence %d", s);
        longest = std::max(longest, (long)seq_start_host[s + 1] - seq_start_host[s]);
    }
    const long n = seq_start_host[num_seqs];
    MC_REQUIRE(skeleton_size_ok(p->width, p->height), "skeleton: width=%d height=%d (1..%d each)", p->width, p->height, MAX_SIZE);
    for (int k = 0; k < 16; ++k) MC_REQUIRE(isfinite(p->screen[k]), "skeleton: screen[%d] is not finite", k);
    if (n == 0) return MC_OK;
    MC_REQUIRE(joints_dev && work_dev && rgb_out_dev, "skeleton: null argument");
    MC_REQUIRE(((uintptr_t)work_dev & 15) == 0 && ((uintptr_t)rgb_out_dev & 3) == 0 && ((uintptr_t)layer_out_dev & 3) == 0 &&
                   ((uintptr_t)joints_dev & 3) == 0,
               "skeleton: work must be 16-byte, rgb_out, layer_out and joints 4-byte aligned");
    const long W = p->width, H = p->height, J = h->J, T = longest, P = J + 4 + T;
    const long per = frame_bytes(h, T);
    MC_REQUIRE(work_bytes >= per, "skeleton: work_bytes=%ld, one frame with a trail of %ld points needs %ld", (long)work_bytes, T, per);
    const long tiles_x = cdiv(W, TILE_W), tiles_y = cdiv(H, TILE_H), tiles = tiles_x * tiles_y;
    const long cap = std::min((long)work_bytes / per, (long)INT_MAX / std::max(P, tiles));      // what one launch indexes
    hipStream_t st = (hipStream_t)stream;
    Info* info = (Info*)work_dev;
    int2* pts = (int2*)((char*)work_dev + cap * (long)sizeof(Info));
    Screen sc;
    for (int k = 0; k < 16; ++k) sc.S[k] = p->screen[k];
    const Dims d = {(int)W, (int)H, (int)J, (int)T, h->nseg, (int)tiles_x, (int)tiles_y, h->trail_R};
    int s = 0;                                 // the first sequence that may reach into the chunk
    for (long f0 = 0; f0 < n; f0 += cap) {
        const long c = std::min(cap, n - f0), f1 = f0 + c;
        while (seq_start_host[s + 1] <= f0) ++s;
        for (int q = s; q < num_seqs && seq_start_host[q] < f1; ++q) {
            if (seq_start_host[q + 1] == seq_start_host[q]) continue;
            hipLaunchKernelGGL(stats_k, dim3(1), dim3(256), 0, st, joints_dev, (long)seq_start_host[q], (long)seq_start_host[q + 1], (int)J, f0, f1,
                               info, stats_out_dev ? stats_out_dev + 6 * q : nullptr);
            MC_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(project_k, dim3(cdiv(c * P, 256)), dim3(256), 0, st, joints_dev, f0, c * P, (int)J, (int)T, sc, info, pts,
                           (int2*)screen_out_dev, (int2*)trail_screen_out_dev, traj_out_dev);
        MC_LAUNCH_CHECK();
        hipLaunchKernelGGL(gather_k, dim3((unsigned)(c * tiles)), dim3(256), 0, st, f0, d, h->palette, info, pts, h->segs, rgb_out_dev, layer_out_dev);
        MC_LAUNCH_CHECK();
    }
    return MC_OK;
}
