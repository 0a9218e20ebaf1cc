// Baseline JPEG encoder: uint8 RGB frames [n,H,W,3] in HBM, as mc_render_frames and mc_skeleton_frames leave them -> n complete JFIF
// files (SOI ... EOI) back to back in one device byte buffer, with their offsets.  It stands where the reference runs two ffmpeg child
// processes (convert_img_to_mp4 / add_audio_to_video, mogen/datasets/EMAGE_2024/utils/media.py:4-33): video.AviWriter wraps the files into a
// Motion-JPEG AVI, so rendered frames never cross PCIe uncompressed.  Integer arithmetic only: the byte stream is a definition, restated
// in numpy in tests/jpeg_ref.py and compared byte for byte.
//
// FORMAT.  Baseline sequential DCT (SOF0), 8 bit, components Y / Cb / Cr with ids 1 / 2 / 3, JFIF 1.01 APP0 (no density).  Subsampling
// 4:2:0 (MCU 16x16: Y00 Y01 Y10 Y11 Cb Cr) or 4:4:4 (MCU 8x8: Y Cb Cr).  The Annex K quantisation tables scaled by the IJG rule
// (scale = 5000 / q below 50, 200 - 2 q from 50, integer division; (t scale + 50) / 100 clamped to 1..255), one DQT segment each; the four
// Annex K Huffman tables, one DHT segment each, in every frame; DRI with one restart interval per MCU ROW, the marker after row r is
// RST(r mod 8), the last row is followed by EOI.  Every interval starts its DC predictions at 0 and is padded with 1-bits to a byte, so
// MCU rows are independent and the entropy coder runs one workgroup per row.  A frame whose size is no multiple of the MCU is padded by
// replicating its last column and row: pixel (x, y) of the padded frame is pixel (min(x, W - 1), min(y, H - 1)).  SOF0 has the true size.
//
// ARITHMETIC (>> is the arithmetic shift: floor).
//   colour    Y  = (19595 R + 38470 G +  7471 B + 32768) >> 16
//             Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
//             Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16        all in 0..255, sums below 2^25
//   4:2:0     chroma sample = (a + b + c + d + 2) >> 2 over the 2x2 Cb (Cr) values of the padded frame
//   shift     x = sample - 128, in -128..127
//   DCT       T[k][n] = round(2^12 s_k cos((2 n + 1) k pi / 16)), s_0 = sqrt(1/8), s_k = 1/2 (the table below; |T| <= 2009).
//             row pass     R[y][u] = (sum_x T[u][x] x[y][x] + 256) >> 9      3 fractional bits; |sum| <= 128 * 8 * 2009 < 2^21, |R| < 2^12
//             column pass  C[v][u] = sum_y T[v][y] R[y][u]                   15 fractional bits; |C| <= 8 * 2009 * 2^12 < 2^27
//   quantise  with D = Q[v][u] << 15 (Q <= 255, D < 2^23): q = sign(C) ((|C| + (D >> 1)) / D), round half away from zero; < 2^28 in int32
//   order     the block's 64 values in zigzag order, int16
// A DC value is at most 8 * 128 = 1024 in magnitude (a difference 2048: category <= 11 with a code of <= 11 bits), an AC value at most
// 128 (sum_n |cos((2 n + 1) pi / 16)| / 2)^2 = 841 plus rounding (category <= 10): a block takes at most 22 + 63 * (16 + 10) = 1660 bits,
// 52 words.  Whatever the input, the categories stay below 16, so no table index leaves its table.
//
// Four kinds of launch per chunk of frames, on one stream:
//   jpeg_blocks_k   one wave per MCU, four MCUs of a row per workgroup: the RGB tile goes through LDS, then colour, chroma mean, the two
//                   DCT passes with the LDS transpose between them, quantisation, zigzag -> int16 coefficients.
//   jpeg_entropy_k  one workgroup per restart interval, one thread per block, 256 blocks at a time through LDS.  Pass A: every block
//                   derives its DC difference from its predecessor of the same component and counts its bits; the counts are scanned
//                   across the interval.  The words the interval needs are zeroed.  Pass B: every block places its bits at its bit
//                   offset; the first and last word of a block may be shared with its neighbours and are merged with an atomic OR, which
//                   commutes, so the result has no order dependence; the words between belong to the block alone.  Pass C counts the
//                   0xFF bytes: the interval's length after stuffing.
//   jpeg_scan_k     one workgroup: interval lengths + header + 2-byte markers scanned over the chunk, continuing from the offset the
//                   chunk before left; writes every interval's position and the frame offsets.
//   jpeg_pack_k     one workgroup per interval: copies the header in front of a frame's first interval, inserts 0x00 after every 0xFF
//                   (count, scan, write) and appends RSTm or EOI.
// A frame depends on nothing but its pixels, so the result does not depend on the chunking, and two runs give the same bytes.
#include "mc_common.h"
#include "../../include/motioncraft_amd.h"
#include <algorithm>
#include <limits.h>
#include <new>
#include <vector>

namespace {

constexpr int BLOCK_WORDS = 52;                // 1660 bits
constexpr int BLOCK_BYTES = 4 * BLOCK_WORDS;   // of bit buffer per block; twice that after stuffing
constexpr int TILE = 256;                      // blocks of an interval in LDS at a time: one per thread
constexpr int TILE_STRIDE = 66;                // int16 per staged block: 33 dwords, so 32 lanes read 32 banks
constexpr long MAX_GRID = (1L << 24) - 1;      // workgroups of 256 threads in one launch: gridDim.x * blockDim.x stays below 2^32

__constant__ int c_T[64] = {1448, 1448, 1448, 1448,  1448,  1448,  1448,  1448,  2009, 1703,  1138,  400,   -400,  -1138, -1703, -2009,
                            1892, 784,  -784, -1892, -1892, -784,  784,   1892,  1703, -400,  -2009, -1138, 1138,  2009,  400,   -1703,
                            1448, -1448, -1448, 1448, 1448, -1448, -1448, 1448,  1138, -2009, 400,   1703,  -1703, -400,  2009,  -1138,
                            784,  -1892, 1892, -784, -784,  1892,  -1892, 784,   400,  -1138, 1703,  -2009, 2009,  -1703, 1138,  -400};
// the natural (row-major) index of zigzag position k
const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                            35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Annex K, natural order
const uint8_t LUMA_Q[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                            18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t CHROMA_Q[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                              99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
const uint8_t DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const uint8_t AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1,
     0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a,
     0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3,
     0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1,
     0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
     0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca,
     0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

struct Geo {
    int W, H;
    int M, bpm;                // MCU side in pixels (16 or 8), blocks per MCU (6 or 3)
    int mcols, mrows;          // MCUs per row = per restart interval; MCU rows = intervals per frame
    int nb;                    // blocks per interval
    int hdr_len;
    long blocks;               // per frame
    long ibytes;               // bit buffer of one interval, a multiple of 256: no two intervals share a cache line
};

// inclusive-to-exclusive scan of one int per thread of a 256-thread workgroup; `sh` = 4 ints of LDS, reusable after the call
__device__ __forceinline__ int block_excl_scan(int v, int* sh, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += sh[w];
    total = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return before + inc - v;
}

__global__ __launch_bounds__(256) void jpeg_blocks_k(const uint8_t* __restrict__ rgb, long f0, Geo g, const int* __restrict__ qtab,
                                                     const uint8_t* __restrict__ zpos, int16_t* __restrict__ coef) {
    __shared__ uint8_t raw[4][768];            // the MCU's pixels as they lie in the frame, edges replicated
    __shared__ int pix[4][3][256];             // Y - 128, Cb, Cr
    __shared__ int blk[4][6][64], mid[4][6][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int groups = (g.mcols + 3) >> 2;
    const long fl = blockIdx.x / (g.mrows * groups);
    const int rem = (int)(blockIdx.x - fl * (g.mrows * groups));
    const int my = rem / groups, mx = (rem - my * groups) * 4 + wave;
    const bool live = mx < g.mcols;            // a dead wave keeps the barriers company
    const int M = g.M, MM = M * M, ms = M == 16 ? 4 : 3;
    const uint8_t* src = rgb + (f0 + fl) * g.H * g.W * 3;
    if (live)
        for (int i = lane; i < 3 * MM; i += 64) {
            const int y = i / (3 * M), o = i - y * 3 * M, x = o / 3, ch = o - 3 * x;
            const int sy = min(my * M + y, g.H - 1), sx = min(mx * M + x, g.W - 1);
            raw[wave][i] = src[((long)sy * g.W + sx) * 3 + ch];
        }
    __syncthreads();
    if (live)
        for (int p = lane; p < MM; p += 64) {
            const int R = raw[wave][3 * p], G = raw[wave][3 * p + 1], B = raw[wave][3 * p + 2];
            pix[wave][0][p] = ((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128;
            pix[wave][1][p] = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
            pix[wave][2][p] = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
        }
    __syncthreads();
    const int r8 = lane >> 3, c8 = lane & 7;
    if (live) {
        if (M == 16) {
#pragma unroll
            for (int k = 0; k < 4; ++k) blk[wave][k][lane] = pix[wave][0][(8 * (k >> 1) + r8) << ms | (8 * (k & 1) + c8)];
            const int i = (2 * r8) << ms | (2 * c8);
#pragma unroll
            for (int c = 1; c < 3; ++c) {
                const int* q = pix[wave][c];
                blk[wave][3 + c][lane] = ((q[i] + q[i + 1] + q[i + 16] + q[i + 17] + 2) >> 2) - 128;
            }
        } else {
            blk[wave][0][lane] = pix[wave][0][lane];
            blk[wave][1][lane] = pix[wave][1][lane] - 128;
            blk[wave][2][lane] = pix[wave][2][lane] - 128;
        }
    }
    __syncthreads();
    if (live)
        for (int k = 0; k < g.bpm; ++k) {      // row pass: lane = (row y, frequency u)
            int s = 0;
#pragma unroll
            for (int x = 0; x < 8; ++x) s += c_T[c8 * 8 + x] * blk[wave][k][r8 * 8 + x];
            mid[wave][k][lane] = (s + 256) >> 9;
        }
    __syncthreads();
    if (live) {
        const long first = (fl * g.blocks + ((long)my * g.mcols + mx) * g.bpm) * 64;
        const int z = zpos[lane];
        for (int k = 0; k < g.bpm; ++k) {      // column pass: lane = (frequency v, frequency u)
            int s = 0;
#pragma unroll
            for (int y = 0; y < 8; ++y) s += c_T[r8 * 8 + y] * mid[wave][k][y * 8 + c8];
            const int D = qtab[(k >= g.bpm - 2 ? 64 : 0) + lane] << 15;
            const int q = (abs(s) + (D >> 1)) / D;
            coef[first + k * 64 + z] = (int16_t)(s < 0 ? -q : q);
        }
    }
}

// the bits of one block, in order, handed to `sink.put(code, length)` with length <= 26
template <class Sink>
__device__ __forceinline__ void code_block(const int16_t* c, int pred, const unsigned* dc, const unsigned* ac, Sink& sink) {
    auto value = [&](unsigned h, int v) {      // Huffman code of the category, then the value's bits
        const int a = abs(v), cat = a ? 32 - __clz(a) : 0;
        const unsigned e = h ? ac[(h - 1) << 4 | cat] : dc[cat];        // h = run + 1 for AC, 0 for DC
        sink.put((e >> 8) << cat | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << cat) - 1)), (int)(e & 255) + cat);
    };
    value(0, (int)c[0] - pred);
    int run = 0;
    for (int i = 1; i < 64; ++i) {
        const int v = c[i];
        if (v == 0) {
            ++run;
            continue;
        }
        for (; run > 15; run -= 16) sink.put(ac[0xF0] >> 8, (int)(ac[0xF0] & 255));      // ZRL
        value(run + 1, v);
        run = 0;
    }
    if (run) sink.put(ac[0] >> 8, (int)(ac[0] & 255));                                  // EOB
}

struct CountBits {
    int bits = 0;
    __device__ __forceinline__ void put(unsigned, int len) { bits += len; }
};

// MSB-first into 32-bit words: bit p of the interval is bit 31 - (p & 31) of word p >> 5
struct PlaceBits {
    unsigned* words;
    long w;
    unsigned long long acc = 0;
    int n;                                     // bits of acc not yet written; starts at the offset inside the first word
    bool first = true;
    __device__ PlaceBits(unsigned* words_, int bit) : words(words_), w(bit >> 5), n(bit & 31) {}
    __device__ __forceinline__ void put(unsigned code, int len) {
        acc = acc << len | code;
        n += len;
        if (n >= 32) {
            const unsigned v = (unsigned)(acc >> (n - 32));
            if (first) atomicOr(&words[w], v);                          // may hold the tail of the block before
            else words[w] = v;
            first = false, ++w, n -= 32;
        }
    }
    __device__ __forceinline__ void finish() {
        if (n > 0) atomicOr(&words[w], (unsigned)(acc << (32 - n)));   // may hold the head of the block after
    }
};

__global__ __launch_bounds__(256) void jpeg_entropy_k(Geo g, const unsigned* __restrict__ huff, const int16_t* __restrict__ coef,
                                                      int* __restrict__ bitoff, unsigned* __restrict__ bits, int2* __restrict__ lens) {
    __shared__ unsigned tab[4][256];           // (code << 8 | length): DC luma, DC chroma, AC luma, AC chroma
    __shared__ int tile[TILE * TILE_STRIDE / 2];
    __shared__ int sh[4];
    const int t = threadIdx.x;
    const long interval = blockIdx.x;          // frame of the chunk * mrows + MCU row
    const long ib = interval * g.nb;           // its first block in the chunk
    unsigned* words = bits + interval * (g.ibytes >> 2);
    for (int i = t; i < 4 * 256; i += 256) tab[0][i] = huff[i];

    auto stage = [&](int base, int nt) {       // coefficients of blocks base .. base + nt of the interval -> LDS
        __syncthreads();
        const int* src = (const int*)(coef + (ib + base) * 64);
        for (int e = t; e < nt * 32; e += 256) tile[(e >> 5) * (TILE_STRIDE / 2) + (e & 31)] = src[e];
        __syncthreads();
    };
    auto pred_of = [&](int j, int& chroma) {   // DC of block j's predecessor of the same component in scan order, 0 at the row's start
        const int k = j % g.bpm;
        chroma = k >= g.bpm - 2;
        const int back = (g.bpm == 6 && k >= 1 && k <= 3) ? 1 : (g.bpm == 6 && k == 0) ? 3 : g.bpm;
        return j - back >= 0 ? (int)coef[(ib + j - back) * 64] : 0;
    };

    int total = 0;
    for (int base = 0; base < g.nb; base += TILE) {                     // pass A
        const int nt = min(TILE, g.nb - base);
        stage(base, nt);
        CountBits cnt;
        if (t < nt) {
            int chroma;
            const int pred = pred_of(base + t, chroma);
            code_block((const int16_t*)tile + t * TILE_STRIDE, pred, tab[chroma], tab[2 + chroma], cnt);
        }
        int sum;
        const int off = block_excl_scan(cnt.bits, sh, sum);
        if (t < nt) bitoff[ib + base + t] = total + off;
        total += sum;
    }
    const int pad = -total & 7, nbytes = (total + pad) >> 3, nwords = (total + pad + 31) >> 5;
    for (int i = t; i < nwords; i += 256) words[i] = 0;
    __syncthreads();
    if (t == 0 && pad) atomicOr(&words[total >> 5], ((1u << pad) - 1) << (32 - pad - (total & 31)));
    for (int base = 0; base < g.nb; base += TILE) {                     // pass B
        const int nt = min(TILE, g.nb - base);
        stage(base, nt);
        if (t < nt) {
            int chroma;
            const int pred = pred_of(base + t, chroma);
            PlaceBits place(words, bitoff[ib + base + t]);
            code_block((const int16_t*)tile + t * TILE_STRIDE, pred, tab[chroma], tab[2 + chroma], place);
            place.finish();
        }
    }
    __syncthreads();
    int ff = 0;                                                         // pass C
    for (int i = t; i < nwords; i += 256) {
        const unsigned w = __hip_atomic_load(&words[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int k = 0; k < 4; ++k) ff += (4 * i + k < nbytes) && ((w >> (24 - 8 * k)) & 255) == 255;
    }
    int sum;
    block_excl_scan(ff, sh, sum);
    if (t == 0) lens[interval] = make_int2(nbytes + sum, nbytes);
}

__global__ __launch_bounds__(256) void jpeg_scan_k(Geo g, long f0, int frames, const int2* __restrict__ lens, long* __restrict__ pos,
                                                   long* __restrict__ offsets) {
    __shared__ long part[256];
    const int t = threadIdx.x;
    const long N = (long)frames * g.mrows, per = (N + 255) / 256, lo = min(N, t * per), hi = min(N, lo + per);
    auto bytes = [&](long i) { return (long)lens[i].x + 2 + (i % g.mrows == 0 ? g.hdr_len : 0); };     // the interval, its marker, the header
    long s = 0;
    for (long i = lo; i < hi; ++i) s += bytes(i);
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        long run = f0 ? offsets[f0] : 0;
        for (int k = 0; k < 256; ++k) {
            const long v = part[k];
            part[k] = run, run += v;
        }
        offsets[f0 + frames] = run;
    }
    __syncthreads();
    long run = part[t];
    for (long i = lo; i < hi; ++i) {
        pos[i] = run;
        if (i % g.mrows == 0) offsets[f0 + i / g.mrows] = run;
        run += bytes(i);
    }
}

__global__ __launch_bounds__(256) void jpeg_pack_k(Geo g, const uint8_t* __restrict__ hdr, const int2* __restrict__ lens,
                                                   const long* __restrict__ pos, const unsigned* __restrict__ bits, uint8_t* __restrict__ out) {
    __shared__ int sh[4];
    const int t = threadIdx.x;
    const long interval = blockIdx.x;
    const int row = (int)(interval % g.mrows);
    const unsigned* words = bits + interval * (g.ibytes >> 2);
    const int2 len = lens[interval];
    uint8_t* o = out + pos[interval];
    if (row == 0) {
        for (int i = t; i < g.hdr_len; i += 256) o[i] = hdr[i];
        o += g.hdr_len;
    }
    int shift = 0;                             // 0x00 bytes inserted so far
    for (int base = 0; base < len.y; base += 4 * 256) {
        const int b0 = base + 4 * t, valid = min(4, max(0, len.y - b0));
        const unsigned w = valid ? words[b0 >> 2] : 0;
        int ff = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) ff += k < valid && ((w >> (24 - 8 * k)) & 255) == 255;
        int sum;
        int at = b0 + shift + block_excl_scan(ff, sh, sum);
        for (int k = 0; k < valid; ++k) {
            const unsigned v = (w >> (24 - 8 * k)) & 255;
            o[at++] = (uint8_t)v;
            if (v == 255) o[at++] = 0;
        }
        shift += sum;
    }
    if (t == 0) o[len.x] = 0xFF, o[len.x + 1] = (uint8_t)(row + 1 < g.mrows ? 0xD0 + (row & 7) : 0xD9);
}

long align256(long v) { return (v + 255) & ~255L; }

// (code << 8 | length) per symbol from a DHT's counts and values (Annex C)
void huffman_codes(const uint8_t* counts, const uint8_t* vals, unsigned* out) {
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len, code <<= 1)
        for (int i = 0; i < counts[len - 1]; ++i) out[vals[k++]] = code++ << 8 | (unsigned)len;
}

}  // namespace

struct mc_mjpeg {
    Geo g{};
    long sec[5] = {};                          // bytes per frame of the work sections: lengths, positions, bit offsets, coefficients, bits
    int* qtab = nullptr;                       // [2][64] natural order
    uint8_t* zpos = nullptr;                   // [64] zigzag position of a natural index
    unsigned* huff = nullptr;                  // [4][256]
    uint8_t* hdr = nullptr;                    // [g.hdr_len]: SOI .. SOS
    ~mc_mjpeg() {
        (void)hipFree(qtab);
        (void)hipFree(zpos);
        (void)hipFree(huff);
        (void)hipFree(hdr);
    }
    long frame_work() const { return sec[0] + sec[1] + sec[2] + sec[3] + sec[4]; }
    long frame_max() const { return g.hdr_len + (long)g.mrows * (2L * BLOCK_BYTES * g.nb + 2); }
};

extern "C" int mc_mjpeg_create(int32_t width, int32_t height, int32_t quality, int32_t subsampling, mc_mjpeg** out) {
    MC_REQUIRE(out, "mjpeg: null argument");
    MC_REQUIRE(width >= 1 && height >= 1 && width <= MC_MJPEG_MAX_SIZE && height <= MC_MJPEG_MAX_SIZE, "mjpeg: width=%d height=%d (1..%d each)", width, height, MC_MJPEG_MAX_SIZE);
    MC_REQUIRE(quality >= 1 && quality <= 100, "mjpeg: quality=%d (1..100)", quality);
    MC_REQUIRE(subsampling == MC_MJPEG_420 || subsampling == MC_MJPEG_444, "mjpeg: subsampling=%d (MC_MJPEG_420 or MC_MJPEG_444)", subsampling);
    mc_mjpeg* h = new (std::nothrow) mc_mjpeg;
    MC_REQUIRE(h, "mjpeg: out of host memory");
    Geo& g = h->g;
    g.W = width, g.H = height;
    g.M = subsampling == MC_MJPEG_420 ? 16 : 8, g.bpm = subsampling == MC_MJPEG_420 ? 6 : 3;
    g.mcols = cdiv(width, g.M), g.mrows = cdiv(height, g.M);
    g.nb = g.mcols * g.bpm;
    g.blocks = (long)g.nb * g.mrows;
    g.ibytes = align256((long)g.nb * BLOCK_BYTES);

    int q[2][64];
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        q[0][i] = std::min(255, std::max(1, (LUMA_Q[i] * scale + 50) / 100));
        q[1][i] = std::min(255, std::max(1, (CHROMA_Q[i] * scale + 50) / 100));
    }
    uint8_t zpos[64];
    for (int k = 0; k < 64; ++k) zpos[ZIGZAG[k]] = (uint8_t)k;
    std::vector<unsigned> huff(4 * 256, 0u);
    for (int c = 0; c < 2; ++c) {
        huffman_codes(DC_BITS[c], DC_VALS, &huff[c * 256]);
        huffman_codes(AC_BITS[c], AC_VALS[c], &huff[(2 + c) * 256]);
    }

    std::vector<uint8_t> hd;
    auto put = [&](std::initializer_list<int> v) {
        for (int b : v) hd.push_back((uint8_t)b);
    };
    put({0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int c = 0; c < 2; ++c) {
        put({0xFF, 0xDB, 0, 67, c});
        for (int k = 0; k < 64; ++k) hd.push_back((uint8_t)q[c][ZIGZAG[k]]);
    }
    put({0xFF, 0xC0, 0, 17, 8, height >> 8, height & 255, width >> 8, width & 255, 3, 1, subsampling == MC_MJPEG_420 ? 0x22 : 0x11, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int c = 0; c < 2; ++c) {
        put({0xFF, 0xC4, 0, 2 + 1 + 16 + 12, c});
        hd.insert(hd.end(), DC_BITS[c], DC_BITS[c] + 16), hd.insert(hd.end(), DC_VALS, DC_VALS + 12);
        put({0xFF, 0xC4, 0, 2 + 1 + 16 + 162, 0x10 | c});
        hd.insert(hd.end(), AC_BITS[c], AC_BITS[c] + 16), hd.insert(hd.end(), AC_VALS[c], AC_VALS[c] + 162);
    }
    put({0xFF, 0xDD, 0, 4, g.mcols >> 8, g.mcols & 255});
    put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    g.hdr_len = (int)hd.size();

    h->sec[0] = align256(8L * g.mrows), h->sec[1] = align256(8L * g.mrows), h->sec[2] = align256(4 * g.blocks);
    h->sec[3] = align256(128 * g.blocks), h->sec[4] = g.mrows * g.ibytes;

    auto upload = [&]() -> int {
        MC_HIP(hipMalloc((void**)&h->qtab, sizeof(q)));
        MC_HIP(hipMemcpy(h->qtab, q, sizeof(q), hipMemcpyHostToDevice));
        MC_HIP(hipMalloc((void**)&h->zpos, sizeof(zpos)));
        MC_HIP(hipMemcpy(h->zpos, zpos, sizeof(zpos), hipMemcpyHostToDevice));
        MC_HIP(hipMalloc((void**)&h->huff, huff.size() * sizeof(unsigned)));
        MC_HIP(hipMemcpy(h->huff, huff.data(), huff.size() * sizeof(unsigned), hipMemcpyHostToDevice));
        MC_HIP(hipMalloc((void**)&h->hdr, hd.size()));
        MC_HIP(hipMemcpy(h->hdr, hd.data(), hd.size(), hipMemcpyHostToDevice));
        return MC_OK;
    };
    if (const int rc = upload()) {
        delete h;
        return rc;
    }
    *out = h;
    return MC_OK;
}

extern "C" void mc_mjpeg_destroy(mc_mjpeg* h) { delete h; }

extern "C" int64_t mc_mjpeg_work_bytes(const mc_mjpeg* h, int32_t frames) {
    if (!h || frames < 1) return -1;
    return frames * h->frame_work();
}

extern "C" int64_t mc_mjpeg_max_bytes(const mc_mjpeg* h, int32_t frames) {
    if (!h || frames < 0 || frames > LONG_MAX / h->frame_max()) return -1;
    return frames * h->frame_max();
}

extern "C" int mc_mjpeg_encode(mc_mjpeg* h, const uint8_t* rgb_dev, int32_t n, void* work_dev, int64_t work_bytes, uint8_t* out_dev,
                               int64_t out_capacity, int64_t* offsets_dev, void* stream) {
    MC_REQUIRE(h && rgb_dev && work_dev && out_dev && offsets_dev, "mjpeg: null argument");
    MC_REQUIRE(n >= 1, "mjpeg: n=%d frames", n);
    MC_REQUIRE(((uintptr_t)work_dev & 255) == 0 && ((uintptr_t)offsets_dev & 7) == 0, "mjpeg: work must be 256-byte, offsets 8-byte aligned");
    const Geo& g = h->g;
    const long per = h->frame_work(), bound = mc_mjpeg_max_bytes(h, n);
    MC_REQUIRE(work_bytes >= per, "mjpeg: work_bytes=%ld, one frame of %dx%d needs %ld", (long)work_bytes, g.W, g.H, per);
    MC_REQUIRE(bound >= 0 && out_capacity >= bound, "mjpeg: out_capacity=%ld, %d frames of %dx%d may take %ld bytes", (long)out_capacity, n, g.W,
               g.H, bound);
    const long groups = cdiv(g.mcols, 4);
    // frames per launch: what the scratch holds, and what keeps the largest grid, jpeg_blocks_k's c * mrows * groups, within MAX_GRID;
    // the entropy and pack grids, c * mrows, are no larger.  mrows * groups <= 2048 * 512 = 2^20, so at least 15 frames always fit.
    const long cap = std::min({(long)work_bytes / per, MAX_GRID / (g.mrows * groups), (long)n});
    char* w = (char*)work_dev;
    int2* lens = (int2*)w;
    long* pos = (long*)(w + cap * h->sec[0]);
    int* bitoff = (int*)(w + cap * (h->sec[0] + h->sec[1]));
    int16_t* coef = (int16_t*)(w + cap * (h->sec[0] + h->sec[1] + h->sec[2]));
    unsigned* bits = (unsigned*)(w + cap * (h->sec[0] + h->sec[1] + h->sec[2] + h->sec[3]));
    hipStream_t st = (hipStream_t)stream;
    for (long f0 = 0; f0 < n; f0 += cap) {
        const long c = std::min(cap, n - f0);
        hipLaunchKernelGGL(jpeg_blocks_k, dim3((unsigned)(c * g.mrows * groups)), dim3(256), 0, st, rgb_dev, f0, g, h->qtab, h->zpos, coef);
        MC_LAUNCH_CHECK();
        hipLaunchKernelGGL(jpeg_entropy_k, dim3((unsigned)(c * g.mrows)), dim3(256), 0, st, g, h->huff, coef, bitoff, bits, lens);
        MC_LAUNCH_CHECK();
        hipLaunchKernelGGL(jpeg_scan_k, dim3(1), dim3(256), 0, st, g, f0, (int)c, lens, pos, (long*)offsets_dev);
        MC_LAUNCH_CHECK();
        hipLaunchKernelGGL(jpeg_pack_k, dim3((unsigned)(c * g.mrows)), dim3(256), 0, st, g, h->hdr, lens, pos, bits, out_dev);
        MC_LAUNCH_CHECK();
    }
    return MC_OK;
}
