"""numpy / Python-int restatement of the baseline JPEG encoder ``mc_mjpeg_*`` (the header comment of csrc/mc_mjpeg.hip): the same integer
definitions written plainly -- one loop over blocks, one bit writer -- so that the device's byte stream can be held to equality.  Also the
images and the case table the host and device tests of ``video.py`` share.  Test infrastructure, like ``raster_ref.py``."""
import math

import numpy as np

# the natural (row-major) index of zigzag position k
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57,
          50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
# Annex K.1, natural order
LUMA_Q = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
          18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
CHROMA_Q = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
# Annex K.3: the number of codes of each length 1..16, then the symbols in code order
DC_BITS = [[0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]]
DC_VALS = list(range(12))
AC_BITS = [[0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]]
_TAIL = [16 * r + s for r in range(16) for s in range(1, 11)]           # every (run, size) symbol in ascending order
AC_VALS = [
    [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
     0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82],
    [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
     0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1]]
# both tables end with the symbols not named so far, in ascending order (the 16-bit codes)
AC_VALS = [head + [s for s in _TAIL if s not in head] for head in AC_VALS]
assert [len(v) for v in AC_VALS] == [162, 162] == [sum(b) for b in AC_BITS] and [sum(b) for b in DC_BITS] == [12, 12]

# T[k][n] = round(2^12 s_k cos((2 n + 1) k pi / 16)), s_0 = sqrt(1/8), s_k = 1/2
T = np.array([[1448, 1448, 1448, 1448, 1448, 1448, 1448, 1448], [2009, 1703, 1138, 400, -400, -1138, -1703, -2009],
              [1892, 784, -784, -1892, -1892, -784, 784, 1892], [1703, -400, -2009, -1138, 1138, 2009, 400, -1703],
              [1448, -1448, -1448, 1448, 1448, -1448, -1448, 1448], [1138, -2009, 400, 1703, -1703, -400, 2009, -1138],
              [784, -1892, 1892, -784, -784, 1892, -1892, 784], [400, -1138, 1703, -2009, 2009, -1703, 1138, -400]], np.int64)
assert all(T[k][n] == round(4096 * (math.sqrt(1 / 8) if k == 0 else 0.5) * math.cos((2 * n + 1) * k * math.pi / 16)) for k in range(8) for n in range(8))

SUBSAMPLINGS = ('4:2:0', '4:4:4')


def quant_tables(quality):
    """The IJG rule: [luma, chroma], natural order, each 1..255."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [[min(255, max(1, (t * scale + 50) // 100)) for t in table] for table in (LUMA_Q, CHROMA_Q)]


def huffman_codes(bits, vals):
    """symbol -> (code, length), Annex C."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


DC_CODES = [huffman_codes(DC_BITS[c], DC_VALS) for c in range(2)]
AC_CODES = [huffman_codes(AC_BITS[c], AC_VALS[c]) for c in range(2)]


def mcu_grid(W, H, subsampling):
    """(MCU side, MCUs per row, MCU rows)."""
    M = 16 if subsampling == '4:2:0' else 8
    return M, -(-W // M), -(-H // M)


def header(W, H, quality, subsampling):
    """SOI, JFIF APP0, two DQT, SOF0, four DHT, DRI (one MCU row), SOS."""
    M, mcols, _ = mcu_grid(W, H, subsampling)
    out = bytearray([0xFF, 0xD8, 0xFF, 0xE0, 0, 16]) + b'JFIF\0' + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0])
    for c, table in enumerate(quant_tables(quality)):
        out += bytes([0xFF, 0xDB, 0, 67, c] + [table[ZIGZAG[k]] for k in range(64)])
    out += bytes([0xFF, 0xC0, 0, 17, 8, H >> 8, H & 255, W >> 8, W & 255, 3, 1, 0x22 if M == 16 else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    for c in range(2):
        out += bytes([0xFF, 0xC4, 0, 31, c] + DC_BITS[c] + DC_VALS)
        out += bytes([0xFF, 0xC4, 0, 181, 0x10 | c] + AC_BITS[c] + AC_VALS[c])
    out += bytes([0xFF, 0xDD, 0, 4, mcols >> 8, mcols & 255])
    out += bytes([0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    return bytes(out)


def ycbcr(rgb):
    """The JFIF matrix in 16-bit fixed point; >> floors.  Three int64 planes in 0..255."""
    R, G, B = (rgb[..., c].astype(np.int64) for c in range(3))
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    return Y, Cb, Cr


def fdct_quantise(block, Q):
    """8x8 level-shifted samples, Q [64] natural order -> the 64 quantised values in zigzag order."""
    rows = (block @ T.T + 256) >> 9                    # rows[y][u] = (sum_x T[u][x] block[y][x] + 256) >> 9: 3 fractional bits
    C = (T @ rows).reshape(64)                         # C[v][u] = sum_y T[v][y] rows[y][u]: 15 fractional bits
    assert np.abs(block @ T.T).max() < 2 ** 21 and np.abs(C).max() < 2 ** 27
    D = np.asarray(Q, np.int64) << 15
    q = np.sign(C) * ((np.abs(C) + (D >> 1)) // D)     # round half away from zero
    return [int(v) for v in q[ZIGZAG]]


class BitWriter:
    """MSB first; ``finish`` pads with 1-bits to a byte and stuffs 0x00 after every 0xFF."""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, length):
        assert 0 <= code < 1 << length
        self.acc, self.n = self.acc << length | code, self.n + length

    def finish(self, stats=None):
        pad = -self.n % 8
        self.put((1 << pad) - 1, pad)
        raw = self.acc.to_bytes(self.n // 8, 'big')
        if stats is not None:
            stats['stuffed'] = stats.get('stuffed', 0) + raw.count(b'\xff')
            stats['longest'] = max(stats.get('longest', 0), len(raw))
        return raw.replace(b'\xff', b'\xff\x00')


def code_block(zz, pred, dc, ac, bw, stats=None):
    """One block's bits: DC category + bits of the difference, then (run, size) + bits per non-zero AC value, ZRL per 16 zeros in
    front of one, EOB when the block ends in zeros."""
    def value(v):
        cat = abs(v).bit_length()
        return cat, (v if v >= 0 else v - 1) & ((1 << cat) - 1)
    before = bw.n
    cat, extra = value(zz[0] - pred)
    assert cat <= 11
    bw.put(*dc[cat]), bw.put(extra, cat)
    run = 0
    for v in zz[1:]:
        if v == 0:
            run += 1
            continue
        while run > 15:
            bw.put(*ac[0xF0])
            run -= 16
            if stats is not None:
                stats['zrl'] = stats.get('zrl', 0) + 1
        cat, extra = value(v)
        assert cat <= 10
        bw.put(*ac[run << 4 | cat]), bw.put(extra, cat)
        run = 0
    if run:
        bw.put(*ac[0])
    assert bw.n - before <= 1660


def encode(rgb, quality=90, subsampling='4:2:0', stats=None):
    """uint8 [H, W, 3] -> the bytes of one JPEG file.  ``stats`` (a dict) counts ZRL symbols and stuffed bytes."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3 and subsampling in SUBSAMPLINGS and 1 <= quality <= 100
    H, W = rgb.shape[:2]
    M, mcols, mrows = mcu_grid(W, H, subsampling)
    padded = np.pad(rgb, ((0, mrows * M - H), (0, mcols * M - W), (0, 0)), mode='edge')       # the last column / row replicated
    Y, Cb, Cr = ycbcr(padded)
    if M == 16:
        Cb, Cr = ((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2 for p in (Cb, Cr))
        layout = [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (2, 0, 0)]           # (component, block row, block column) in the MCU
    else:
        layout = [(0, 0, 0), (1, 0, 0), (2, 0, 0)]
    planes = [Y - 128, Cb - 128, Cr - 128]
    luma_q, chroma_q = quant_tables(quality)
    out = bytearray(header(W, H, quality, subsampling))
    for my in range(mrows):                            # one restart interval per MCU row
        bw, pred = BitWriter(), [0, 0, 0]
        for mx in range(mcols):
            for c, by, bx in layout:
                side = M // 8 if c == 0 else 1         # blocks of this component along an MCU side
                y0, x0 = 8 * (my * side + by), 8 * (mx * side + bx)
                zz = fdct_quantise(planes[c][y0:y0 + 8, x0:x0 + 8], chroma_q if c else luma_q)
                code_block(zz, pred[c], DC_CODES[c > 0], AC_CODES[c > 0], bw, stats)
                pred[c] = zz[0]
        out += bw.finish(stats)
        out += bytes([0xFF, 0xD0 + my % 8 if my + 1 < mrows else 0xD9])
    return bytes(out)


def max_bytes(W, H, subsampling):
    """The bound ``mc_mjpeg_max_bytes`` gives for one frame."""
    M, mcols, mrows = mcu_grid(W, H, subsampling)
    return len(header(W, H, 50, subsampling)) + mrows * (2 * 208 * mcols * (6 if M == 16 else 3) + 2)


# ---- the images and cases the host and device tests share -----------------------------------------------------------------------------

def image(content, W, H, seed=0):
    """uint8 [H, W, 3]."""
    y, x = np.mgrid[0:H, 0:W]
    if content == 'constant':                          # all EOB, zero DC differences after the first block
        return np.broadcast_to(np.array([200, 30, 90], np.uint8), (H, W, 3)).copy()
    if content == 'noise':                             # long codes; 0xFF bytes in the stream are certain
        return np.random.RandomState(1000 + seed).randint(0, 256, (H, W, 3)).astype(np.uint8)
    if content == 'checker':                           # one-pixel 0 / 255: the largest categories
        return np.repeat((((x + y + seed) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    if content == 'ramp':                              # a smooth ramp under a one-pixel ripple: at quality 10 only the lowest and the
        # highest frequency survive, with a zero run of more than 16 between them (a ramp alone ends in EOB and never needs ZRL)
        v = 40 + (110 * x) // max(W - 1, 1) + (30 * y) // max(H - 1, 1) + 60 * ((x & 1) ^ (y & 1) ^ (seed & 1))
        return np.stack([v, v, 255 - v], axis=2).astype(np.uint8)
    if content == 'shapes':                            # what the renderers draw: white background, flat colours, hard edges
        img = np.full((H, W, 3), 255, np.uint8)
        img[(x - W * 0.4) ** 2 + (y - H * 0.5) ** 2 <= (0.3 * min(W, H) + seed) ** 2] = [220, 40, 40]
        img[(abs(x - y - seed) <= 1) & (x > W // 4)] = [0, 0, 255]
        img[H // 2:, W // 2:W // 2 + max(W // 5, 1)] = [96, 96, 96]
        return img
    raise ValueError(content)


CONTENTS = ('constant', 'noise', 'checker', 'ramp', 'shapes')
QUALITIES = (10, 50, 90, 100)
# (W, H, content, quality, subsampling): every size, content, quality and subsampling at least once, the full cross at 37x23.
# 16x16 one MCU; 17x33 one pixel over both ways; 37x23 ragged; 272x16 17 MCUs in one interval; 16x144 nine MCU rows, so the RST counter
# wraps; 700x16 / 700x8 put 264 blocks into one interval, more than the 256 the entropy kernel holds in LDS at a time, and at quality
# 100 more than the 1024 bytes the pack kernel moves per pass.
CASES = [(37, 23, c, q, s) for c in CONTENTS for q in QUALITIES for s in SUBSAMPLINGS] + [
    (16, 16, 'constant', 90, '4:2:0'), (16, 16, 'noise', 100, '4:4:4'), (17, 33, 'noise', 90, '4:2:0'), (17, 33, 'checker', 50, '4:4:4'),
    (64, 48, 'ramp', 10, '4:2:0'), (64, 48, 'shapes', 90, '4:4:4'), (64, 48, 'noise', 50, '4:2:0'), (272, 16, 'noise', 100, '4:2:0'),
    (272, 16, 'ramp', 10, '4:4:4'), (16, 144, 'checker', 90, '4:2:0'), (16, 144, 'noise', 90, '4:4:4'), (700, 16, 'noise', 100, '4:2:0'),
    (700, 8, 'shapes', 50, '4:4:4')]
assert {c[:2] for c in CASES} >= {(16, 16), (17, 33), (37, 23), (64, 48), (272, 16), (16, 144)}


def case_id(case):
    return '{}x{}-{}-q{}-{}'.format(*case).replace(':', '')


_cache = {}


def reference(case, seed=0):
    """(image, its encoding, the encoder's statistics) of a case, computed once."""
    key = (case, seed)
    if key not in _cache:
        W, H, content, quality, subsampling = case
        img, stats = image(content, W, H, seed), {}
        _cache[key] = (img, encode(img, quality, subsampling, stats), stats)
    return _cache[key]
