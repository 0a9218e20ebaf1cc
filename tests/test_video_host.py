"""Host side of ``video.py`` (no GPU): the restatement ``jpeg_ref.py`` judged by libjpeg (through PIL), ``AviWriter`` walked chunk by
chunk, the argument errors, the library's symbols and the tools' new flags.

Pillow is asked for inside the tests that need libjpeg's judgement (``decode``, ``libjpeg()``), after what they can assert without it:
where it is missing those skip, and the writer, argument, export and tool tests run as they are, fed the restatement's own files."""
import contextlib
import fractions
import io
import os
import runpy
import struct
import sys

import numpy as np
import pytest
import torch

import jpeg_ref as J
from avi_walk import decode, walk_avi
import motioncraft_amd as mc
from motioncraft_amd import lib as L
from motioncraft_amd import video

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
PIL_SUBSAMPLING = {'4:4:4': 0, '4:2:0': 2}


# ---- the restatement under libjpeg's eyes ---------------------------------------------------------------------------------------------

def segments(data):
    """[(marker, payload)] of a JPEG file's header, up to and including SOS."""
    out, i = [], 2
    while True:
        assert data[i] == 0xFF
        n = struct.unpack('>H', data[i + 2:i + 4])[0]
        out.append((data[i + 1], data[i + 4:i + 2 + n]))
        i += 2 + n
        if out[-1][0] == 0xDA:
            return out


def libjpeg():
    """``PIL.Image``: libjpeg's encoder."""
    return pytest.importorskip('PIL.Image')


@pytest.mark.parametrize('case', J.CASES, ids=J.case_id)
def test_restatement_is_a_legal_jpeg_of_the_true_size(case):
    """libjpeg decodes every case of the device test, restart markers and stuffing included, to the true size and mode RGB."""
    W, H, content, quality, subsampling = case
    im = decode(J.reference(case)[1])
    assert im.size == (W, H) and im.mode == 'RGB'


@pytest.mark.parametrize('case', J.CASES, ids=J.case_id)
def test_restatement_segments_markers_and_bound(case):
    """What needs no decoder: the header's segments in their order, DRI, one RSTm per MCU row counting mod 8, EOI, the stuffed bytes,
    and the stream inside the bound the library promises."""
    W, H, content, quality, subsampling = case
    img, data, stats = J.reference(case)
    assert len(data) <= J.max_bytes(W, H, subsampling)
    M, mcols, mrows = J.mcu_grid(W, H, subsampling)
    seg = segments(data)
    assert [m for m, _ in seg] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert seg[8][1] == struct.pack('>H', mcols) and data[-2:] == b'\xff\xd9'
    body = data[len(J.header(W, H, quality, subsampling)):]
    assert [body[i + 1] for i in range(len(body) - 1) if body[i] == 0xFF and body[i + 1] != 0] == [0xD0 + r % 8 for r in range(mrows - 1)] + [0xD9]
    assert body.count(b'\xff\x00') == stats.get('stuffed', 0)


def test_tables_are_the_standards():
    """libjpeg writes the Annex K tables when it is not asked to optimise: the same DHT segments, and at quality 50 the same DQT."""
    assert J.quant_tables(50) == [J.LUMA_Q, J.CHROMA_Q] and set(J.quant_tables(100)[0]) == {1} and max(J.quant_tables(1)[1]) == 255
    assert J.quant_tables(10)[0][:4] == [80, 55, 50, 80] and J.quant_tables(90)[0][:4] == [3, 2, 2, 3]
    assert sorted(J.ZIGZAG) == list(range(64)) and J.ZIGZAG[:6] == [0, 1, 8, 16, 9, 2]
    buf = io.BytesIO()
    libjpeg().fromarray(J.image('noise', 16, 16)).save(buf, format='JPEG', quality=50, subsampling=2)
    theirs = {(m, p[0]): p for m, p in segments(buf.getvalue()) if m in (0xC4, 0xDB)}
    ours = {(m, p[0]): p for m, p in segments(J.header(16, 16, 50, '4:2:0')) if m in (0xC4, 0xDB)}
    assert len(ours) == 6 and ours == theirs


def psnr(a, b):
    mse = np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)
    return np.inf if mse == 0 else 10 * np.log10(255 ** 2 / mse)


def test_quality_against_libjpeg():
    """PSNR of decode(restatement) against the source, beside the PSNR of decode(PIL's own encoding) with the SAME quantisation tables
    and subsampling, over every case that is not noise.  The two encoders differ in the DCT's rounding and in the chroma mean only.
    Measured: the worst shortfall is 0.245 dB (37x23 shapes, quality 100, 4:4:4: every table entry is 1, so the DCT's own rounding is
    all there is, 56.81 dB against 57.06), the next 0.21 dB (700x8 shapes, quality 50, 4:4:4), every other case is within 0.07 dB.  The
    bound is the worst shortfall rounded up to the next 0.1 dB."""
    Image, worst = libjpeg(), -np.inf
    for case in J.CASES:
        W, H, content, quality, subsampling = case
        if content == 'noise':
            continue
        img, data, _ = J.reference(case)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format='JPEG', qtables=J.quant_tables(quality), subsampling=PIL_SUBSAMPLING[subsampling])
        theirs = decode(buf.getvalue())
        assert {k: list(v) for k, v in theirs.quantization.items()} == dict(enumerate(J.quant_tables(quality)))      # the same tables went in
        ours = psnr(decode(data), img)
        short = 0.0 if ours == np.inf else psnr(theirs, img) - ours
        print(f'{J.case_id(case)}: {ours:.2f} dB, libjpeg {psnr(theirs, img):.2f} dB')
        worst = max(worst, short)
    print(f'worst shortfall {worst:.3f} dB')
    assert worst <= 0.3


def test_restatement_properties():
    """What each content is in the table for, and the arithmetic's ranges."""
    flat, stats = J.image('constant', 37, 23), {}
    data = J.encode(flat, 90, '4:2:0', stats)
    # all EOB: a block after the first of its component is a 2-bit zero difference and an EOB of 2 or 4 bits
    assert stats.get('zrl', 0) == 0 and stats['longest'] <= (18 * 6 + 3 * 20 + 7) // 8 and len(data) < len(J.header(37, 23, 90, '4:2:0')) + 2 * (21 + 2)
    R, G, B = np.meshgrid(*[np.array([0, 1, 127, 128, 254, 255])] * 3)
    Y, Cb, Cr = J.ycbcr(np.stack([R, G, B], axis=-1).astype(np.uint8))
    assert min(Y.min(), Cb.min(), Cr.min()) == 0 and max(Y.max(), Cb.max(), Cr.max()) == 255
    grey = J.ycbcr(np.full((1, 1, 3), 77, np.uint8))
    assert [int(p[0, 0]) for p in grey] == [77, 128, 128]
    # the DCT of a constant block is its DC alone, 8 x the value at quality 100 (within the table's rounding)
    zz = J.fdct_quantise(np.full((8, 8), 100, np.int64), [1] * 64)
    assert abs(zz[0] - 800) <= 1 and not any(zz[1:])
    # the extremes stay inside the categories the Huffman tables have
    for block in (np.full((8, 8), -128), np.full((8, 8), 127), np.where(np.add.outer(np.arange(8), np.arange(8)) & 1, 127, -128)):
        zz = J.fdct_quantise(block.astype(np.int64), [1] * 64)
        assert abs(zz[0]) <= 1024 and max(abs(v) for v in zz[1:]) <= 1023
    st = {}
    J.encode(J.image('ramp', 64, 48), 10, '4:2:0', st)
    assert st['zrl'] >= 1
    st = {}
    J.encode(J.image('noise', 37, 23), 100, '4:4:4', st)
    assert st['stuffed'] >= 1


# ---- AviWriter ------------------------------------------------------------------------------------------------------------------------

def pil_jpegs(n, W=37, H=23):
    """(images, PIL's encodings of them): the writer takes any JPEG bytes -- the restatement's where there is no Pillow, since what
    the writer's tests judge is the container.  A byte behind EOI, which decoders ignore, makes the length of file k odd for odd k
    and even for even k, so both kinds of chunk are there."""
    try:
        from PIL import Image
    except ImportError:
        Image = None
    imgs = [J.image('shapes', W, H, seed) for seed in range(n)]
    files = []
    for k, im in enumerate(imgs):
        buf = io.BytesIO()
        if Image is None:
            buf.write(J.encode(im, 60 + k))
        else:
            Image.fromarray(im).save(buf, format='JPEG', quality=60 + k)
        data = buf.getvalue()
        files.append(data if len(data) & 1 == k & 1 else data + b'\0')
    return imgs, files


@pytest.mark.parametrize('fps,want', [(20, (20, 1)), (30, (30, 1)), (29.97, (2997, 100)), (30000 / 1001, (30000, 1001)), (fractions.Fraction(24000, 1001), (24000, 1001)),
                                      (12.5, (25, 2))])
def test_avi_structure_and_frame_rate(tmp_path, fps, want):
    """``dwRate / dwScale`` is ``Fraction(fps).limit_denominator(1001)``: exact for every rate that has such a fraction -- 29.97 is
    2997 / 100, the NTSC rate 30000 / 1001 is itself."""
    imgs, files = pil_jpegs(4)
    path = str(tmp_path / 'a.avi')
    with video.AviWriter(path, 37, 23, fps) as w:
        w.add_frames(files[:1])
        w.add_frames(files[1])                                     # one frame as plain bytes
        w.add_frames(files[2:])
    avi = walk_avi(path)
    assert avi['rate_scale'] == want and avi['frames'] == 4 and (avi['width'], avi['height']) == (37, 23) and avi['audio'] is None
    assert avi['usec'] == round(1e6 * want[1] / want[0])
    assert avi['video'] == files and avi['padded'] == sum(len(f) & 1 for f in files) == 2        # odd-sized chunks are padded


def test_avi_payloads_decode_to_the_frames(tmp_path):
    imgs, files = pil_jpegs(4)
    path = str(tmp_path / 'a.avi')
    with video.AviWriter(path, 37, 23, 20) as w:
        w.add_frames(files)
    for im, data in zip(imgs, walk_avi(path)['video']):
        got = decode(data)
        assert got.size == (37, 23) and psnr(got, im) > 20


def audio_share(i, rate, fps):
    f = fractions.Fraction(fps).limit_denominator(1001)
    return round((i + 1) * rate / f) - round(i * rate / f)


@pytest.mark.parametrize('fps,rate,channels', [(20, 16000, 1), (30, 44100, 1), (29.97, 16000, 1), (30000 / 1001, 22050, 2), (7, 8001, 1)])
def test_avi_audio_is_interleaved_cut_and_padded(tmp_path, fps, rate, channels):
    n = 9
    _, files = pil_jpegs(n)
    f = fractions.Fraction(fps).limit_denominator(1001)
    total = round(n * rate / f)
    rs = np.random.RandomState(3)
    for extra in (+1000, -1000, 0):                                # longer than the video, shorter, exactly as long
        pcm = rs.randint(-32768, 32768, (total + extra, channels)).astype(np.int16)
        path = str(tmp_path / f'a{extra}.avi')
        with video.AviWriter(path, 37, 23, fps, audio_rate=rate, audio_channels=channels) as w:
            w.add_audio(pcm[:500] if channels > 1 else pcm[:500, 0])
            w.add_audio(pcm[500:])
            w.add_frames(files)
        avi = walk_avi(path)
        assert (avi['audio_rate'], avi['channels'], avi['frames']) == (rate, channels, n) and avi['video'] == files
        counts = [len(a) // (2 * channels) for a in avi['audio']]
        assert counts == [audio_share(i, rate, fps) for i in range(n)] and sum(counts) == total == avi['streams'][1]['length']
        back = np.frombuffer(b''.join(avi['audio']), '<i2').reshape(-1, channels)
        kept = min(total, total + extra)
        assert np.array_equal(back[:kept], pcm[:kept]) and not back[kept:].any()      # cut, or padded with silence
    if rate * f.denominator % f.numerator:
        assert len(set(counts)) > 1                                # the shares differ where rate / fps is no integer


def test_avi_limit_raises_before_the_chunk(tmp_path):
    _, files = pil_jpegs(6)
    path = str(tmp_path / 'limited.avi')
    probe = str(tmp_path / 'probe.avi')
    with video.AviWriter(probe, 37, 23, 20, audio_rate=8000) as w:
        w.add_frames(files[:3])
    three = os.path.getsize(probe)
    w = video.AviWriter(path, 37, 23, 20, audio_rate=8000, limit=three + 40)
    w.add_frames(files[:3])
    with pytest.raises(ValueError, match='RIFF limit'):
        w.add_frames(files[3:])
    assert w.frames == 3
    w.close()
    w.close()                                                      # idempotent
    assert open(path, 'rb').read() == open(probe, 'rb').read()     # no half-written chunk: the file of the three frames, whole
    assert walk_avi(path)['frames'] == 3
    with pytest.raises(ValueError, match='closed'):
        w.add_frames(files[:1])
    exact = video.AviWriter(str(tmp_path / 'exact.avi'), 37, 23, 20, audio_rate=8000, limit=three)
    exact.add_frames(files[:3])                                    # the limit itself is allowed
    exact.close()
    assert os.path.getsize(str(tmp_path / 'exact.avi')) == three
    assert video.RIFF_LIMIT == 2 ** 31 - 1


def test_argument_errors(tmp_path):
    for kw in (dict(width=0), dict(height=16385), dict(width=8.0), dict(quality=0), dict(quality=101), dict(quality=90.0), dict(subsampling='4:2:2'),
               dict(subsampling=0)):
        with pytest.raises(ValueError):
            video.JpegEncoder(**{**dict(width=16, height=16), **kw})
    enc = video.JpegEncoder(16, 8)
    assert (enc.quality, enc.subsampling) == (90, '4:2:0')
    for bad in (np.zeros((1, 8, 16, 3), np.uint8), torch.zeros(1, 8, 16, 3), torch.zeros(1, 16, 8, 3, dtype=torch.uint8), torch.zeros(8, 16, dtype=torch.uint8),
                torch.zeros(1, 8, 16, 3, dtype=torch.uint8)):                     # the last: host memory
        with pytest.raises(ValueError):
            enc.encode(bad)
    with pytest.raises(ValueError, match='device'):
        enc.encode(torch.zeros(1, 8, 16, 3, dtype=torch.uint8))
    enc.close()
    p = str(tmp_path / 'x.avi')
    for kw in (dict(width=0), dict(fps=0), dict(fps=-1), dict(fps='30'), dict(fps=1e-9), dict(audio_rate=0), dict(audio_rate=16000.0),
               dict(audio_channels=0), dict(limit=0), dict(limit=2 ** 31)):
        with pytest.raises(ValueError):
            video.AviWriter(**{**dict(path=p, width=16, height=16, fps=20), **kw})
    assert not os.path.exists(p)                                   # a refused writer leaves no file
    with video.AviWriter(p, 16, 16, 20) as w:
        with pytest.raises(ValueError, match='audio_rate'):
            w.add_audio(np.zeros(4, np.int16))
        with pytest.raises(ValueError, match='JPEG'):
            w.add_frames([b'BM not a jpeg'])
    with video.AviWriter(p, 16, 16, 20, audio_rate=8000) as w:
        for bad in (np.zeros(4, np.float32), np.zeros((4, 2), np.int16), np.zeros((2, 2, 2), np.int16)):
            with pytest.raises(ValueError, match='audio'):
                w.add_audio(bad)
    frames = torch.zeros(2, 8, 16, 3, dtype=torch.uint8)
    for args, kw in (((frames.float(), p, 20), {}), ((frames[0], p, 20), {}), ((frames[:0], p, 20), {}), ((frames, p, 20), dict(audio=np.zeros(4, np.int16))),
                     ((frames, p, 20), dict(audio_rate=8000)), ((frames, p, 20), dict(audio=np.zeros(4), audio_rate=8000)), ((frames, p, 20), {})):
        with pytest.raises(ValueError):                            # the last: host memory
            video.save_avi(*args, **kw)


def test_library_and_package_export_the_encoder():
    lib = L.load()
    for name in ('mc_mjpeg_create', 'mc_mjpeg_destroy', 'mc_mjpeg_work_bytes', 'mc_mjpeg_max_bytes', 'mc_mjpeg_encode'):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.mc_mjpeg_work_bytes(None, 1) == -1 and lib.mc_mjpeg_max_bytes(None, 1) == -1
    for name in ('video', 'JpegEncoder', 'AviWriter', 'save_avi'):
        assert name in mc.__all__ and hasattr(mc, name)
    assert mc.JpegEncoder is video.JpegEncoder


# ---- the tools' flags -----------------------------------------------------------------------------------------------------------------

def run_main(name, *args):
    """A tool's ``main`` in this process, under its own command line -> (0, its exit code or the exception it ended with; its stdout)."""
    argv, path, out = sys.argv, list(sys.path), io.StringIO()
    sys.argv = [os.path.join(ROOT, 'tools', name)] + list(args)
    try:
        with contextlib.redirect_stdout(out), contextlib.redirect_stderr(io.StringIO()):
            runpy.run_path(sys.argv[0], run_name='__main__')
        return 0, out.getvalue()
    except SystemExit as e:
        return e.code, out.getvalue()
    except (ValueError, RuntimeError) as e:
        return e, out.getvalue()
    finally:
        sys.argv, sys.path[:] = argv, path


def test_tool_flags(tmp_path):
    """The new flags parse; a bad value is refused before the device is touched; without a GPU ``--avi`` ends with the library's
    message and writes nothing."""
    for tool, flags in (('render_npz.py', ('--avi', '--avi_quality', '--audio')), ('skeleton_npy.py', ('--avi', '--avi_quality')),
                        ('sample.py', ('--render_avi', '--anim_avi', '--avi_quality')), ('video_time.py', ('--frames', '--quality'))):
        rc, out = run_main(tool, '--help')
        assert rc == 0 and all(f in out for f in flags), (tool, rc)
    refused = lambda rc, *words: isinstance(rc, ValueError) and all(w in str(rc) for w in words)
    npy, avi = str(tmp_path / 'joints.npy'), str(tmp_path / 'a.avi')
    np.save(npy, np.zeros((3, 22, 3), np.float32))
    assert refused(run_main('skeleton_npy.py', npy)[0], '--out', '--avi')                       # one of the two is needed
    assert refused(run_main('skeleton_npy.py', npy, '--avi', avi, '--avi_quality', '0')[0], '--avi_quality')
    npz = str(tmp_path / 'res_x.npz')
    np.savez(npz, poses=np.zeros((2, 165)), expressions=np.zeros((2, 100)), trans=np.zeros((2, 3)), betas=np.zeros(300))
    assert refused(run_main('render_npz.py', npz, '--smplx_model', 'none.npz')[0], '--out', '--avi')
    # the speech goes into the AVI and nowhere else
    assert refused(run_main('render_npz.py', npz, '--smplx_model', 'none.npz', '--out', str(tmp_path), '--audio', 'x.wav')[0], '--audio', '--avi')
    assert refused(run_main('render_npz.py', npz, '--smplx_model', 'none.npz', '--avi', avi, '--avi_quality', '101')[0], '--avi_quality')
    if not torch.cuda.is_available():
        rc, _ = run_main('skeleton_npy.py', npy, '--avi', avi)
        assert isinstance(rc, RuntimeError) and 'no HIP device visible' in str(rc)
    assert not os.path.exists(avi)
