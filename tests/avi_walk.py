"""What the host and the device tests of ``video.py`` share besides ``jpeg_ref.py``: the AVI chunk walker, which needs the standard
library alone, and libjpeg's decoder behind PIL.  Test infrastructure: neither test file imports the other."""
import io
import struct

import pytest


def decode(data):
    """JPEG bytes -> the loaded PIL image.  Pillow is looked for HERE, so that only a test that asks libjpeg for a judgement skips
    without it, and only after the assertions in front of the call."""
    Image = pytest.importorskip('PIL.Image')
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def walk_avi(path):
    """Read an AVI file chunk by chunk, checking its structure on the way: RIFF size, word alignment, every idx1 entry.  Returns what
    the headers say and the payloads of the movi chunks."""
    data = open(path, 'rb').read()
    assert data[:4] == b'RIFF' and data[8:12] == b'AVI ' and struct.unpack('<I', data[4:8])[0] == len(data) - 8
    out = dict(file_bytes=len(data), video=[], audio=None, streams=[], padded=0)

    def children(lo, hi):
        at = lo
        while at < hi:
            tag, size = data[at:at + 4], struct.unpack('<I', data[at + 4:at + 8])[0]
            assert at + 8 + size <= hi, (tag, at)
            yield tag, at, at + 8, size
            if size & 1:
                assert data[at + 8 + size] == 0                    # the pad byte
                out['padded'] += 1
            at += 8 + size + (size & 1)
        assert at == hi

    top = list(children(12, len(data)))
    assert [(t, data[b:b + 4]) if t == b'LIST' else t for t, _, b, _ in top] == [(b'LIST', b'hdrl'), (b'LIST', b'movi'), b'idx1']
    (_, _, hb, hs), (_, _, mb, ms), (_, _, ib, isz) = top
    for tag, _, b, size in children(hb + 4, hb + hs):
        if tag == b'avih':
            assert size == 56
            f = struct.unpack('<14I', data[b:b + 56])
            out.update(usec=f[0], flags=f[3], frames=f[4], nstreams=f[6], width=f[8], height=f[9])
        else:
            assert tag == b'LIST' and data[b:b + 4] == b'strl'
            (t1, _, b1, s1), (t2, _, b2, s2) = children(b + 4, b + size)
            assert (t1, s1, t2) == (b'strh', 56, b'strf')
            h = struct.unpack('<4s4sIHHIIIIIIIIhhhh', data[b1:b1 + 56])
            out['streams'].append(dict(type=h[0], handler=h[1], scale=h[6], rate=h[7], length=h[9], sample_size=h[12], rect=h[13:], strf=data[b2:b2 + s2]))
    movi = []
    for tag, at, b, size in children(mb + 4, mb + ms):
        movi.append((tag, at - mb, size))                          # idx1 counts from the 'movi' tag
        (out['video'] if tag == b'00dc' else movi_audio(out)).append(data[b:b + size])
    index = [struct.unpack('<4sIII', data[ib + 16 * k:ib + 16 * k + 16]) for k in range(isz // 16)]
    assert isz % 16 == 0 and [(t, o, s) for t, _, o, s in index] == movi and all(f == 0x10 for _, f, _, _ in index)
    for tag, _, offset, size in index:                             # every entry points at the header of the chunk it names
        assert data[mb + offset:mb + offset + 4] == tag and struct.unpack('<I', data[mb + offset + 4:mb + offset + 8])[0] == size
    v = out['streams'][0]
    assert out['nstreams'] == len(out['streams']) and (v['type'], v['handler']) == (b'vids', b'MJPG') and v['length'] == out['frames'] == len(out['video'])
    assert v['rect'] == (0, 0, out['width'], out['height']) and out['flags'] & 0x10
    assert struct.unpack('<IiiHH4sIiiII', v['strf']) == (40, out['width'], out['height'], 1, 24, b'MJPG', 3 * out['width'] * out['height'], 0, 0, 0, 0)
    out['rate_scale'] = (v['rate'], v['scale'])
    assert out['usec'] == round(1e6 * v['scale'] / v['rate'])
    if len(out['streams']) == 2:
        a = out['streams'][1]
        fmt = struct.unpack('<HHIIHHH', a['strf'])
        assert a['type'] == b'auds' and fmt[0] == 1 and fmt[5] == 16 and fmt[4] == 2 * fmt[1] == a['sample_size'] and fmt[3] == fmt[2] * fmt[4] and fmt[6] == 0
        assert (a['rate'], a['scale']) == (fmt[2], 1) and a['length'] * fmt[4] == sum(len(c) for c in out['audio'])
        assert [t for t, _, _ in movi] == [b'00dc', b'01wb'] * out['frames']      # each frame is followed by its share of the audio
        out.update(audio_rate=fmt[2], channels=fmt[1])
    else:
        assert out['audio'] is None and all(t == b'00dc' for t, _, _ in movi)
    return out


def movi_audio(out):
    if out['audio'] is None:
        out['audio'] = []
    return out['audio']
