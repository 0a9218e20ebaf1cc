"""On the MI355X: ``video.JpegEncoder`` (``mc_mjpeg_*``, csrc/mc_mjpeg.hip) against the numpy restatement ``jpeg_ref.py``.

Every assertion on the encoder's output is BYTE EQUALITY with the restatement: the encoder is integer arithmetic from the pixels to the
bit stream, so there is no tolerance to state.  With it go ``offsets`` ascending from 0 to the total length, the bound of
``mc_mjpeg_max_bytes``, and the two refusals of ``mc_mjpeg_encode``, which are return codes, not faults.
"""
import ctypes
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

import jpeg_ref as J
import raster_ref
import smplx_lbs_ref as lbs_ref
from avi_walk import decode, walk_avi
from motioncraft_amd import lib as L
from motioncraft_amd import render as mr
from motioncraft_amd import skeleton as sk
from motioncraft_amd import video

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


def encode(images, quality, subsampling, **kw):
    """[n, H, W, 3] uint8 on the host -> the device's files."""
    images = np.ascontiguousarray(images)
    enc = video.JpegEncoder(images.shape[2], images.shape[1], quality, subsampling)
    out = enc.encode(torch.from_numpy(images).cuda(), **kw)
    enc.close()
    return out


@pytest.mark.parametrize('case', J.CASES, ids=J.case_id)
def test_bytes_equal_the_restatement(case):
    W, H, content, quality, subsampling = case
    img, want, stats = J.reference(case)
    if content == 'noise':
        assert stats['stuffed'] >= 1               # the case is about 0xFF 0x00: it must not stop covering it
    if content == 'ramp' and quality == 10:
        assert stats['zrl'] >= 1                   # ... and this one about ZRL
    if W == 700:
        assert stats['longest'] > (1024 if content == 'noise' else 0)
    got = encode(img[None], quality, subsampling)
    assert len(got) == 1 and got[0] == want, (len(got[0]), len(want))


def scene_frames():
    """One small frame from each renderer: white background, flat colours, hard edges."""
    v, f = raster_ref.octahedron(2, 0.5)
    r = mr.MeshRenderer(f, v.shape[0], width=64, height=48)
    mesh = r.render(torch.from_numpy(v[None].astype(np.float32)).cuda())
    r.close()
    rs = np.random.RandomState(0)
    joints = rs.uniform(-0.4, 0.4, (3, 22, 3)).astype(np.float32) + np.array([0, 0.9, 0], np.float32)
    s = sk.SkeletonRenderer(sk.T2M_CHAINS, width=64, height=48)
    skel = s.render(torch.from_numpy(joints).cuda())
    s.close()
    assert (mesh != 255).any() and (skel != 255).any() and (mesh == 255).any()
    return mesh, skel


@pytest.mark.parametrize('subsampling', J.SUBSAMPLINGS)
def test_rendered_frames_equal_the_restatement(subsampling):
    for frames in scene_frames():
        enc = video.JpegEncoder(64, 48, 90, subsampling)
        got = enc.encode(frames)
        enc.close()
        host = frames.cpu().numpy()
        assert len(got) == host.shape[0]
        for i, data in enumerate(got):
            assert data == J.encode(host[i], 90, subsampling), i


def five():
    return np.stack([J.image(c, 37, 23, seed) for seed, c in enumerate(('shapes', 'noise', 'ramp', 'checker', 'constant'))])


def test_batches_chunks_and_repetition_give_the_same_bytes():
    imgs = five()
    want = [J.encode(im, 50, '4:2:0') for im in imgs]
    assert len(set(want)) == 5
    enc = video.JpegEncoder(37, 23, 50, '4:2:0')
    dev = torch.from_numpy(imgs).cuda()
    need = lambda n: int(enc.native().lib.mc_mjpeg_work_bytes(enc.native().handle, n))
    assert 0 < need(1) < need(2) < need(5) == 5 * need(1) and need(0) == -1
    assert enc.encode(dev) == want
    assert enc.encode(dev) == want                                               # a second call on the same object and scratch
    for wb in (need(1), need(2), need(2) + 256, 0):                              # 5, 3, 3 and 5 chunks
        assert enc.encode(dev, work_bytes=wb) == want, wb
    assert enc.encode(dev[3]) == want[3:4] and enc.encode(dev[:1]) == want[:1]  # n = 1, as [H, W, 3] and as [1, H, W, 3]
    assert enc.encode(dev[:0]) == []
    assert enc.encode(dev.flip(0)) == want[::-1]
    assert enc.encode(dev[:, :, :, [0, 1, 2]].transpose(1, 2).contiguous().transpose(1, 2)) == want      # not contiguous
    enc.close()


def test_offsets_refusals_and_the_bound():
    """The C entry points themselves: ``offsets``, the bound, and the two refusals.  A refusal is a return code: nothing is launched."""
    imgs = np.stack([J.image('noise', 37, 23, seed) for seed in range(3)])
    want = [J.encode(im, 100, '4:4:4') for im in imgs]
    o = L.NativeObject('mjpeg', 37, 23, 100, video.SUBSAMPLINGS['4:4:4'])
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    bound, wb = int(o.lib.mc_mjpeg_max_bytes(o.handle, 3)), int(o.lib.mc_mjpeg_work_bytes(o.handle, 3))
    assert bound == 3 * J.max_bytes(37, 23, '4:4:4') and int(o.lib.mc_mjpeg_max_bytes(o.handle, 1)) * 3 == bound
    assert all(len(w) <= bound // 3 for w in want)                               # noise at quality 100 stays inside the bound
    assert o.lib.mc_mjpeg_max_bytes(None, 1) == -1 and o.lib.mc_mjpeg_work_bytes(None, 1) == -1 and o.lib.mc_mjpeg_max_bytes(o.handle, -1) == -1
    rgb = torch.from_numpy(imgs).cuda()
    work = torch.empty(wb, dtype=torch.uint8, device='cuda')
    out = torch.full((bound,), 0xA5, dtype=torch.uint8, device='cuda')
    offsets = torch.full((4,), -7, dtype=torch.int64, device='cuda')
    call = lambda work_bytes, capacity: o.lib.mc_mjpeg_encode(o.handle, ptr(rgb), 3, ptr(work), work_bytes, ptr(out), capacity, ptr(offsets), None)
    assert call(wb, bound - 1) == 1 and 'out_capacity' in L.last_error()
    assert call(wb // 3 - 1, bound) == 1 and 'work_bytes' in L.last_error()
    torch.cuda.synchronize()
    assert (out == 0xA5).all() and (offsets == -7).all()                         # untouched
    assert call(wb, bound) == L.MC_OK, L.last_error()
    torch.cuda.synchronize()
    at = offsets.cpu().tolist()
    assert at[0] == 0 and all(a < b for a, b in zip(at, at[1:])) and at[3] == sum(len(w) for w in want)
    data = out.cpu().numpy().tobytes()
    assert [data[at[i]:at[i + 1]] for i in range(3)] == want
    assert (out[at[3]:] == 0xA5).all()                                           # nothing is written behind the last file
    h = ctypes.c_void_p()
    for bad in ((0, 8, 90, 0), (8, 16385, 90, 0), (8, 8, 0, 0), (8, 8, 101, 1), (8, 8, 90, 2)):
        assert o.lib.mc_mjpeg_create(*bad, ctypes.byref(h)) == 1, bad
    o.close()


def test_save_avi_of_rendered_frames_with_a_tone(tmp_path):
    """``save_avi`` end to end: skeleton frames from the device + a synthetic tone -> the host test's chunk walker and PIL."""
    _, skel = scene_frames()
    rate, fps = 16000, 20
    tone = np.round(8000 * np.sin(2 * np.pi * 440 * np.arange(rate // 4) / rate)).astype(np.int16)       # longer than 3 frames: cut
    path = str(tmp_path / 'clip.avi')
    size = video.save_avi(skel, path, fps, audio=tone, audio_rate=rate, quality=90)
    avi = walk_avi(path)
    assert size == avi['file_bytes'] and avi['frames'] == 3 and (avi['width'], avi['height']) == (64, 48) and avi['rate_scale'] == (20, 1)
    host = skel.cpu().numpy()
    for i, data in enumerate(avi['video']):
        assert data == J.encode(host[i], 90, '4:2:0')
    assert [len(a) // 2 for a in avi['audio']] == [800, 800, 800]
    assert np.array_equal(np.frombuffer(b''.join(avi['audio']), '<i2'), tone[:2400])
    silent = str(tmp_path / 'silent.avi')
    video.save_avi(skel, silent, fps, subsampling='4:4:4')
    assert walk_avi(silent)['audio'] is None
    for data in avi['video']:                                                    # libjpeg last: without Pillow only this is left out
        im = decode(data)
        assert im.size == (64, 48) and im.mode == 'RGB'


def test_save_avi_is_all_or_nothing(tmp_path, monkeypatch):
    """A clip that passes the RIFF limit at its last frame, and an encoder that cannot be created: the error comes out and no
    header-only or partial file stays at ``path``."""
    _, skel = scene_frames()
    path = str(tmp_path / 'clip.avi')
    size = video.save_avi(skel, path, 20)
    assert size == os.path.getsize(path)
    writer = video.AviWriter
    monkeypatch.setattr(video, 'AviWriter', lambda *a, **kw: writer(*a, limit=size - 1, **kw))
    with pytest.raises(ValueError, match='RIFF limit'):
        video.save_avi(skel, path, 20)
    assert os.listdir(tmp_path) == []
    monkeypatch.setattr(video, 'AviWriter', writer)

    def refuse(self):
        raise RuntimeError('no encoder')
    monkeypatch.setattr(video.JpegEncoder, 'native', refuse)
    with pytest.raises(RuntimeError, match='no encoder'):
        video.save_avi(skel, path, 20)
    assert os.listdir(tmp_path) == []


def run_tool(name, *args):
    run = subprocess.run(['timeout', '-k', '10', '120', sys.executable, os.path.join(ROOT, 'tools', name)] + list(args), capture_output=True, text=True,
                         timeout=150)
    assert run.returncode == 0, run.stderr[-2000:]
    return run.stdout


def test_skeleton_tool_writes_one_file(tmp_path):
    """``tools/skeleton_npy.py joints.npy --avi out.avi`` in a child process: one file, no frames directory, no ffmpeg."""
    rs = np.random.RandomState(1)
    npy, avi = str(tmp_path / 'joints.npy'), str(tmp_path / 'out.avi')
    np.save(npy, rs.uniform(-0.4, 0.4, (5, 22, 3)).astype(np.float32) + np.array([0, 0.9, 0], np.float32))
    run_tool('skeleton_npy.py', npy, '--avi', avi, '--anim_size', '96x64', '--avi_quality', '75')
    assert sorted(os.listdir(tmp_path)) == ['joints.npy', 'out.avi']
    got = walk_avi(avi)
    assert (got['frames'], got['width'], got['height'], got['rate_scale'], got['audio']) == (5, 96, 64, (20, 1), None)
    r = sk.SkeletonRenderer(sk.T2M_CHAINS, width=96, height=64)
    frames = r.render(torch.from_numpy(np.load(npy)).cuda()).cpu().numpy()
    r.close()
    assert got['video'] == [J.encode(f, 75, '4:2:0') for f in frames] and decode(got['video'][4]).size == (96, 64)


def test_mesh_tool_muxes_the_speech(tmp_path):
    """``tools/render_npz.py res_x.npz --smplx_model ... --avi out.avi --audio x.wav`` in a child process: the counterpart of
    ``add_audio_to_video``.  The stereo wav comes back mono at its own rate, cut to the video's length."""
    mpath, npz, wav, avi = (str(tmp_path / n) for n in ('model.npz', 'res_x.npz', 'x.wav', 'out.avi'))
    np.savez(mpath, **lbs_ref.synthetic_model(V=1031, shape_space=300, seed=13))
    rs = np.random.RandomState(2)
    np.savez(npz, betas=np.zeros(300), poses=lbs_ref.random_poses(4, 19, scale=0.2), expressions=0.5 * rs.randn(4, 100), trans=np.tile([[0.0, 1.0, 0.0]], (4, 1)))
    left = rs.randint(-20000, 20000, 11025).astype('<i2')                        # two equal channels: their mean is the channel, exactly
    with wave.open(wav, 'wb') as f:
        f.setnchannels(2), f.setsampwidth(2), f.setframerate(22050), f.writeframes(np.stack([left, left], axis=1).tobytes())
    out = run_tool('render_npz.py', npz, '--smplx_model', mpath, '--avi', avi, '--audio', wav, '--render_size', '96x64', '--render_fps', '25')
    assert '22050 Hz' in out and sorted(os.listdir(tmp_path)) == ['model.npz', 'out.avi', 'res_x.npz', 'x.wav']
    got = walk_avi(avi)
    assert (got['frames'], got['width'], got['height'], got['rate_scale'], got['audio_rate'], got['channels']) == (4, 96, 64, (25, 1), 22050, 1)
    assert [len(a) // 2 for a in got['audio']] == [882] * 4                      # 22050 / 25
    assert np.array_equal(np.frombuffer(b''.join(got['audio']), '<i2'), left[:4 * 882])
    assert all(decode(v).size == (96, 64) for v in got['video'])
