"""GPU: the weight handling that the denoiser model and the four encoders share (mc_params.h, lib.NativeObject), at small
sizes: a missing or mis-sized parameter fails finalize with a message that names the object, the parameter and the
expected size; no forward call runs before finalize; an encoder accepts new weights after finalize and refuses to run
until it is finalized again, after which (and after any repeated finalize) its output is bit-identical; the model refuses
new weights once finalized and keeps working."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import EVAL_BERT, EVAL_DIMS, SMALL, SMALL_SEED, T2M_DIMS, T2M_TEXT, synth_inputs
from motioncraft_amd import lib as L
from oracle import weights as W

pytestmark = pytest.mark.gpu

ENCODERS = ('textenc', 'evalenc', 't2meval', 'wavenc')


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(items):
    return [(k, np.ascontiguousarray(v, dtype=np.float32)) for k, v in items]


# Each spec: `obj` a finalized wrapper; `args` its create arguments; `items` the parameters it uploaded; `forward(o)` runs
# the object's forward calls on any NativeObject `o` of that kind -> (return code, outputs); `ref` = forward(obj) outputs;
# `missing` / `short` the parameters the error cases leave out / shorten; `label` the prefix of the object's lookup errors.
def _model():
    from motioncraft_amd.engine import NativeModel
    from motioncraft_amd.weights import pack_state_dict
    sd = W.make_state_dict(SMALL, SMALL_SEED)
    nm = NativeModel(SMALL, sd, cfg_scale=SMALL['scale'])

    def forward(o):                    # the model's forward calls all go through a context
        h = ctypes.c_void_p()
        rc = o.lib.mc_ctx_create(o.handle, 2, 24, 1, ctypes.byref(h))
        if rc == L.MC_OK:
            o.lib.mc_ctx_destroy(h)
        return rc, []
    return SimpleNamespace(kind='model', obj=nm, args=(ctypes.byref(nm.cfg),), items=_f32(pack_state_dict(sd, SMALL).items()),
                           forward=forward, missing='l1.ffn.w2', short='enc.b', label='')


def _textenc():
    from motioncraft_amd.text_encoder import NativeTextEncoder
    shapes = W.text_encoder_param_shapes(128, 1, 256, clip_width=64, clip_layers=1, clip_ff=128, vocab=100)
    sd = W.make_text_encoder_state(shapes, seed=5)
    enc = NativeTextEncoder(dict(latent_dim=128, num_layers=1, ff_size=256, num_heads=2), sd,
                            clip=dict(width=64, layers=1, heads=1, ff=128))
    tokens = torch.randint(0, 100, (2, 77), generator=torch.Generator().manual_seed(1)).to(torch.int32).cuda()

    def forward(o):
        feat, xf = torch.empty(2, 77, 64, device='cuda'), torch.empty(2, 77, 128, device='cuda')
        return o.lib.mc_textenc_forward_tokens(o.handle, _p(tokens), 2, _p(feat), _p(xf), _stream()), [feat, xf]
    return SimpleNamespace(kind='textenc', obj=enc, args=(ctypes.byref(enc.cfg),), items=_f32(sd.items()), forward=forward,
                           missing='clip.transformer.resblocks.0.mlp.c_proj.weight', short='textTransEncoder.layers.0.linear1.bias',
                           label='text encoder: ')


def _evalenc():
    from motioncraft_amd.evaluation import NativeEvalEncoder
    bert = dict(EVAL_BERT, vocab_size=100)
    sd = W.make_eval_encoder_state(W.eval_encoder_param_shapes(bert=bert, **EVAL_DIMS), seed=6)
    enc = NativeEvalEncoder(sd, bert=bert, **EVAL_DIMS)
    g = torch.Generator().manual_seed(2)
    motion = torch.randn(2, 8, EVAL_DIMS['nfeats'], generator=g).cuda()
    lengths = torch.tensor([8, 5], dtype=torch.int32).cuda()
    ids = torch.randint(0, 100, (2, 6), generator=g).to(torch.int32).cuda()
    mask = torch.tensor([[1] * 6, [1] * 4 + [0] * 2], dtype=torch.uint8).cuda()

    def forward(o):
        mu, tu = (torch.empty(2, EVAL_DIMS['latent_dim'], device='cuda') for _ in range(2))
        rc = o.lib.mc_evalenc_encode_motion(o.handle, _p(motion), _p(lengths), 2, 8, _p(mu), _stream())
        if rc == L.MC_OK:
            rc = o.lib.mc_evalenc_encode_text(o.handle, _p(ids), _p(mask), 2, 6, _p(tu), _stream())
        return rc, [mu, tu]
    return SimpleNamespace(kind='evalenc', obj=enc, args=(ctypes.byref(enc.cfg),), items=_f32(sd.items()), forward=forward,
                           missing='textencoder.text_model.transformer.layer.1.attention.k_lin.weight', short='motionencoder.mu_token',
                           label='evaluation encoder: ')


def _t2meval():
    from motioncraft_amd.evaluation import NativeT2MEvaluator
    sd = W.make_t2m_eval_state(W.t2m_eval_param_shapes(**T2M_DIMS, **T2M_TEXT), seed=7)
    enc = NativeT2MEvaluator(sd, **T2M_DIMS, **T2M_TEXT)
    g = torch.Generator().manual_seed(3)
    motion = torch.randn(2, 16, T2M_DIMS['input_size'], generator=g).cuda()
    lengths = torch.tensor([16, 9], dtype=torch.int32).cuda()
    word = torch.randn(2, 5, T2M_TEXT['word_size'], generator=g).cuda()
    pos = torch.nn.functional.one_hot(torch.randint(0, T2M_TEXT['pos_size'], (2, 5), generator=g), T2M_TEXT['pos_size']).float().cuda()
    sent = torch.tensor([5, 3], dtype=torch.int32).cuda()

    def forward(o):
        me = torch.empty(2, T2M_DIMS['motion_latent_size'], device='cuda')
        te = torch.empty(2, T2M_TEXT['output_size'], device='cuda')
        rc = o.lib.mc_t2meval_encode_motion(o.handle, _p(motion), _p(lengths), 2, 16, _p(me), _stream())
        if rc == L.MC_OK:
            rc = o.lib.mc_t2meval_encode_text(o.handle, _p(word), _p(pos), _p(sent), 2, 5, _p(te), _stream())
        return rc, [me, te]
    return SimpleNamespace(kind='t2meval', obj=enc, args=(ctypes.byref(enc.cfg),), items=_f32(sd.items()), forward=forward,
                           missing='text_encoder.gru.weight_hh_l0_reverse', short='movement_encoder.main.3.bias',
                           label='t2m evaluator: ')


def _wavenc():
    from motioncraft_amd.wav_encoder import NativeWavEncoder, pack_wav_encoder
    sd = W.make_wav_encoder_state(64, 2, seed=8)
    enc = NativeWavEncoder(64, 2, sd)
    wav = torch.randn(2, 2000, 2, generator=torch.Generator().manual_seed(4)).cuda()
    frames = enc.out_len(2000)

    def forward(o):
        out = torch.empty(2, frames, 64, device='cuda')
        return o.lib.mc_wavenc_forward(o.handle, _p(wav), 2, 2000, _p(out), _stream()), [out]
    return SimpleNamespace(kind='wavenc', obj=enc, args=(2, 64), items=_f32((k, v.numpy()) for k, v in pack_wav_encoder(sd).items()),
                           forward=forward, missing='b5.down.w', short='b2.conv2.b', label='wav encoder: ')


_BUILD = dict(model=_model, textenc=_textenc, evalenc=_evalenc, t2meval=_t2meval, wavenc=_wavenc)


@pytest.fixture(scope='module')
def specs():
    built = {}
    yield built
    for s in built.values():
        s.obj.close()


def _spec(specs, kind):
    if kind not in specs:
        s = _BUILD[kind]()
        rc, s.ref = s.forward(s.obj)
        assert rc == L.MC_OK, L.last_error()
        specs[kind] = s
    return specs[kind]


def _refused_before_finalize(s, o):
    rc, _ = s.forward(o)
    return rc != L.MC_OK and 'not finalized' in L.last_error()


def _same_as_ref(s, o):
    rc, out = s.forward(o)
    assert rc == L.MC_OK, L.last_error()
    return all(torch.equal(a, b) for a, b in zip(out, s.ref))


@pytest.mark.parametrize('kind', tuple(_BUILD))
def test_finalize_names_a_missing_parameter(specs, kind):
    s = _spec(specs, kind)
    o = L.NativeObject(kind, *s.args)
    o.upload((k, a) for k, a in s.items if k != s.missing)
    with pytest.raises(RuntimeError) as e:
        o.finalize()
    assert f"mc_{kind}_finalize failed (code 3): {s.label}missing parameter '{s.missing}'" in str(e.value)
    assert _refused_before_finalize(s, o)                  # a failed finalize leaves the object unusable
    o.close()


@pytest.mark.parametrize('kind', tuple(_BUILD))
def test_finalize_names_the_expected_element_count(specs, kind):
    s = _spec(specs, kind)
    n = dict(s.items)[s.short].size
    o = L.NativeObject(kind, *s.args)
    o.upload((k, a.ravel()[:-1] if k == s.short else a) for k, a in s.items)
    with pytest.raises(RuntimeError) as e:
        o.finalize()
    assert f"mc_{kind}_finalize failed (code 3): {s.label}parameter '{s.short}' has {n - 1} elements, expected {n}" in str(e.value)
    assert _refused_before_finalize(s, o)
    o.close()


@pytest.mark.parametrize('kind', tuple(_BUILD))
def test_nothing_runs_before_finalize(specs, kind):
    s = _spec(specs, kind)
    o = L.NativeObject(kind, *s.args)
    o.upload(s.items)
    assert _refused_before_finalize(s, o)                  # the model: mc_ctx_create
    o.finalize()
    assert _same_as_ref(s, o)
    o.close()


@pytest.mark.parametrize('kind', ENCODERS)
def test_encoder_set_param_after_finalize_needs_a_new_finalize(specs, kind):
    s = _spec(specs, kind)
    s.obj.upload(s.items[:1])
    assert _refused_before_finalize(s, s.obj)
    s.obj.upload(s.items)
    s.obj.finalize()
    assert _same_as_ref(s, s.obj)


@pytest.mark.parametrize('kind', ENCODERS)
def test_encoder_finalize_twice_is_exact(specs, kind):
    s = _spec(specs, kind)
    for _ in range(2):
        s.obj.finalize()                                   # rebuilds the derived buffers (evalenc, t2meval)
        assert _same_as_ref(s, s.obj)


def test_model_weights_are_immutable_once_finalized(specs):
    s = _spec(specs, 'model')
    nm = s.obj
    x, xf, mask = (t.cuda() for t in synth_inputs(SMALL, 2, 24, seed=9, lengths=[24, 17]))

    def denoise():
        ctx = nm.context(2, 24, max_steps=1)
        ctx.set_timesteps([640])
        ctx.set_condition(xf, mask)
        out = ctx.denoise(x, 0)
        ctx.close()
        return out
    before = denoise()
    name, a = s.items[0]
    with pytest.raises(RuntimeError, match=f'mc_model_set_param\\({name}\\): the model is finalized; weights are immutable'):
        nm.upload([(name, 2 * a)])
    assert torch.equal(denoise(), before)


def test_failed_create_leaves_nothing_to_close():
    o = L.NativeObject.__new__(L.NativeObject)
    with pytest.raises(RuntimeError, match=r'mc_wavenc_create failed \(code 1\)'):
        o.__init__('wavenc', 2, 10)                        # out_dim must be a multiple of 16
    assert o.handle is None
    o.close()
