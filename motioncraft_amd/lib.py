"""ctypes binding of libmotioncraft_amd.so, derived from the one definition of the C-ABI: include/motioncraft_amd.h.

The header is read once when this module is imported: its constants, structs and prototypes become ``CONSTANTS``, ``STRUCTS`` and
``FUNCTIONS``, and nothing of the ABI is restated here.  A declaration the parser cannot type is an ``ImportError`` naming it.

The library is the product: there is no CPU or eager-PyTorch fallback.  Importing this module succeeds without the library (so
configs/registries can be used on a CPU box), but any attempt to run the path raises ``RuntimeError`` when the HIP library is missing
or no MI355X is visible.
"""
import ctypes
import os
import re

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libmotioncraft_amd.so')
HEADER_PATH = os.path.join(_HERE, '..', 'include', 'motioncraft_amd.h')

_SCALARS = {'void': None, 'char': ctypes.c_char, 'int': ctypes.c_int, 'float': ctypes.c_float, 'double': ctypes.c_double,
            **{f'{u}int{bits}_t': getattr(ctypes, f'c_{u}int{bits}') for u in ('', 'u') for bits in (8, 16, 32, 64)}}


def parse_header(text):
    """``(constants, structs, functions)`` of a header in the dialect of include/motioncraft_amd.h and nothing more: comments,
    preprocessor lines (``#define NAME <integer>`` is a constant), ``enum { NAME = <integer>, ... };``, opaque ``typedef struct X X;``,
    ``typedef struct X { fields } X;`` (several declarators per field, pointers, arrays of numeric or macro dimensions) and prototypes of
    ``mc_*`` functions (``(void)``, array parameters, ``T**``).  Scalars are typed by name, ``char*`` is ``c_char_p``, a pointer to a
    struct of the header is ``POINTER`` of it and every other pointer ``c_void_p``."""
    consts, structs, funcs, types = {}, {}, {}, dict(_SCALARS)

    def fail(why, decl):
        raise ImportError(f'C-ABI header: {why} in `{decl}`')

    def integer(word, decl):
        try:
            return consts[word] if word in consts else int(word, 0)
        except ValueError:
            fail(f'{word!r} is not an integer', decl)

    def ctype(base, stars, decl, void_ok=False):
        if base not in types:
            fail(f'unknown type {base!r}', decl)
        if stars:
            return ctypes.c_char_p if (base, stars) == ('char', 1) else ctypes.POINTER(types[base]) if stars == 1 and base in structs \
                else ctypes.c_void_p
        if types[base] is None and not void_ok:
            fail(f'a value of incomplete type {base!r}', decl)
        return types[base]

    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    text = re.sub(r'^[ \t]*#[ \t]*ifdef __cplusplus\n.*?^[ \t]*#[ \t]*endif', ' ', text, flags=re.S | re.M)       # extern "C" { and }
    for name, value in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S[^\n]*?)[ \t]*$', text, re.M):
        consts[name] = integer(value, f'#define {name} {value}')
    *statements, rest = re.split(r';(?![^{]*\})', re.sub(r'^[ \t]*#[^\n]*$', ' ', text, flags=re.M))
    if rest.strip():
        fail('unparsed statement', ' '.join(rest.split()))
    for s in statements:
        s = ' '.join(s.split())
        if m := re.fullmatch(r'enum \{(.*)\}', s):
            for item in m[1].split(','):
                name, _, value = (w.strip() for w in item.partition('='))
                consts[name] = integer(value, s)
        elif m := re.fullmatch(r'typedef struct (\w+) \1', s):
            types[m[1]] = None
        elif m := re.fullmatch(r'typedef struct (\w+) \{(.*)\} \1', s):
            fields = []
            for f in filter(None, (f.strip() for f in m[2].split(';'))):
                decl = f'{f}; of {m[1]}'
                fm = re.fullmatch(r'(?:const )?(\w+) ?(\**) ?(.+)', f) or fail('unparsed field', decl)
                for d in fm[3].split(','):
                    dm = re.fullmatch(r'(\w+)((?:\[\w+\])*)', d.strip()) or fail('unparsed field', decl)
                    t = ctype(fm[1], len(fm[2]), decl)
                    for dim in reversed(re.findall(r'\w+', dm[2])):
                        t = t * integer(dim, decl)
                    fields.append((dm[1], t))
            structs[m[1]] = types[m[1]] = type(m[1], (ctypes.Structure,), {'_fields_': fields})
        elif m := re.fullmatch(r'(?:const )?(\w+) ?(\**) ?(\w+) ?\((.*)\)', s):
            if not m[3].startswith('mc_'):
                fail(f'{m[3]!r} is not an mc_* function', s)
            args = []
            for p in m[4].split(',') if m[4].strip() != 'void' else ():
                pm = re.fullmatch(r'(?:const )?(\w+) ?(\**) ?\w*((?:\[\w*\])*)', p.strip()) or fail(f'unparsed parameter {p.strip()!r}', s)
                args.append(ctype(pm[1], len(pm[2]) + bool(pm[3]), s))
            funcs[m[3]] = (ctype(m[1], len(m[2]), s, void_ok=True), args)
        else:
            fail('unparsed statement', s)
    return consts, structs, funcs


with open(HEADER_PATH) as _f:
    CONSTANTS, STRUCTS, FUNCTIONS = parse_header(_f.read())
globals().update(CONSTANTS)                   # every constant of the header under its own name: MC_OK, MC_PREC_F16, MC_RENDER_MAX_SIZE, ...


def named(prefix):
    """the constants ``<prefix>NAME`` as ``{'name': value}``: the codes of one argument, e.g. ``named('MC_PREC_')``"""
    return {k[len(prefix):].lower(): v for k, v in CONSTANTS.items() if k.startswith(prefix)}


ModelConfig = STRUCTS['mc_model_config']
StepCoefs = STRUCTS['mc_step_coefs']
Inpaint = STRUCTS['mc_inpaint']
Seed = STRUCTS['mc_seed']
GemmStrided = STRUCTS['mc_gemm_strided']
EvalEncConfig = STRUCTS['mc_evalenc_config']
T2MEvalConfig = STRUCTS['mc_t2meval_config']
SMPLXConfig = STRUCTS['mc_smplx_config']
TextEncConfig = STRUCTS['mc_textenc_config']
RenderParams = STRUCTS['mc_render_params']
SkeletonParams = STRUCTS['mc_skeleton_params']
EXPORTED_SYMBOLS = tuple(FUNCTIONS)
NATIVE_OBJECTS = tuple(n[3:-len('_set_param')] for n in FUNCTIONS if n.endswith('_set_param'))       # the handles with a parameter store
MC_OK, MAX_TRANSL, POST_MAXTAP, SKELETON_MAX_LAYERS = (CONSTANTS[n] for n in ('MC_OK', 'MC_MAX_TRANSL', 'MC_POST_MAXTAP', 'MC_SKELETON_MAX_LAYERS'))
TEMPORAL_FORMS = named('MC_TEMPORAL_')        # mc_op_temporal_attention's form
ENC_ATTN_FORMS = named('MC_ENC_ATTN_')        # mc_op_enc_attention's form
GM_PLAIN, GM_ENC = CONSTANTS['MC_GM_PLAIN'], CONSTANTS['MC_GM_ENC']                                 # mc_op_gemm_strided's mode
ACT_NONE, ACT_GELU, ACT_SILU, ACT_LRELU, ACT_QUICKGELU = (CONSTANTS[f'MC_ACT_{n}'] for n in ('NONE', 'GELU', 'SILU', 'LRELU', 'QUICKGELU'))

_lib = None


def load(require_gpu=False):
    """Load the shared library (no compute call).  Raises RuntimeError if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f'{LIB_PATH} not found: build it with `python -m motioncraft_amd.build` '
                '(hipcc --offload-arch=gfx950). There is no CPU fallback for this path.')
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in FUNCTIONS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    if require_gpu:
        n = ctypes.c_int(0)
        rc = _lib.mc_device_count(ctypes.byref(n))
        if rc != MC_OK or n.value < 1:
            raise RuntimeError('motioncraft_amd: no HIP device visible (the hot path runs on MI355X only): '
                               + last_error())
    return _lib


def last_error():
    return (_lib.mc_last_error() or b'').decode() if _lib is not None else ''


def check(rc, what=''):
    if rc != MC_OK:
        raise RuntimeError(f'motioncraft_amd {what} failed (code {rc}): {last_error()}')


def ptr(t):
    """the address of a tensor's first element as the ``void*`` the entry points take; None is NULL"""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream(device=None):
    """torch's current stream on ``device`` (None: the current device) as the ``void* stream`` the entry points take"""
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class NativeObject:
    """Owner of one handle of kind ``mc_<kind>`` (``NATIVE_OBJECTS``): created from ``cfg_args`` (mc_<kind>_create's
    arguments before the out handle), filled by ``upload``, made usable by ``finalize``, freed by ``close``."""
    handle = None                             # stays None when create fails: close() and __del__ then do nothing

    def __init__(self, kind, *cfg_args):
        self.lib, self.kind = load(require_gpu=True), kind
        h = ctypes.c_void_p()
        check(getattr(self.lib, f'mc_{kind}_create')(*cfg_args, ctypes.byref(h)), f'mc_{kind}_create')
        self.handle = h

    def upload(self, items):
        """(name, array) pairs -> mc_<kind>_set_param, as contiguous float32 host arrays."""
        set_param = getattr(self.lib, f'mc_{self.kind}_set_param')
        for name, a in items:
            a = np.ascontiguousarray(a, dtype=np.float32)
            check(set_param(self.handle, name.encode(), a.ctypes.data_as(ctypes.c_void_p), a.size), f'mc_{self.kind}_set_param({name})')

    def finalize(self):
        check(getattr(self.lib, f'mc_{self.kind}_finalize')(self.handle), f'mc_{self.kind}_finalize')

    def close(self):
        if self.handle:
            getattr(self.lib, f'mc_{self.kind}_destroy')(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
