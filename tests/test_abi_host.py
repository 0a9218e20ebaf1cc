"""CPU: the ctypes bindings are derived from include/motioncraft_amd.h (lib.parse_header).  The parser on one snippet per construct
of the header's dialect, the derived struct layouts and constants against the C compiler, and the built library's dynamic symbols
against the header's prototypes."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from motioncraft_amd import build, lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'motioncraft_amd.h')


def test_comments_preprocessor_lines_and_constants():
    consts, structs, funcs = lib.parse_header('''
        /* a block comment ; with { a brace
           over two lines */
        #ifndef GUARD_H          // a line comment ; }
        #define GUARD_H
        #include <stdint.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define MC_A 3
        #define MC_B 0x10        /* hexadecimal */
        #define MC_C MC_A
        enum { MC_D = 0,         /* first */
               MC_E = 5, MC_F = MC_B };
        #ifdef __cplusplus
        }
        #endif
        #endif /* GUARD_H */
    ''')
    assert consts == dict(MC_A=3, MC_B=16, MC_C=3, MC_D=0, MC_E=5, MC_F=16) and not structs and not funcs


def test_opaque_handles_and_out_handles():
    _, structs, funcs = lib.parse_header('typedef struct mc_h mc_h;\nint mc_h_create(int32_t n, mc_h** out);\nvoid mc_h_destroy(mc_h* h);\n'
                                         'int64_t mc_h_bytes(const mc_h* h);')
    assert not structs
    assert funcs == dict(mc_h_create=(ctypes.c_int, [ctypes.c_int32, ctypes.c_void_p]), mc_h_destroy=(None, [ctypes.c_void_p]),
                         mc_h_bytes=(ctypes.c_int64, [ctypes.c_void_p]))


def test_struct_fields_multi_declarator_pointer_and_arrays():
    consts, structs, _ = lib.parse_header('''
        #define MC_N 8
        typedef struct mc_s {
            const float* a_dev; int64_t lda, a_gstride;      /* a pointer and two declarators on one line */
            uint8_t flag;
            int32_t width, height;
            float screen[12];
            int32_t channel[MC_N];
            float value[MC_N][2];
            double d;
        } mc_s;''')

    class Hand(ctypes.Structure):
        _fields_ = [('a_dev', ctypes.c_void_p), ('lda', ctypes.c_int64), ('a_gstride', ctypes.c_int64), ('flag', ctypes.c_uint8),
                    ('width', ctypes.c_int32), ('height', ctypes.c_int32), ('screen', ctypes.c_float * 12), ('channel', ctypes.c_int32 * 8),
                    ('value', (ctypes.c_float * 2) * 8), ('d', ctypes.c_double)]
    s = structs['mc_s']
    assert [n for n, _ in s._fields_] == [n for n, _ in Hand._fields_] and ctypes.sizeof(s) == ctypes.sizeof(Hand) == 192
    for name, _ in Hand._fields_:
        assert (getattr(s, name).offset, getattr(s, name).size) == (getattr(Hand, name).offset, getattr(Hand, name).size), name
    v = s()
    v.value[7][1], v.a_dev = 2.5, 4096
    assert v.value[7][1] == 2.5 and len(v.value) == 8 and len(v.value[0]) == 2 and v.a_dev == 4096


def test_prototypes_multi_line_void_array_parameter_and_pointer_kinds():
    _, structs, funcs = lib.parse_header('''
        typedef struct mc_s { int32_t n; } mc_s;
        typedef struct mc_h mc_h;
        const char* mc_name(void);
        int mc_f(mc_h* h, const int32_t radius[4], const char* key,
                 const mc_s* s, double x,
                 uint64_t seed, float y, uint8_t* bytes_dev, void* stream);''')
    assert funcs['mc_name'] == (ctypes.c_char_p, [])
    res, args = funcs['mc_f']
    assert res is ctypes.c_int and args[:3] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p] and args[3]._type_ is structs['mc_s']
    assert args[4:] == [ctypes.c_double, ctypes.c_uint64, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]


@pytest.mark.parametrize('snippet, names', [
    ('int mc_f(size_t n, int32_t m);', ('size_t', 'mc_f')),                                      # unknown type of a parameter
    ('typedef struct mc_s { int32_t n; unsigned flags; } mc_s;', ('unsigned', 'flags', 'mc_s')),  # ... of a field
    ('mc_result mc_f(void);', ('mc_result', 'mc_f')),                                            # ... of a result
    ('int mc_f(int a);\nstatic int mc_x = 3;\nint mc_g(int a);', ('unparsed', 'mc_x')),           # a statement between two `;`
    ('int mc_f(int a);\nint mc_g(int a)', ('unparsed', 'mc_g')),                                   # ... and after the last one
    ('int mc_f(unsigned int a);', ('unparsed', 'unsigned int a', 'mc_f')),
    ('int mc_f(int a);\nint other_f(int a);', ('other_f',)),                                      # a prototype that is not mc_*
    ('#define MC_A (1 << 4)', ('MC_A',)),                                                         # a constant that is no integer
    ('typedef struct mc_h mc_h;\nint mc_f(mc_h h);', ('mc_h', 'mc_f')),                           # an opaque struct by value
])
def test_what_the_parser_cannot_type_is_an_import_error_naming_the_declaration(snippet, names):
    with pytest.raises(ImportError) as e:
        lib.parse_header(snippet)
    assert all(n in str(e.value) for n in names), str(e.value)


def test_header_surface_and_public_names():
    """every prototype, struct and constant of the header is bound, and the names the package uses are bindings to them"""
    hdr = open(HEADER).read()
    assert set(lib.FUNCTIONS) == set(re.findall(r'\b(mc_[a-z_0-9]+)\s*\(', hdr)) and len(lib.FUNCTIONS) >= 109
    assert set(lib.STRUCTS) == set(re.findall(r'\}\s*(mc_\w+)\s*;', hdr)) and len(lib.STRUCTS) >= 11
    assert set(re.findall(r'#define\s+(MC_\w+)\s+\S', hdr)) <= set(lib.CONSTANTS)
    assert all(getattr(lib, k) == v for k, v in lib.CONSTANTS.items())
    assert lib.ModelConfig is lib.STRUCTS['mc_model_config'] and lib.SkeletonParams is lib.STRUCTS['mc_skeleton_params']
    assert lib.NATIVE_OBJECTS == ('model', 'textenc', 'evalenc', 't2meval', 'wavenc', 'smplx')
    assert (lib.MC_OK, lib.MAX_TRANSL, lib.POST_MAXTAP, lib.SKELETON_MAX_LAYERS) == (0, 8, 129, 64)
    assert lib.TEMPORAL_FORMS == dict(step=0, whole=1, lsplit=2, pair=3, f16x3=4, f16=5) and lib.ENC_ATTN_FORMS == dict(layer=0, small=1, stream=2)
    assert (lib.GM_PLAIN, lib.GM_ENC) == (0, 4) and (lib.ACT_NONE, lib.ACT_GELU, lib.ACT_SILU, lib.ACT_LRELU, lib.ACT_QUICKGELU) == (0, 1, 2, 3, 4)
    assert lib.named('MC_PREC_') == dict(f32=0, f16=1, f16x3=2) and lib.named('MC_TIE_') == dict(stable=0, reverse=1)
    assert lib.FUNCTIONS['mc_last_error'] == (ctypes.c_char_p, []) and lib.FUNCTIONS['mc_ctx_workspace_bytes'] == (ctypes.c_int64, [ctypes.c_void_p])
    seed = lib.Seed()
    assert len(seed.transl_value) == lib.MAX_TRANSL and len(seed.transl_value[0]) == 2 and len(lib.RenderParams().screen) == 12


def test_derived_layouts_and_constants_agree_with_the_c_compiler(tmp_path):
    """a host program that includes the header prints sizeof and every offsetof, and every constant; the derived classes say the same"""
    try:
        cc = build._hipcc()
    except RuntimeError:
        pytest.skip('no compiler')
    lines = ['#include <stddef.h>', '#include <stdio.h>', f'#include "{HEADER}"', 'int main(void) {']
    for name, cls in lib.STRUCTS.items():
        lines.append(f'    printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'    printf("{name}.{f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));' for f, _ in cls._fields_]
    lines += [f'    printf("{name} %lld\\n", (long long)({name}));' for name in lib.CONSTANTS]
    src, exe = tmp_path / 'abi_layout.cpp', tmp_path / 'abi_layout'
    src.write_text('\n'.join(lines + ['    return 0;', '}', '']))
    subprocess.run([cc, '-x', 'c++', str(src), '-o', str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    derived = []
    for name, cls in lib.STRUCTS.items():
        derived.append(f'{name} {ctypes.sizeof(cls)}')
        derived += [f'{name}.{f} {getattr(cls, f).offset} {getattr(cls, f).size}' for f, _ in cls._fields_]
    derived += [f'{name} {value}' for name, value in lib.CONSTANTS.items()]
    assert len(out) > len(lib.STRUCTS) + len(lib.CONSTANTS) and out == derived, [(a, b) for a, b in zip(out, derived) if a != b]


def test_the_library_defines_exactly_the_headers_entry_points():
    """the reverse of test_host's check: no mc_* dynamic function symbol of the built library is missing from the header (the header
    declares functions only, so data symbols are not its business)"""
    nm = shutil.which('nm')
    if nm is None:
        pytest.skip('no nm')
    lib.load(require_gpu=False)
    out = subprocess.run([nm, '-D', '--defined-only', lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.split()[-2] == 'T' and line.split()[-1].startswith('mc_')}
    assert defined == set(lib.EXPORTED_SYMBOLS), defined ^ set(lib.EXPORTED_SYMBOLS)
