"""The C ABI, once for every export (no GPU).  meshdiffusion_amd/_lib.py reads its ctypes binding from include/meshdiffusion_hip.h:
the header, the binding and the built library must be one thing, and the header parser must refuse what it cannot type."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from meshdiffusion_amd import _lib


def test_every_prototype_resolves_in_the_library_with_the_derived_types(hip_lib):
    raw = C.CDLL(_lib.LIB_PATH)
    for header, table, optional in (("meshdiffusion_hip.h", _lib.SIGNATURES, False),
                                    ("meshdiffusion_hip_experimental.h", _lib.ABLATION_SIGNATURES, True)):
        text = open(os.path.join(ROOT, "include", header)).read()
        # names and argument counts once more without the parser: plain searches of the header's text, comments included
        declared = set(re.findall(r"\b(md_[a-z0-9_]+)\s*\(", text))
        assert table and (declared >= set(table) if optional else declared == set(table)), declared ^ set(table)
        for name, (res, args) in table.items():
            params = re.search(rf"\b(?:int|int64_t|void) {name}\(([^;]*)\);", text).group(1)
            assert len(args) == (0 if params.strip() == "void" else len(params.split(","))), name
            if hasattr(raw, name) or not optional:          # the experimental header counts where the library exports it
                fn = getattr(hip_lib, name)
                assert hasattr(raw, name) and fn.restype is res and list(fn.argtypes) == args, name
    # the slots a hand-written table gets wrong silently: 64-bit sizes, doubles, the two kinds of struct pointer
    sig = _lib.SIGNATURES
    assert sig["md_gemm_conv"] == (C.c_int, [C.POINTER(_lib.MdGemmConvArgs), C.c_void_p])            # a struct in host memory
    assert sig["md_pack_batch"][1] == [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p]      # jobs_dev: a device array
    assert sig["md_packed_weight_bytes"][0] is C.c_int64 and sig["md_gn_apply"][1][-3:] == [C.c_float, C.c_uint64, C.c_void_p]
    assert sig["md_adam_ema_step_d"][1][5:13] == [C.c_int64] + [C.c_double] * 5 + [C.c_int32, C.c_double]
    # every MD_X of the header is X here; computed defines are evaluated; WINO_FMT is written in the header's terms
    assert (_lib.OK, _lib.ERR_BAD_ARG, _lib.CFG_C3_128, _lib.CFG_C3_128_FAST, _lib.CFG_G1_128_N128, _lib.CFG_COUNT) == (0, -1, 0, 14, 22, 23)
    assert _lib.SDF_REG_WORKSPACE_BYTES == 64 * 24 and _lib.LAPLACE_WORKSPACE_BYTES == 64 * 8
    assert _lib.WINO_FMT == {False: _lib.WINO_FMT_BF16X3, "f8": _lib.WINO_FMT_F16F8, "f6": _lib.WINO_FMT_F16F6} == {False: 0, "f8": 1, "f6": 2}
    with pytest.raises(_lib.MeshDiffusionHipError, match="no_such_header.h not found"):
        _lib._read("no_such_header.h")


def test_library_header_and_binding_are_one_abi_version(hip_lib):
    assert _lib.ABI_VERSION == hip_lib.md_abi_version() == 16


def test_cfg_table_comes_from_the_library(hip_lib):
    info = _lib.cfg_info(_lib.CFG_C3_128)
    assert info["taps"] == 27 and info["lds_bytes"] <= 160 * 1024 and info["threads"] == 512
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert " T md_gemm_conv" in nm
    table = _lib.CFG_NT_KC
    product = {c: v for c, v in table.items() if c < _lib.CFG_COUNT}
    assert len(product) == 20 and not {11, 12, 13} & set(product)                  # the reserved ids are unknown to the library
    assert hasattr(hip_lib, "md_wgrad_set_debug") == (len(table) > len(product))    # timing ids: ablation builds only
    assert table[_lib.CFG_C3_128] == (128, 32) and table[_lib.CFG_C3_128_K16] == (128, 16) and table[_lib.CFG_C3_32] == (32, 32)
    assert table[_lib.CFG_G1_64_LOW] == (64, 32) and table[_lib.CFG_C5X_32_K16] == (32, 16) and table[_lib.CFG_C3_128_FAST] == (128, 32)
    for cfg, (nt, kc) in table.items():
        assert (nt, kc) == (_lib.cfg_info(cfg)["nt"], _lib.cfg_info(cfg)["kc"]) and nt in (32, 64, 128) and kc in (16, 32)


# ---- the parser on synthetic header text: pure Python, no library ------------------------------------------------------
GOOD = """
/* a comment with md_not_a_prototype(int) and
#define MD_NOT 1 in it */
#define GUARD_H
#include <stdint.h>
extern "C" {
#define MD_A 4            // a line comment
#define MD_BYTES (MD_A * 24)
enum { MD_E0 = 0, MD_E1, MD_E5 = MD_A + 1, MD_NEG = (-2) };
typedef struct MdThing {
  const float* w;      /* pointer */
  int64_t s_row, s_k;
  double alpha;
} MdThing;
int md_version(void); void md_set(int32_t flags);
int64_t md_bytes(const MdThing* args, int64_t n, uint32_t* bits, const uint8_t* mask,
                 float eps, double lr, uint64_t seed, void* stream);
int md_batch(const MdThing* things_dev, int n);
}
"""


def test_parser_reads_a_well_formed_header():
    sigs, structs, consts = _lib.parse_header(GOOD)
    thing = structs["MdThing"]
    assert list(structs) == ["MdThing"] and issubclass(thing, C.Structure)
    assert thing._fields_ == [("w", C.c_void_p), ("s_row", C.c_int64), ("s_k", C.c_int64), ("alpha", C.c_double)]
    assert sigs == {
        "md_version": (C.c_int, []), "md_set": (None, [C.c_int32]), "md_batch": (C.c_int, [C.c_void_p, C.c_int]),
        "md_bytes": (C.c_int64, [C.POINTER(thing), C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_double, C.c_uint64, C.c_void_p])}
    assert consts == {"A": 4, "BYTES": 96, "E0": 0, "E1": 1, "E5": 5, "NEG": -2}           # a computed define evaluates
    # a second header sees the structs and constants of the one it includes
    more = _lib.parse_header("#define MD_TWICE (MD_BYTES * 2)\nint md_more(MdThing* t);", structs, consts)
    assert more[0] == {"md_more": (C.c_int, [C.POINTER(thing)])} and more[2]["TWICE"] == 192 and "TWICE" not in consts


@pytest.mark.parametrize("text,named", [
    ("int md_f(long n);", "long"), ("long md_f(int n);", "long"), ("int md_f(unsigned int n);", "unsigned int n"),   # unknown types
    ("int md_f(MdOther* p);", "MdOther"),                                       # a struct the header does not declare
    ("int md_f(void (*cb)(int), void* stream);", "md_f"),                       # a function-pointer parameter
    ("int md_f(int32_t dims[3]);", "dims[3]"), ("int md_f(float** rows);", "float** rows"),                          # an array parameter
    ("int md_f(int32_t a, int32_t b)\nint md_g(void);", "md_f"), ("int md_f(int32_t a,", "md_f"),                    # md_f( without a complete prototype
    ("int md_g(void); int x = md_f(3);", "md_f"), ("static inline int md_f(int a) { return a; }", "md_f"),
    ("int md_f(void); int md_f(void);", "md_f"),                                # declared twice
    ("#define MD_X 1.5", "MD_X"), ("#define MD_X \"text\"", "MD_X"), ("#define MD_X 0x10", "MD_X"), ("#define MD_X", "MD_X"),   # non-integer defines
    ("#define MD_X(a) ((a) * 2)", "MD_X"), ("#define MD_X (MD_LATER * 2)\n#define MD_LATER 1", "MD_LATER"),
    ("#define MD_X 1\n#define MD_X 2", "MD_X"), ("#define MD_X (1 + \\\n 2)", "MD_X"), ("enum { MD_A = 1.5 };", "MD_A"),
    ("typedef struct MdS { long n; } MdS;", "long"), ("typedef struct MdS { int32_t a[4]; } MdS;", "a[4]"),          # struct members it cannot type
    ("typedef struct MdS { float *a, b; } MdS;", "float *a, b"), ("typedef struct MdS { int32_t a : 3; } MdS;", "a : 3"),
    ("typedef int32_t md_index;", "md_index"), ('extern "C" {\nint md_f(void);', "md_f"),                            # nothing but enums, structs, prototypes
])
def test_parser_refuses_what_it_cannot_type(text, named):
    with pytest.raises(_lib.MeshDiffusionHipError) as err:
        _lib.parse_header(text)
    assert named in str(err.value), str(err.value)
