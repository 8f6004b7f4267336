"""ctypes binding of libmeshdiffusion_hip.so, read from the C ABI's own declaration (include/meshdiffusion_hip.h).

At import the header is parsed (`parse_header`): its prototypes become SIGNATURES, its two structs the ctypes classes
MdGemmConvArgs / MdPackJob, and every `MD_X` constant the module attribute `X` (MD_CFG_C3_128 -> CFG_C3_128,
MD_ABI_VERSION -> ABI_VERSION, ...).  Nothing about an export is written down here a second time.

There is NO fallback: if the shared library is missing or an entry point fails, the caller
gets an exception.  PyTorch is only used by the callers for device memory and streams; every
argument that crosses this boundary is a raw device pointer or a plain integer/float.
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MD_LIB") or os.path.join(_HERE, "libmeshdiffusion_hip.so")   # MD_LIB: an A/B build (build.py MD_LIB_SUFFIX)
INCLUDE = os.path.join(os.path.dirname(_HERE), "include")                               # as build.py

_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
            "float": C.c_float, "double": C.c_double}
_POINTEES = set(_SCALARS) | {"void", "int8_t", "uint8_t"}     # a pointer to one of these is a c_void_p
_ENUM = re.compile(r"enum\s*\{([^{}]*)\}\s*;\s*")
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;\s*")
_PROTO = re.compile(r"(?:const\s+)?(\w+)\s*(\*?)\s*\b(md_\w+)\s*\(([^(){};]*)\)\s*;\s*")
_PARAM = re.compile(r"(?:const\s+)?(\w+)\s*(\*?)\s*(?:\b(\w+))?")
_MEMBER = re.compile(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+(?:\s*,\s*\w+)*)")


class MeshDiffusionHipError(RuntimeError):
    pass


def parse_header(text, structs=None, constants=None):
    """The C ABI declared by a header: ({name: (restype, [argtypes])}, {struct name: ctypes class}, {X: int} per MD_X).

    The accepted subset is the one written at the top of include/meshdiffusion_hip.h.  Whatever lies outside it raises
    MeshDiffusionHipError naming the text: after comments and preprocessor lines the header must be nothing but enums, structs and
    md_* prototypes, so no declaration can be passed over.  `structs` / `constants`: those of a header this one includes."""
    structs, constants, sigs = dict(structs or {}), dict(constants or {}), {}

    def fail(what, where):
        raise MeshDiffusionHipError(f"C header: {what}: {' '.join(where.split())[:120]!r}")

    def integer(expr, where):
        """An integer expression: decimal literals, earlier MD_ names, + - * and parentheses."""
        def known(m):
            if m.group(1) not in constants:
                fail(f"MD_{m.group(1)} is not defined earlier", where)
            return str(constants[m.group(1)])
        expr = re.sub(r"\bMD_(\w+)", known, expr)
        if not re.fullmatch(r"[\d\s()+*-]*\d[\d\s()+*-]*", expr) or "**" in expr:
            fail("not an integer expression", where)
        try:
            return int(eval(expr, {"__builtins__": {}}))
        except Exception:
            fail("not an integer expression", where)

    def ctype(base, star, where, device=False):
        if star:
            if base in structs and not device:
                return C.POINTER(structs[base])
            if base in _POINTEES or base in structs:
                return C.c_void_p
        elif base in _SCALARS:
            return _SCALARS[base]
        fail(f"unknown type {base + star!r}", where)

    def define(name, value, where):
        if not name.startswith("MD_"):
            fail("a constant's name must begin with MD_", where)
        if name[3:] in constants:
            fail(f"{name} is defined twice", where)
        constants[name[3:]] = value

    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    body = []
    for line in text.split("\n"):
        if line.rstrip().endswith("\\"):
            fail("line continuation", line)
        m = re.match(r"\s*#\s*define\s+(MD_\w+)(.*)", line)
        if m:                                        # a function-like macro fails here too: "(x) ..." is no integer expression
            define(m.group(1), integer(m.group(2), line), line)
        elif not line.lstrip().startswith("#"):      # include guard, #include, #ifdef __cplusplus: nothing of the ABI
            body.append(line)
    text = "\n".join(body)
    text, wrapped = re.subn(r'extern\s+"C"\s*\{', " ", text, count=1)
    if wrapped:
        if not text.rstrip().endswith("}"):
            fail('extern "C" { is not closed at the end', text[-80:])
        text = text.rstrip()[:-1]
    text, pos = text.strip(), 0
    while pos < len(text):
        rest = text[pos:pos + 400]
        if (m := _ENUM.match(text, pos)):
            value = -1
            for item in filter(None, (i.strip() for i in m.group(1).split(","))):
                name, eq, expr = (p.strip() for p in item.partition("="))
                if not re.fullmatch(r"\w+", name):
                    fail("enumerator", item)
                value = integer(expr, item) if eq else value + 1
                define(name, value, item)
        elif (m := _STRUCT.match(text, pos)):
            if m.group(1) != m.group(3) or m.group(1) in structs:
                fail("struct tag and typedef name differ, or the struct is declared twice", rest)
            fields = []
            for member in filter(None, (i.strip() for i in m.group(2).split(";"))):
                mm = _MEMBER.fullmatch(member)
                if not mm or (mm.group(2) and "," in mm.group(3)):
                    fail("struct member", member)
                fields += [(n.strip(), ctype(mm.group(1), mm.group(2), member)) for n in mm.group(3).split(",")]
            structs[m.group(1)] = type(m.group(1), (C.Structure,), {"_fields_": fields})
        elif (m := _PROTO.match(text, pos)):
            base, star, name, params = m.groups()
            if name in sigs:
                fail(f"{name} is declared twice", rest)
            args = []
            for param in ([] if params.strip() in ("", "void") else params.split(",")):
                pm = _PARAM.fullmatch(param.strip())
                if not pm:
                    fail(f"parameter of {name}", param)
                args.append(ctype(pm.group(1), pm.group(2), param, device=(pm.group(3) or "").endswith("_dev")))
            sigs[name] = (None if (base, star) == ("void", "") else ctype(base, star, rest), args)
        else:
            fail("not an enum, a struct or a complete md_* prototype", rest)
        pos = m.end()
    return sigs, structs, constants


def _read(name):
    path = os.path.join(INCLUDE, name)
    if not os.path.exists(path):
        raise MeshDiffusionHipError(f"{path} not found: the ctypes binding is read from the C header")
    with open(path) as f:
        return f.read()


# name -> (restype, argtypes); exactly the entry points of include/meshdiffusion_hip.h
SIGNATURES, _STRUCTS, CONSTANTS = parse_header(_read("meshdiffusion_hip.h"))
# include/meshdiffusion_hip_experimental.h: MD_BUILD_ABLATIONS=1 builds only; attached where the symbol exists
ABLATION_SIGNATURES = parse_header(_read("meshdiffusion_hip_experimental.h"), _STRUCTS, CONSTANTS)[0]
for _name in list(CONSTANTS) + list(_STRUCTS):
    if _name in globals():
        raise MeshDiffusionHipError(f"C header: {_name} would replace an attribute of {__name__}")
globals().update(CONSTANTS)      # CFG_*, OUT_*, PREC_*, PACK_*, ABI_VERSION, ...: MD_X of the header is X here
globals().update(_STRUCTS)       # MdGemmConvArgs, MdPackJob
WINO_FMT = {False: CONSTANTS["WINO_FMT_BF16X3"], "f8": CONSTANTS["WINO_FMT_F16F8"], "f6": CONSTANTS["WINO_FMT_F16F6"]}

# cfg -> (NT, KC) of every md_gemm_conv configuration id the loaded library knows; filled by load() from md_gemm_conv_cfg_info
CFG_NT_KC = {}
# timing-only ablation ids of C3_128_V2 / C3_128_FAST: known to MD_BUILD_ABLATIONS=1 libraries only (tools/bench_conv.py)
ABLATION_CFGS = (101, 102, 103, 104, 105, 111, 113, 114, 116, 117, 118, 122)

_lib = None


def load():
    """dlopen the library (once) and attach prototypes.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MeshDiffusionHipError(
            f"{LIB_PATH} not found: run `python -m meshdiffusion_amd.build` (needs hipcc). "
            "There is no CPU fallback for the HIP path.")
    # ORDER MATTERS: PyTorch bundles its own libamdhip64.so (SONAME libamdhip64.so.7).  Importing torch
    # first makes the dynamic linker satisfy our DT_NEEDED libamdhip64.so.7 with that already-loaded
    # copy, so torch and this library share ONE HIP runtime (streams, events and the null stream mean
    # the same thing on both sides).  Loading us first would pull in /opt/rocm's runtime next to
    # torch's and every launch would fail with hipErrorNoDevice.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in ABLATION_SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    abi = CONSTANTS["ABI_VERSION"]       # the library and the header this binding was read from belong together (MD_LIB builds too)
    if lib.md_abi_version() != abi:
        raise MeshDiffusionHipError(f"ABI version mismatch: library {lib.md_abi_version()}, header {abi}")
    ablation = all(hasattr(lib, name) for name in ABLATION_SIGNATURES)    # such a build knows the timing-only ids too
    for cfg in list(range(CONSTANTS["CFG_COUNT"])) + list(ABLATION_CFGS if ablation else ()):
        rc, info = _cfg_info(lib, cfg)
        if rc == CONSTANTS["OK"]:                # reserved ids answer MD_ERR_UNSUPPORTED
            CFG_NT_KC[cfg] = info[:2]
    if torch.cuda.is_available() and lib.md_device_count() != torch.cuda.device_count():
        raise MeshDiffusionHipError("libmeshdiffusion_hip.so is not sharing PyTorch's HIP runtime "
                                    f"({lib.md_device_count()} vs {torch.cuda.device_count()} devices)")
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        raise MeshDiffusionHipError(f"{what} failed with code {rc}")


def _cfg_info(lib, cfg):
    v = [C.c_int32() for _ in range(6)]
    rc = lib.md_gemm_conv_cfg_info(cfg, *[C.byref(x) for x in v])
    return rc, tuple(x.value for x in v)


def cfg_info(cfg):
    rc, info = _cfg_info(load(), cfg)
    check(rc, f"cfg_info({cfg})")
    return dict(zip(("nt", "kc", "cols", "taps", "lds_bytes", "threads"), info))
