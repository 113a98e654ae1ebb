"""CPU-side checks of the drop-in boundary: the in-tree library loads, exports every symbol
that include/deeplip_hip.h declares, and the ctypes binding covers exactly that set.
No compute call is made (there is no GPU in the build container)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


def header_symbols():
    text = open(os.path.join(ROOT, "include", "deeplip_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dlip_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from deeplip_amd import build
    path = build.build(verbose=False)
    lib = ctypes.CDLL(path)
    syms = header_symbols()
    assert len(syms) >= 18
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in deeplip_hip.h but not exported"


def test_binding_matches_header():
    from deeplip_amd import _lib
    assert sorted(list(_lib.SIGNATURES) + ["dlip_error_string", "dlip_source_sha"]) == header_symbols()
    l = _lib.lib()
    assert l.dlip_abi_version() == _lib.ABI_VERSION
    from deeplip_amd import build
    assert l.dlip_source_sha().decode() == build.source_sha() == build.library_sha()      # the library IS these sources
    assert l.dlip_error_string(0) == b"ok"
    assert b"invalid argument" in l.dlip_error_string(-1)


def test_debug_key_7_is_reserved():
    """Key 7 forced a retired experiment (the rows kernel's general mode): a positive value is refused, resetting it is accepted.
    Host-only: dlip_debug_set makes no device call."""
    from deeplip_amd import _lib
    l = _lib.lib()
    assert l.dlip_debug_set(_lib.DBG_ROWS2D, 1) != 0
    assert l.dlip_debug_set(_lib.DBG_ROWS2D, 0) == 0
    assert l.dlip_debug_set(_lib.DBG_ROWS2D, -1) == 0


def test_ops_refuse_cpu_tensors():
    import torch
    from deeplip_amd import ops
    from deeplip_amd._lib import DeepLipHipError
    with pytest.raises(DeepLipHipError):
        ops.meanstd_pool(torch.zeros(1, 4, 8))
    with pytest.raises(DeepLipHipError):
        ops.conv_nhwc(torch.zeros(1, 2, 2, 4), torch.zeros(4, 1, 1, 4))


def test_binding_arity_matches_header():
    """Every ctypes signature has as many arguments as the header's prototype (ctypes would push a short or long list without
    complaint; the kernel would then read garbage pointers)."""
    from deeplip_amd import _lib
    text = open(os.path.join(ROOT, "include", "deeplip_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    seen = 0
    for m in re.finditer(r"\b(dlip_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        name, args = m.group(1), m.group(2).strip()
        n = 0 if args in ("", "void") else len(args.split(","))
        if name in _lib.SIGNATURES:
            assert len(_lib.SIGNATURES[name]) == n, f"{name}: header has {n} arguments, binding {len(_lib.SIGNATURES[name])}"
            seen += 1
    assert seen == len(_lib.SIGNATURES)


# ---- the binding is derived from the header (deeplip_amd/_lib.py parse_header): what the derivation must yield ----
P, VP, I32, I64, F32, F64 = ctypes.POINTER, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_double


def test_derived_signatures_match_handwritten_expectations():
    """One prototype of each kind, its ctypes list typed out here from the C declaration: a wrong width, a float taken for a
    double, two swapped arguments or a host pointer passed as an integer make ctypes push garbage without complaint."""
    from deeplip_amd import _lib
    D = P(_lib.ConvDesc)
    want = {
        # int64_t and double scalars among int32_t
        "dlip_powspec_wave_fft64_f32": (ctypes.c_int, [VP, VP, VP, I64, I64, I32, I32, I32, I32, F64, I32, I32, VP]),
        # int64_t return, host descriptor, host int32_t*
        "dlip_conv_pool_partial_bytes": (I64, [D, P(I32)]),
        # host arrays of device pointers and of int32_t beside device pointers
        "dlip_tcn_dw_fwd_f32": (ctypes.c_int, [VP, I32, P(VP), P(VP), P(VP), P(VP), P(I32), P(I32), P(I32), I32, I32, I32, I32, VP]),
        "dlip_plan_end": (ctypes.c_int, [VP, P(VP)]),
        # three consecutive float scalars
        "dlip_bn_rows_train_fwd_f32": (ctypes.c_int, [VP] * 9 + [I32, I32, F32, F32, F32, I32, I32, VP, VP]),
        "dlip_abi_version": (ctypes.c_int, []),
        "dlip_error_string": (ctypes.c_char_p, [ctypes.c_int]),
    }
    for name, (restype, argtypes) in want.items():
        assert _lib.PROTOTYPES[name] == (restype, argtypes), name
        if name != "dlip_error_string":
            assert _lib.SIGNATURES[name] == argtypes
    fn = _lib.lib().dlip_conv_pool_partial_bytes          # and that is what the loaded library's functions carry
    assert fn.restype is I64 and list(fn.argtypes) == want["dlip_conv_pool_partial_bytes"][1]
    # every return type of the header is one of these four
    assert {r for r, _ in _lib.PROTOTYPES.values()} == {ctypes.c_int, I32, I64, ctypes.c_char_p}
    assert len(_lib.SIGNATURES) == len(_lib.PROTOTYPES) - 2 >= 154


HOST_POINTERS = {   # every parameter the CPU dereferences (DLIP_HOST in the header): function -> argument positions
    "dlip_conv_nhwc_f32": [0], "dlip_conv_nhwc_f16x3": [0], "dlip_conv_nhwc_stats_f16x3": [0], "dlip_conv2_nhwc_f16x3": [0],
    "dlip_conv_pool_f16x3": [0], "dlip_conv_pool_partial_bytes": [0, 1], "dlip_conv_stats_chunks": [0], "dlip_conv_plan": [0, 2, 3],
    "dlip_conv_kernel_kind": [0], "dlip_conv_route": [0, 5, 6, 7], "dlip_span_scope_end": [1], "dlip_plan_end": [1], "dlip_chomp_concat_f32": [0, 1, 2],
    "dlip_tcn_dw_fwd_f32": [2, 3, 4, 5, 6, 7, 8], "dlip_tcn_dw_dgrad_f32": [0, 2, 3, 4, 5], "dlip_tcn_dw_wgrad_f32": [2, 3, 4, 5, 6],
}


def test_host_pointers_are_exactly_the_marked_ones():
    """Everything else that is a pointer travels as an integer address (c_void_p): a DLIP_HOST mark lost or added in the header
    changes what ctypes passes, and shows here."""
    from deeplip_amd import _lib
    got = {}
    for name, args in _lib.SIGNATURES.items():
        pos = [i for i, t in enumerate(args) if isinstance(getattr(t, "_type_", None), type)]      # POINTER(...) classes
        if pos:
            got[name] = pos
    assert got == HOST_POINTERS
    assert sum(len(v) for v in got.values()) == 38


def _parse(text):
    from deeplip_amd import _lib
    return _lib.parse_header(text)


def test_parser_refuses_unknown_types():
    from deeplip_amd._lib import DeepLipHipError
    with pytest.raises(DeepLipHipError, match="dlip_f"):
        _parse("int dlip_f(const float* x, size_t n);")
    with pytest.raises(DeepLipHipError, match="dlip_f"):
        _parse("int dlip_f(unsigned int n);")
    with pytest.raises(DeepLipHipError, match="dlip_f"):
        _parse("int dlip_f(DLIP_HOST int32_t n);")                      # a host mark on a scalar
    with pytest.raises(DeepLipHipError, match="dlip_f"):
        _parse("int dlip_f(DLIP_HOST const dlip_other_desc* d);")       # a host struct the binding has no class for
    with pytest.raises(DeepLipHipError, match="dlip_g"):
        _parse("void dlip_g(int32_t n);")
    with pytest.raises(DeepLipHipError, match="dlip_g"):
        _parse("float* dlip_g(void);")


def test_parser_on_synthetic_headers():
    consts, fields, protos = _parse("""
        /* int dlip_in_block_comment(int32_t n); */
        // int dlip_in_line_comment(int32_t n);
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define DLIP_ABI_VERSION 7
        #define DLIP_EINVAL (-1)   /* a negative one */
        #define DLIP_HOST
        #define DLIP_DERIVED (DLIP_ABI_VERSION * 2)
        enum { DLIP_A = 0, DLIP_B = 5,
               DLIP_C = 6 };
        typedef void* dlip_stream_t;
        typedef struct dlip_conv_desc {
          int32_t N, H;   /* input */
          int32_t K;
        } dlip_conv_desc;
        #define DLIP_FLAG 1
        int dlip_after_define(DLIP_HOST const dlip_conv_desc* d, const void* w, int32_t flags);
        int64_t
        dlip_three_lines(const float* x,
                         DLIP_HOST const float* const* rows, DLIP_HOST dlip_plan_t* plan, uint32_t seed,
                         double a, dlip_stream_t stream);
        const char* dlip_text(int code);
        #ifdef __cplusplus
        }
        #endif
    """)
    from deeplip_amd import _lib
    assert consts == {"DLIP_ABI_VERSION": 7, "DLIP_EINVAL": -1, "DLIP_A": 0, "DLIP_B": 5, "DLIP_C": 6, "DLIP_FLAG": 1}
    assert fields == [("N", I32), ("H", I32), ("K", I32)]
    assert protos == {
        "dlip_after_define": (ctypes.c_int, [P(_lib.ConvDesc), VP, I32]),         # the #define above it did not leak into `int`
        "dlip_three_lines": (I64, [VP, P(VP), P(VP), ctypes.c_uint32, F64, VP]),
        "dlip_text": (ctypes.c_char_p, [ctypes.c_int]),
    }


def test_shared_constants_come_from_the_header():
    from deeplip_amd import _lib, build
    text = open(os.path.join(ROOT, "include", "deeplip_hip.h")).read()
    abi = int(re.search(r"^#define DLIP_ABI_VERSION (\d+)$", text, flags=re.M).group(1))
    lib = ctypes.CDLL(build.build(verbose=False))
    assert lib.dlip_abi_version() == _lib.ABI_VERSION == abi
    names = ["N", "H", "W", "C", "K", "R", "S", "stride_h", "stride_w", "pad_h", "pad_w", "dil_h", "dil_w", "Ho", "Wo", "ldx", "ldy", "ldr"]
    assert _lib.ConvDesc._fields_ == [(n, I32) for n in names] and ctypes.sizeof(_lib.ConvDesc) == 72
    # the two layouts the kernels assume: the debug table's last key, and a lift buffer = the pair + max(4096 maxima, the broadcast)
    assert _lib.DBG_GROUPED == 10 and _lib.DBG_CONV_TILE == 0 and _lib.DBG_ROWS2D == 7
    assert _lib.LIFT_WORDS == 2 + 2 * _lib.LIFT_BCAST == 4098
    assert _lib._EVID_WORDS == 32 * 32 and _lib._ST_LOW == 4
    assert sorted(_lib._STATUS_NAMES) == [0, 1, 2, 3]       # one message per producer family word, below the low-side word
