"""_lib.call, the one checked way from Python into the library, pinned down without a GPU.

Every case passes ``stream=None`` or names an entry point without a stream, so nothing of torch.cuda is touched; the refusals
relied on are DLIP_CHECK_ARG ones (DLIP_EINVAL before any HIP call, as in test_train_args_cpu.py) on made-up addresses that are
never dereferenced, and the calls that would go further meet a stub bound in place of the library function.
"""
import re

import pytest
import torch

from deeplip_amd import _lib
from deeplip_amd._lib import DeepLipHipError, call

PRELU = "dlip_prelu_rows_fwd_f32"       # (x, slope, y, M, C, stream)
X, SLOPE, Y = 0x10000, 0x11000, 0x12000


def bind(monkeypatch, name, stub):
    monkeypatch.setattr(_lib.lib(), name, stub)


def must_not_run(*a):
    pytest.fail("the library function was entered")


def test_a_refused_argument_raises_with_the_functions_name():
    with pytest.raises(DeepLipHipError, match=r"dlip_prelu_rows_fwd_f32 failed: .*invalid argument.*code -1"):
        call(PRELU, X, SLOPE, Y, 0, 8, stream=None)         # M = 0


def test_what_replaces_the_name_in_the_message():
    with pytest.raises(DeepLipHipError, match=r"^my label failed: .*invalid argument.*code -1"):
        call(PRELU, X, SLOPE, Y, 0, 8, stream=None, what="my label")


@pytest.mark.parametrize("args", [(X, SLOPE, Y, 3), (X, SLOPE, Y, 3, 8, 0)], ids=["one too few", "one too many"])
def test_arity_is_exact_and_checked_before_the_library(monkeypatch, args):
    """ctypes by itself refuses the first and ACCEPTS the second (a cdecl function takes surplus arguments in silence)."""
    bind(monkeypatch, PRELU, must_not_run)
    with pytest.raises(TypeError, match=rf"{PRELU} takes 5 arguments.*6 parameters.*got {len(args)}"):
        call(PRELU, *args, stream=None)


def test_a_stream_is_never_made_out_of_a_surplus_argument(monkeypatch):
    bind(monkeypatch, PRELU, must_not_run)
    with pytest.raises(TypeError, match=PRELU):
        call(PRELU, X, SLOPE, Y, 3, 8, None)                # refused on the count alone, before the current stream is looked up


def header_prototypes():
    """name -> parameter declarations, read from the header on this test's own terms"""
    with open(_lib.HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
    return {name: [p.strip() for p in params.split(",")] for name, params in re.findall(r"\b(dlip_\w+)\s*\(([^()]*)\)\s*;", text)}


def test_a_trailing_stream_is_expected_exactly_where_the_header_ends_in_one(monkeypatch):
    protos = header_prototypes()
    assert set(_lib.SIGNATURES) <= set(protos)
    stream_first = []
    for name, argtypes in _lib.SIGNATURES.items():
        params = protos[name]
        assert len(params) == len(argtypes) or params in ([""], ["void"])
        last = params[-1].startswith("dlip_stream_t")
        if not last and any(p.startswith("dlip_stream_t") for p in params):
            stream_first.append(name)
        seen = []
        bind(monkeypatch, name, lambda *a: seen.append(a) or 0)
        n = len(argtypes)
        if last:
            call(name, *range(1, n), stream=0xABC)
            assert seen == [(*range(1, n), 0xABC)], name
            with pytest.raises(TypeError, match=name):
                call(name, *range(1, n + 1), stream=0xABC)  # ... and not one argument more
        else:
            call(name, *range(1, n + 1))
            assert seen == [tuple(range(1, n + 1))], name
            with pytest.raises(TypeError, match=name):
                call(name, *range(1, n + 1), stream=None)   # no implicit stream here, so none to replace
        assert len(seen) == 1, name
    assert sorted(stream_first) == ["dlip_plan_end", "dlip_span_scope_end"]
    assert PRELU in _lib.STREAM_LAST and not {"dlip_plan_end", "dlip_span_scope_end", "dlip_debug_set"} & _lib.STREAM_LAST


def test_an_entry_point_without_a_stream():
    with pytest.raises(DeepLipHipError, match=r"dlip_debug_set failed"):
        call("dlip_debug_set", _lib.DBG_ROWS2D, 1)          # key 7 is reserved: forcing the retired mode is refused
    assert call("dlip_debug_set", _lib.DBG_ROWS2D, -1) is None


def test_tensors_arrive_as_their_address_and_none_as_null(monkeypatch):
    seen = []
    bind(monkeypatch, PRELU, lambda *a: seen.append(a) or 0)
    x = torch.zeros(8)
    call(PRELU, x, None, x[4:], 1, 8, stream=None)
    assert seen == [(x.data_ptr(), None, x.data_ptr() + 16, 1, 8, None)]


def test_an_unknown_name_raises():
    for name in ("dlip_prelu_rows_fwd_f33", "dlip_error_string"):      # not in the header; in it, but no status comes back
        with pytest.raises(DeepLipHipError, match=name):
            call(name, X, stream=None)
