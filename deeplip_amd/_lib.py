"""ctypes binding of libdeeplip_hip.so (C ABI: include/deeplip_hip.h).

There is no CPU fallback anywhere in this package: if the library is missing or fails to load,
``lib()`` raises and every op that needs it fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import threading

import torch  # must be imported first: the library binds to the HIP runtime torch already loaded

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DLIP_LIB_PATH") or os.path.join(_PKG, "lib", "libdeeplip_hip.so")  # env override: A/B builds
HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "deeplip_hip.h")   # what build.py compiles (and hashes) the library from

_lock = threading.Lock()
_lib = None
_status = None
_status_np = None

c_f = C.c_void_p      # device pointer (passed as integer address); the three names tests spell expected argtypes with
c_i32 = C.c_int32
c_i64 = C.c_int64


class DeepLipHipError(RuntimeError):
    pass


class DeepLipRangeError(DeepLipHipError):
    """An activation left the range of the split-fp16 ("f16x3") arithmetic (|v| >= 65520): the results of the
    launches since the last check are invalid.  Recourse: pack that model in the exact mode,
    ``deeplip_amd.packing.set_precision("f32")`` (same engine, fp32 MFMA)."""


class ConvDesc(C.Structure):
    """struct dlip_conv_desc (_fields_: the header's, set below)"""


# ---- the binding is DERIVED from include/deeplip_hip.h: its prototypes, integer #defines, enums and dlip_conv_desc ----
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "float": C.c_float,
            "double": C.c_double, "dlip_stream_t": C.c_void_p, "dlip_plan_t": C.c_void_p}
_PARAM = re.compile(r"(DLIP_HOST )?(?:const )?(\w+) ?(\*(?: ?const ?\*)?)?(?: ?\w+)?")   # [DLIP_HOST] [const] T [* | * const*] [name]


def _argtype(decl: str, proto: str):
    """ctypes class of one parameter declaration (whitespace normalised, no space in front of a '*')."""
    m = _PARAM.fullmatch(decl)
    host, base, stars = m.groups() if m else (None, None, None)
    if stars and not host:
        return C.c_void_p                               # a device pointer, whatever it points to: passed as an integer address
    if stars and stars != "*":
        return C.POINTER(C.c_void_p)                    # DLIP_HOST T* const*: a host array of device pointers
    if stars and base == "dlip_conv_desc":
        return C.POINTER(ConvDesc)
    if stars and base in _SCALARS:
        return C.POINTER(_SCALARS[base])                # DLIP_HOST T*: a host array or out-parameter
    if not stars and not host and base in _SCALARS:
        return _SCALARS[base]
    raise DeepLipHipError(f"deeplip_hip.h: no ctypes mapping for parameter '{decl}' of {proto}")


def parse_header(text: str):
    """(constants, dlip_conv_desc fields, prototypes) of a header written like include/deeplip_hip.h: {DLIP_NAME: int} from the
    integer #defines and the enums, [(field, ctype)], {dlip_name: (restype, argtypes)}.  A type outside the closed table above
    raises: a new one must fail here, at import, not bind as something else."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts = {n: int(v) for n, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(DLIP_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)   # preprocessor lines would otherwise run into the next prototype's return type
    for body in re.findall(r"\benum\s*\{(.*?)\}", text, flags=re.S):
        consts.update((n, int(v)) for n, v in re.findall(r"(DLIP_\w+)\s*=\s*(-?\d+)", body))
    fields = []
    for body in re.findall(r"struct\s+dlip_conv_desc\s*\{(.*?)\}", text, flags=re.S):
        for typ, names in re.findall(r"(\w+)\s+([\w\s,]+);", body):
            fields += [(n.strip(), _SCALARS[typ]) for n in names.split(",")]
    protos = {}
    for stmt in text.split(";"):
        if "(" not in stmt:
            continue                                    # typedefs, struct fields, enums, the extern "C" braces
        stmt = re.sub(r"\s*\*", "*", " ".join(stmt.split()))
        m = re.fullmatch(r"(?:[^()]*[{}] ?)?([\w ]+?\*?) ?\b(dlip_\w+) ?\(([^()]*)\)", stmt)
        if m is None:
            raise DeepLipHipError(f"deeplip_hip.h: not a prototype: '{stmt}'")
        ret, name, args = m.groups()
        restype = C.c_char_p if ret == "const char*" else _SCALARS.get(ret)
        if restype is None:
            raise DeepLipHipError(f"deeplip_hip.h: no ctypes mapping for the return type '{ret}' of {name}")
        args = [a.strip() for a in args.split(",")] if args.strip() not in ("", "void") else []
        protos[name] = (restype, [_argtype(a, name) for a in args])
    return consts, fields, protos


def stream_last(text: str) -> frozenset:
    """Names of the prototypes in such a header whose LAST parameter is a dlip_stream_t: the entry points ``call`` hands the
    current stream to.  (dlip_span_scope_end and dlip_plan_end take theirs first: their callers pass it like any argument.)"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    return frozenset(re.findall(r"\b(dlip_\w+)\s*\([^()]*\bdlip_stream_t(?:\s+\w+)?\s*\)", text))


if not os.path.exists(HEADER_PATH):
    raise DeepLipHipError(f"{HEADER_PATH} not found: deeplip_amd binds libdeeplip_hip.so from the header it is built from "
                          "(a source tree: include/ beside the package). deeplip_amd has no CPU fallback.")
with open(HEADER_PATH) as _f:
    _text = _f.read()
HEADER, ConvDesc._fields_, PROTOTYPES = parse_header(_text)
# name -> argtypes of every launch entry point (the two that return text are bound from PROTOTYPES like the rest)
SIGNATURES = {n: a for n, (_, a) in PROTOTYPES.items() if n not in ("dlip_source_sha", "dlip_error_string")}
STREAM_LAST = stream_last(_text)
ABI_VERSION = HEADER["DLIP_ABI_VERSION"]
LIFT_WORDS = HEADER["DLIP_LIFT_WORDS"]
LIFT_BCAST = HEADER["DLIP_LIFT_BCAST"]
# waveform augmentation (deeplip_amd/augment.py): the FIR kernel's tile, its tap chunk and the longest room response it takes
DLIP_FIR_TILE, DLIP_FIR_TAP_CHUNK, DLIP_FIR_MAX_TAPS = (HEADER[n] for n in ("DLIP_FIR_TILE", "DLIP_FIR_TAP_CHUNK", "DLIP_FIR_MAX_TAPS"))
# ... and the transform route (reverb="fft"): the overlap-save block and the longest room response that route takes
DLIP_OLS_BLOCK, DLIP_OLS_MAX_TAPS = HEADER["DLIP_OLS_BLOCK"], HEADER["DLIP_OLS_MAX_TAPS"]

# sliding-window CMN (deeplip_amd/voiced_frames.py): the kernel's tile of output frames and the longest window it takes
DLIP_CMN_TILE, DLIP_CMN_MAX_WINDOW = HEADER["DLIP_CMN_TILE"], HEADER["DLIP_CMN_MAX_WINDOW"]

# waveform resampling (deeplip_amd/resample.py): the kernel's longest tile of outputs, its LDS budget in words (polyphase table + a
# tile's input span) and the largest up / down factor it takes
DLIP_RESAMPLE_TILE, DLIP_RESAMPLE_LDS_WORDS, DLIP_RESAMPLE_MAX_FACTOR = (HEADER[n] for n in ("DLIP_RESAMPLE_TILE", "DLIP_RESAMPLE_LDS_WORDS",
                                                                                          "DLIP_RESAMPLE_MAX_FACTOR"))


def lib() -> C.CDLL:
    """Load (once) and return the HIP library; raises if it is missing -- never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise DeepLipHipError(
                f"{LIB_PATH} not found: build it with `python -m deeplip_amd.build` "
                "(or __graft_entry__.build()). deeplip_amd has no CPU fallback.")
        l = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (restype, args) in PROTOTYPES.items():
            fn = getattr(l, name)  # AttributeError if the ABI lost a symbol
            fn.argtypes = args
            fn.restype = restype
        v = l.dlip_abi_version()
        if v != ABI_VERSION:
            raise DeepLipHipError(f"libdeeplip_hip.so ABI {v} != binding ABI {ABI_VERSION}; rebuild")
        _lib = l
    return _lib


def check(code: int, what: str) -> None:
    if code != 0:
        msg = lib().dlip_error_string(code).decode()
        raise DeepLipHipError(f"{what} failed: {msg} (code {code})")


def ptr(t) -> int | None:
    """Device address of a torch tensor (None -> NULL)."""
    if t is None:
        return None
    return t.data_ptr()


def stream_handle() -> int:
    if _status is None:
        status_words()      # first launch of the process: register the range-status block
    return torch.cuda.current_stream().cuda_stream


_CURRENT = object()     # call(stream=...): not given


def call(name: str, *args, stream=_CURRENT, what: str | None = None) -> None:
    """Launch the entry point ``name`` and raise DeepLipHipError unless it returns 0 (``what``: the error's label where it is not
    the name).  ``args`` are the header's parameters, exactly as many, tensors standing for their device address (None: NULL) --
    without the trailing dlip_stream_t of an entry point that has one: that is the current stream (stream_handle()), or
    ``stream=`` (a handle or None; torch.cuda is not touched then).  For the entry points that return a status."""
    argtypes = SIGNATURES.get(name)
    if argtypes is None:
        raise DeepLipHipError(f"{name}: no such entry point in include/deeplip_hip.h")
    takes_stream = name in STREAM_LAST
    if len(args) != len(argtypes) - takes_stream:
        raise TypeError(f"{name} takes {len(argtypes) - takes_stream} arguments{' and the stream' if takes_stream else ''} "
                        f"({len(argtypes)} parameters in the header), got {len(args)}")
    args = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    if takes_stream:
        args.append(stream_handle() if stream is _CURRENT else stream)
    elif stream is not _CURRENT:
        raise TypeError(f"{name} has no trailing dlip_stream_t: stream= is not for it")
    check(getattr(lib(), name)(*args), what or name)


def env_switch(name: str) -> bool:
    """An A/B switch of the environment: on unless the variable is set to "0"."""
    return os.environ.get(name, "1") != "0"


# Workspace of the conv kernel's balanced work split: one torch-owned block per (device, stream),
# registered with the library the first time that stream launches a convolution, so the library itself
# never allocates device memory.
_workspaces: dict = {}


def ensure_conv_workspace() -> None:
    st = torch.cuda.current_stream()
    key = (torch.cuda.current_device(), st.cuda_stream)
    if key in _workspaces:
        return
    nbytes = int(lib().dlip_conv_workspace_bytes())
    if nbytes <= 0:
        raise DeepLipHipError("dlip_conv_workspace_bytes failed (no ROCm device?)")
    buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    call("dlip_conv_set_workspace", buf.data_ptr(), nbytes, stream=st.cuda_stream)
    _workspaces[key] = buf


# ---- diagnostic overrides (tests, tools): dlip_debug_set ----
globals().update((n[5:], v) for n, v in HEADER.items() if n.startswith("DLIP_DBG_"))   # DBG_CONV_TILE .. DBG_GROUPED: the header's keys


DEBUG = {}          # what this process set through debug_set (key -> value; -1 / absent = the built-in choice)


def debug_set(key: int, value: int = -1) -> None:
    call("dlip_debug_set", key, value)
    DEBUG[key] = value


# ---- range status of the f16x3 arithmetic: eight words in host-pinned, device-visible memory ----
_STATUS_NAMES = {HEADER["DLIP_ST_CONV"]: "a convolution / linear epilogue", HEADER["DLIP_ST_STEM"]: "the fused stem + pool",
                 HEADER["DLIP_ST_PACK"]: "split_pack (a model input or gradient operand)", HEADER["DLIP_ST_POOL"]: "statistics pooling"}
_ST_LOW = HEADER["DLIP_ST_LOW"]


def status_words():
    """Registers (once) the status block the kernels report range violations to.  It lives in pinned host memory,
    which the GPU addresses directly: the host can look at it at any time without synchronising."""
    global _status, _status_np
    if _status is None:
        t = torch.zeros(8, dtype=torch.int32).pin_memory()
        call("dlip_set_status_words", t.data_ptr())
        _status_np = t.numpy()      # same memory: a forward's check is one numpy read
        _status = t
    return _status


def _range_error(words) -> "DeepLipRangeError":
    high = [n for w, n in sorted(_STATUS_NAMES.items()) if words[w]]
    recourse = ("results since the last check are invalid. Run that model in the exact mode -- arith 'f32' (deeplip_amd.arith / "
                "--arith / model.arith / DLIP_ARITH), i.e. deeplip_amd.packing.set_precision('f32'): exact fp32 MFMA, same engine; "
                "arith 'auto' does it by itself for the batch concerned.")
    if high:
        return DeepLipRangeError("f16x3 arithmetic: an activation with |v| >= 65520 (not representable as hi + lo fp16) was "
                                 f"produced by {', '.join(high)}; " + recourse)
    fam = words[_ST_LOW] - 1
    who = _STATUS_NAMES.get(fam, "a split-format producer")
    return DeepLipRangeError(f"f16x3 arithmetic: {who} produced a tensor whose largest magnitude is below 2^-2 = 0.25: its "
                             "lo halves are fp16 subnormals and the result is no longer fp32-grade (relative error 3e-8 / max|v|); "
                             + recourse)


class StatusBlock:
    """A status block of its own (dlip_status_scope): int32[8] in pinned host memory, handed to the launches a thread makes inside
    ``scope()`` -- a recorded step plan keeps reporting to it on every replay, so the host can tell WHICH plan's batch left the
    range.  Live blocks are also looked at by ``check_range()``: nothing reported anywhere goes unseen."""

    def __init__(self):
        self.t = torch.zeros(8, dtype=torch.int32).pin_memory()
        self.np = self.t.numpy()
        self.private = False        # True: the owner settles every report itself (a pipeline's per-batch f32 re-run); check_range() skips it
        _blocks.add(self)

    def take(self):
        """The error this block holds (and clears), or None.  A host memory read: covers launches that have completed."""
        if not self.np.any():
            return None
        words = self.t.tolist()
        self.t.zero_()
        return _range_error(words)

    def scope(self):
        import contextlib

        @contextlib.contextmanager
        def cm():
            status_words()      # the process-wide block exists before any launch, scoped or not
            call("dlip_status_scope", self.t.data_ptr())
            try:
                yield self
            finally:
                lib().dlip_status_scope(None)
        return cm()


import weakref as _weakref

_blocks = _weakref.WeakSet()


def check_range(sync: bool = False) -> None:
    """Raise DeepLipRangeError if a kernel reported an activation outside what the split format holds since the last call:
    |v| >= 65520 (infinite in fp16), or a whole produced tensor with its largest magnitude in (0, 2^-2) (lo is subnormal
    there: relative accuracy below fp32 grade; include/deeplip_hip.h).  Without ``sync`` only launches that have completed are
    covered (the call is a host memory read); callers that are about to consume results synchronise first (or pass sync=True).
    Covers the process-wide block and every live StatusBlock (recorded plans report to their own)."""
    t = status_words()
    if sync:
        torch.cuda.synchronize()
    if _status_np.any():
        words = t.tolist()
        t.zero_()
        raise _range_error(words)
    for b in list(_blocks):
        if b.private:
            continue
        err = b.take()
        if err is not None:
            raise err


# ---- low-side range scopes: one evidence word per split-producing launch (dlip_range_scope_*) ----
_SCOPE_SLOTS = 128           # launches per scope (a B = 64 fused step makes ~40)
_EVID_WORDS = HEADER["DLIP_EVID_WORDS"]     # int32 words of evidence per launch (32 cache lines)
_RING_CHUNKS = 16
_rings = {}                  # (device index, stream handle) -> [ring tensor, next chunk]
_scope_depth = threading.local()


def scope_slots(device=None):
    """A zeroed block of evidence words owned by the caller (a StepPlan keeps one for its lifetime)."""
    return torch.zeros(_EVID_WORDS * _SCOPE_SLOTS, dtype=torch.int32, device=device if device is not None else "cuda")


class range_scope:
    """``with range_scope():`` around the launches of one forward pass; the verdict kernel goes out on the current stream at
    exit (join side streams first).  Nested scopes fold into the outermost one of the thread.  Eager scopes draw their words from
    a ring of chunks OF THE STREAM THEY OPEN ON (a scope's verdict kernel re-zeroes its chunk on that stream, and the next user of
    the chunk launches on the same stream: in order, so a chunk is clean before it is written again -- one ring shared by all
    streams had no such order between, say, an ExtractPipeline's run stream and the caller's); a StepPlan passes its own block,
    which the recorded launches then address for the plan's lifetime."""

    def __init__(self, slots=None):
        self.slots = slots
        self.outer = False

    def __enter__(self):
        d = getattr(_scope_depth, "n", 0)
        self.outer = d == 0
        if not self.outer:
            _scope_depth.n = d + 1
            return self
        if _status is None:
            status_words()
        slots = self.slots
        if slots is None:
            key = (torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
            with _lock:
                ring = _rings.get(key)
                if ring is None:
                    # zeroed on the current stream = the stream of every later user of this ring
                    ring = _rings[key] = [torch.zeros(_RING_CHUNKS * _EVID_WORDS * _SCOPE_SLOTS, dtype=torch.int32, device="cuda"), 0]
                slots = ring[0][ring[1] * _EVID_WORDS * _SCOPE_SLOTS:(ring[1] + 1) * _EVID_WORDS * _SCOPE_SLOTS]
                ring[1] = (ring[1] + 1) % _RING_CHUNKS
        call("dlip_range_scope_begin", slots.data_ptr(), min(_SCOPE_SLOTS, slots.numel() // _EVID_WORDS))
        _scope_depth.n = d + 1          # only once the scope is really open: a failed begin leaves the thread's depth as it was
        return self

    def __exit__(self, et, ev, tb):
        _scope_depth.n -= 1
        if self.outer:
            rc = lib().dlip_range_scope_end(torch.cuda.current_stream().cuda_stream)
            if et is None:
                check(rc, "dlip_range_scope_end")
        return False


def scoped_eval(fn):
    """Method decorator: an eval-mode call runs inside a low-side range scope (train mode is left alone: its split operands
    carry explicit power-of-two scales, deeplip_amd/autograd*.py)."""
    import functools

    @functools.wraps(fn)
    def wrapper(self, *a, **k):
        if getattr(self, "training", False):
            return fn(self, *a, **k)
        with range_scope():
            return fn(self, *a, **k)
    return wrapper
