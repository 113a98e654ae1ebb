"""Footprint checking for kernel tests: does a launch touch only the memory it owns?

Plain Python and torch, CPU and GPU alike (tests/test_footprint_cpu.py proves on the CPU that the checker checks).

Every tensor a footprint test hands to a kernel lives inside a ``Fenced`` allocation ``[fence | payload | fence]`` whose fences -- and,
for a channel slice (``wide``), whose neighbour channels -- hold a known fill.  After the launch the fill must still be there bit for bit
(the launch wrote nothing it does not own), and the result must not depend on whether the fill was POISON or ZEROS (it read nothing
it does not own, or at least used nothing of it: 0 x NaN is NaN).

POISON is one 8-byte pattern that is a NaN as an fp64, as either of its fp32 words and as each of its four fp16 halves, so the same
fill serves fp32 tensors, split-format (hi | lo fp16) tensors and fp64 partials; in an int32 buffer it is a recognisable constant."""
from __future__ import annotations

import torch

POISON = 0x7FF87FC07FC07FC0
ZEROS = 0
POISON_WORDS = (0x7FC07FC0, 0x7FF87FC0)      # its two 32-bit words (low, high)

MIN_FENCE = 64 << 10
TILE_ROWS = 256                              # the tallest row tile of any kernel here: a fence covers one of the payload's pitch


def finite(value: float) -> int:
    """The 8-byte fill that reads as ``value`` in both fp32 words."""
    w = torch.tensor([value], dtype=torch.float32).view(torch.int32).item() & 0xFFFFFFFF
    return (w << 32 | w) - (1 << 64 if w >> 31 else 0)


def _up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def _pattern(fill: int, nbytes: int, device) -> torch.Tensor:
    """``nbytes`` (a multiple of 8) bytes of the 8-byte fill."""
    return torch.full((nbytes // 8,), fill, dtype=torch.int64, device=device).view(torch.uint8)


class FootprintError(AssertionError):
    pass


class Fenced:
    """One flat allocation [fence | payload | fence].  Each fence is a multiple of 256 bytes (the payload keeps the allocator's
    alignment), covers at least TILE_ROWS rows of ``pitch_bytes`` and is never under 64 KiB; the trailing fence begins at the
    payload's last byte + 1.  The whole allocation starts out as ``fill``."""

    def __init__(self, nbytes: int, device="cpu", fill: int = POISON, pitch_bytes: int = 0, name: str = ""):
        self.nbytes, self.fill, self.name = int(nbytes), fill, name
        self.fence = max(MIN_FENCE, _up(TILE_ROWS * int(pitch_bytes), 256))
        self.total = _up(2 * self.fence + self.nbytes, 8)
        self.buf = _pattern(fill, self.total, device)
        self.lo, self.hi = self.fence, self.fence + self.nbytes

    @property
    def payload(self) -> torch.Tensor:
        return self.buf[self.lo:self.hi]

    def view(self, shape, dtype=torch.float32) -> torch.Tensor:
        """The contiguous payload tensor."""
        return self.payload.view(dtype).view(tuple(shape))

    def expected(self) -> torch.Tensor:
        return _pattern(self.fill, self.total, self.buf.device)

    def _report(self, bad: torch.Tensor, what: str):
        """bad: bool per byte of the allocation -> None or (first offset relative to the payload, bytes that differ, what)."""
        n = int(bad.sum())
        if n == 0:
            return None
        first = int(torch.nonzero(bad)[0, 0]) - self.lo
        return first, n, what

    def violations(self):
        """None, or (first offending byte offset RELATIVE TO THE PAYLOAD -- negative: leading fence, >= nbytes: trailing fence --,
        how many bytes differ, which part)."""
        bad = self.buf != self.expected()
        bad[self.lo:self.hi] = False
        return self._report(bad, "fence")

    def check(self) -> None:
        v = self.violations()
        if v is not None:
            raise FootprintError(f"{self.name or 'allocation'} ({self.nbytes} bytes): {v[2]} overwritten, first at byte {v[0]} relative to "
                                 f"the payload, {v[1]} bytes differ")


class Wide:
    """A tensor [..., left + C + right] inside a Fenced whose channels [left, left + C) are ``t`` and whose other channels are the fill:
    ``full`` goes to the kernel with a channel offset (``left``) and the wide pitch; ``own`` is the slice itself."""

    def __init__(self, t: torch.Tensor, left: int, right: int, fill: int = POISON, name: str = "", copy: bool = True):
        """``copy`` False: ``t`` only gives shape, dtype and device and the slice itself starts out as the fill too (an output)."""
        if t.element_size() != 4:
            raise ValueError("wide: 4-byte elements (fp32, or the split format in its fp32 container)")
        C = t.shape[-1]
        if left % 4 or (left + C + right) % 4 or left < 0 or right < 0:
            raise ValueError("wide: left and the whole width must be multiples of 4 elements (16-byte aligned slices)")
        self.left, self.C, self.right, self.width = left, C, right, left + C + right
        shape = tuple(t.shape[:-1]) + (self.width,)
        self.rows = t.numel() // C
        self.fenced = Fenced(self.rows * self.width * 4, t.device, fill, pitch_bytes=self.width * 4, name=name)
        self.full = self.fenced.view(shape, t.dtype)
        self.own = self.full[..., left:left + C]
        if copy:
            self.own.copy_(t)

    def neighbour_violations(self):
        f = self.fenced
        bad = (f.payload != f.expected()[f.lo:f.hi]).view(self.rows, self.width * 4)
        bad[:, self.left * 4:(self.left + self.C) * 4] = False
        n = int(bad.sum())
        if n == 0:
            return None
        first = int(torch.nonzero(bad.view(-1))[0, 0])
        row, col = divmod(first, self.width * 4)
        return first, n, f"neighbour channel {col // 4} of row {row}"

    def check_neighbours(self) -> None:
        v = self.neighbour_violations()
        if v is not None:
            raise FootprintError(f"{self.fenced.name or 'slice'} [{self.rows} rows x ({self.left} | {self.C} | {self.right})]: {v[2]} "
                                 f"overwritten, first at byte {v[0]} relative to the payload, {v[1]} bytes differ")

    def check(self) -> None:
        self.fenced.check()
        self.check_neighbours()


def wide(t: torch.Tensor, left: int, right: int, fill: int = POISON, name: str = "", copy: bool = True) -> Wide:
    """fp32 tensors: ``left`` (and ``right`` whenever C is) a multiple of 4; split-format tensors: multiples of 32, as ops.conv_nhwc asks.
    ``left`` = 0 is the one-sided form for tensors that take a pitch but no offset (a residual with ldr > K)."""
    return Wide(t, left, right, fill, name, copy)


class Vector:
    """``t`` (bias, slope, post scale / shift, w_scale, packed weights ...) with the fill directly behind its last element."""

    def __init__(self, t: torch.Tensor, fill: int = POISON, name: str = ""):
        self.fenced = Fenced(t.numel() * t.element_size(), t.device, fill, pitch_bytes=0, name=name)
        self.t = self.fenced.view(t.shape, t.dtype)
        self.t.copy_(t)

    def check(self) -> None:
        self.fenced.check()


def vector(t: torch.Tensor, fill: int = POISON, name: str = "") -> Vector:
    return Vector(t, fill, name)


def has_poison(t: torch.Tensor) -> bool:
    """Whether any aligned 32-bit word of ``t`` (4- or 8-byte elements) still is one of POISON's."""
    if t.numel() == 0:
        return False
    w = t.contiguous().view(-1).view(torch.int32)
    return bool(((w == POISON_WORDS[0]) | (w == POISON_WORDS[1])).any())


class FenceArena:
    """Stands in for deeplip_amd.plan.Arena (``take``, ``keep``, ``modules``): with ``ops.ARENA`` set to one, every tensor an ops.*
    wrapper allocates comes out fenced and filled.  It is also the register of everything a test fences by hand (``fenced``, ``wide``,
    ``vector`` below), so that ``check_all`` covers inputs and outputs alike."""

    def __init__(self, fill: int = POISON):
        self.fill = fill
        self.keep: list = []
        self.modules: dict = {}
        self.items: list = []          # Fenced | Wide | Vector, in the order they were made
        self.taken: list = []          # (Fenced, tensor) of every take()

    def take(self, shape, device, dtype) -> torch.Tensor:
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        es = torch.empty((), dtype=dtype).element_size()
        f = Fenced(n * es, device, self.fill, pitch_bytes=(shape[-1] if shape else 1) * es, name=f"take#{len(self.taken)} {shape} {dtype}")
        t = f.view(shape, dtype)
        self.items.append(f)
        self.taken.append((f, t))
        return t

    def fenced(self, t: torch.Tensor, name: str = "") -> torch.Tensor:
        """A fenced copy of ``t`` (same shape and dtype)."""
        f = Fenced(t.numel() * t.element_size(), t.device, self.fill, pitch_bytes=(t.shape[-1] if t.dim() else 1) * t.element_size(), name=name)
        self.items.append(f)
        v = f.view(t.shape, t.dtype)
        v.copy_(t)
        return v

    def filled(self, shape, device, dtype=torch.float32, name: str = "") -> torch.Tensor:
        """A fenced tensor left at the fill (an output the test hands in itself)."""
        t = self.take(shape, device, dtype)
        self.taken[-1][0].name = name or self.taken[-1][0].name
        return t

    def wide(self, t: torch.Tensor, left: int, right: int, name: str = "") -> Wide:
        w = wide(t, left, right, self.fill, name)
        self.items.append(w)
        return w

    def wide_out(self, shape, device, left: int, right: int, name: str = "") -> Wide:
        """An fp32 (or split-format) output slice [..., shape[-1]] with neighbours, everything at the fill."""
        w = Wide(torch.empty(tuple(shape), dtype=torch.float32, device=device), left, right, self.fill, name, copy=False)
        self.items.append(w)
        return w

    def vector(self, t, name: str = ""):
        """None passes through; otherwise the fenced copy itself."""
        if t is None:
            return None
        v = vector(t, self.fill, name)
        self.items.append(v)
        return v.t

    def check_all(self, route: str = "") -> None:
        errs = []
        for it in self.items:
            try:
                it.check()
            except FootprintError as e:
                errs.append(str(e))
        if errs:
            raise FootprintError((f"[{route}] " if route else "") + "; ".join(errs))

    def unwritten(self, t: torch.Tensor) -> bool:
        """Whether any of the poison is left in ``t``'s own extent (meaningful for a POISON arena)."""
        return has_poison(t)
