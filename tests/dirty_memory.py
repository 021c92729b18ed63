"""Recycled memory for the tests: ``torch.empty`` that returns poisoned, guarded blocks.

Every buffer the library fills comes from ``torch.empty`` / ``empty_like`` / ``new_empty``.
Inside ``with dirty(byte, device) as mem:`` those three return, for an allocation on ``device``,
a view of the requested shape and dtype into a uint8 block laid out as

    [ GUARD bytes of 0xA5 | payload, every byte = ``byte`` | GUARD bytes of 0xA5 ]

so a kernel that reads a slot before writing it computes with the pattern (and its result
differs between patterns), and one that stores outside its buffer breaks a guard, which
``mem.check()`` reports.  GUARD is a multiple of the caching allocator's 512-byte granule, so
the payload is aligned as a plain allocation is and every alignment-dependent route of the
library answers as it does in production.

Patterns: 0x00 the clean run; 0xFF NaN in f32 / bf16 / f64, -1 in the ints, 255 in u8;
0x55 a finite 1.5e13 in f32 and bf16 and large positive ints.

Allocations on other devices, calls with ``out=`` and calls with a keyword this module does
not interpret go to the real function untouched.  Not for use around a graph capture: the
fills would be captured and ``check()`` synchronises.

A plain helper module: no conftest, no pytest setting.
"""
from __future__ import annotations

import contextlib
import math

import torch

GUARD = 4096
GUARD_BYTE = 0xA5
CLEAN, NAN, BIG = 0x00, 0xFF, 0x55
PATTERNS = (CLEAN, NAN, BIG)

_ORIG = {"empty": torch.empty, "empty_like": torch.empty_like, "new_empty": torch.Tensor.new_empty}
_active = []


def _same_device(a: torch.device, b: torch.device) -> bool:
    if a.type != b.type:
        return False
    if a.type != "cuda":
        return True

    def index(d):
        return torch.cuda.current_device() if d.index is None else d.index
    return index(a) == index(b)


def _size(args, kwargs):
    """The requested size of an ``empty`` / ``new_empty`` call as a tuple of ints, or None where
    the call is not one this module interprets."""
    if "size" in kwargs:
        if args:
            return None
        args = (kwargs["size"],)
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        args = tuple(args[0])
    try:
        size = tuple(int(s) for s in args)
    except (TypeError, ValueError):
        return None
    if any(isinstance(s, bool) or not isinstance(s, int) for s in args) or any(s < 0 for s in size):
        return None
    return size


class Dirty:
    """The state of one ``dirty`` block: what it handed out, and ``check``."""

    def __init__(self, byte: int, device):
        if not 0 <= int(byte) <= 255:
            raise ValueError(f"byte {byte} is not in 0 .. 255")
        self.byte = int(byte)
        self.device = torch.device(device)
        self.allocations = []  # (block, payload bytes, shape, dtype)

    # -- the allocation path
    def allocate(self, shape, dtype, strides=None) -> torch.Tensor:
        shape = tuple(int(s) for s in shape)
        itemsize = torch.empty((), dtype=dtype, device="meta").element_size()
        nbytes = math.prod(shape) * itemsize
        block = _ORIG["empty"](GUARD + nbytes + GUARD, dtype=torch.uint8, device=self.device)
        block[:GUARD] = GUARD_BYTE
        block[GUARD:GUARD + nbytes] = self.byte
        block[GUARD + nbytes:] = GUARD_BYTE
        flat = block[GUARD:GUARD + nbytes].view(dtype)
        out = flat.view(shape) if strides is None else flat.as_strided(shape, strides, flat.storage_offset())
        self.allocations.append((block, nbytes, shape, dtype))
        return out

    def wants(self, device) -> bool:
        return _same_device(torch.device(device), self.device)

    # -- the guards
    def check(self) -> None:
        """Assert that every guard handed out so far still holds 0xA5 (synchronises)."""
        for n, (block, nbytes, shape, dtype) in enumerate(self.allocations):
            for side, guard, base in (("before", block[:GUARD], -GUARD), ("after", block[GUARD + nbytes:], 0)):
                bad = guard != GUARD_BYTE
                if bool(bad.any()):
                    first = int(bad.nonzero()[0, 0])
                    raise AssertionError(
                        f"guard {side} allocation #{n} (shape {shape}, {dtype}, {nbytes} bytes) overwritten: "
                        f"first bad byte at offset {base + first} from the payload's "
                        f"{'start' if side == 'before' else 'end'}, holds 0x{int(guard[first]):02X}")


def _empty(*args, **kwargs):
    mem = _active[-1]
    if set(kwargs) - {"size", "dtype", "device", "memory_format"}:
        return _ORIG["empty"](*args, **kwargs)
    if kwargs.get("memory_format", torch.contiguous_format) is not torch.contiguous_format:
        return _ORIG["empty"](*args, **kwargs)
    size = _size(args, kwargs)
    device = kwargs.get("device")
    if device is None:
        device = torch.get_default_device() if hasattr(torch, "get_default_device") else "cpu"
    if size is None or not mem.wants(device):
        return _ORIG["empty"](*args, **kwargs)
    dtype = kwargs.get("dtype")
    return mem.allocate(size, torch.get_default_dtype() if dtype is None else dtype)


def _empty_like(*args, **kwargs):
    mem = _active[-1]
    if len(args) != 1 or not isinstance(args[0], torch.Tensor) or set(kwargs) - {"dtype", "device", "memory_format"}:
        return _ORIG["empty_like"](*args, **kwargs)
    if kwargs.get("memory_format", torch.preserve_format) is not torch.preserve_format:
        return _ORIG["empty_like"](*args, **kwargs)
    like = args[0]
    device = kwargs.get("device")
    device = like.device if device is None else device
    if like.layout is not torch.strided or not mem.wants(device):
        return _ORIG["empty_like"](*args, **kwargs)
    dtype = kwargs.get("dtype")
    strides = None
    if not like.is_contiguous():  # the strides the real function would choose (a dense permutation)
        strides = _ORIG["empty_like"](like, device="meta").stride()
    return mem.allocate(like.shape, like.dtype if dtype is None else dtype, strides)


def _new_empty(self, *args, **kwargs):
    mem = _active[-1]
    if set(kwargs) - {"size", "dtype", "device"}:
        return _ORIG["new_empty"](self, *args, **kwargs)
    size = _size(args, kwargs)
    device = kwargs.get("device")
    device = self.device if device is None else device
    if size is None or not mem.wants(device):
        return _ORIG["new_empty"](self, *args, **kwargs)
    dtype = kwargs.get("dtype")
    return mem.allocate(size, self.dtype if dtype is None else dtype)


@contextlib.contextmanager
def dirty(byte: int, device):
    """Replace ``torch.empty``, ``torch.empty_like`` and ``torch.Tensor.new_empty`` for the block;
    yields the ``Dirty`` whose ``check()`` verifies the guards.  Restores the three names on the
    way out, also after an exception.  Blocks do not nest."""
    if _active:
        raise RuntimeError("dirty blocks do not nest")
    mem = Dirty(byte, device)
    _active.append(mem)
    torch.empty, torch.empty_like, torch.Tensor.new_empty = _empty, _empty_like, _new_empty
    try:
        yield mem
    finally:
        torch.empty, torch.empty_like = _ORIG["empty"], _ORIG["empty_like"]
        torch.Tensor.new_empty = _ORIG["new_empty"]
        _active.pop()


def check() -> None:
    """``check()`` of the active ``dirty`` block."""
    if not _active:
        raise RuntimeError("check() outside a dirty block")
    _active[-1].check()


def bits(t: torch.Tensor) -> torch.Tensor:
    """``t`` as integers of its element size, contiguous, so that NaN compares equal to NaN."""
    t = t.detach().contiguous()
    if t.dtype.is_floating_point:
        t = t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    elif t.dtype == torch.bool:
        t = t.view(torch.uint8)
    return t
