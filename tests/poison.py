"""Poisoned, guard-banded buffers for the kernel parity tests (tests/test_gpu_poisoned.py; proven on CPU tensors by tests/test_poison_host.py).

A `Ledger` hands out tensors that sit inside a larger allocation [front band | interior, rounded up to 512 bytes | back band], the whole of which is
filled with a repeating 16-bit pattern.  A kernel that leaves an output element unwritten leaves the pattern there (`untouched`), one that stores outside
its buffer changes a band (`check`), and one whose result depends on memory it should not read gives different bits under the two patterns.
`poisoned(ledger)` serves every `torch.empty` / `torch.empty_like` of the gswm_amd modules from the ledger.  A plain module: no pytest plugin, no settings."""
from __future__ import annotations

import contextlib
import os
import sys
from typing import List, Optional

import torch

NAN = 0x7FFF        # a NaN as fp16, as bf16, as fp32 (0x7FFF7FFF) and as fp64; the bytes 0xFF, 0x7F
FINITE = 0x4D4D     # about 21.2 as fp16, about 2.15e8 as bf16 and as fp32 (0x4D4D4D4D): finite, and nothing a kernel computes by accident

ALIGN = 512         # the caching allocator's granule: the interior keeps the alignment a plain torch.empty has
# The largest single store tile of the project is 256 rows x 1280 columns of a 16-bit type (a 256-row tile of the matmul engine at the widest output the
# UNet has) = 640 KiB; a store that is off by a whole tile still lands in a band.  Rounded up to 1 MiB per side.
BAND_BYTES = 1 << 20
assert BAND_BYTES >= 256 * 1280 * 2 and BAND_BYTES % ALIGN == 0

_HERE = os.path.abspath(__file__)
_SAME_SIZE_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _signed16(p: int) -> int:
    return p - 0x10000 if p >= 0x8000 else p


def _call_site() -> str:
    """the nearest frame outside this file (the wrapper line that asked for the buffer) and, when there is one, the test function above it"""
    f = sys._getframe(1)
    first, test = None, None
    while f is not None:
        fn = f.f_code.co_filename
        if os.path.abspath(fn) != _HERE and "contextlib" not in fn:
            if first is None:
                first = f"{os.path.basename(fn)}:{f.f_lineno} in {f.f_code.co_name}"
            elif os.path.basename(fn).startswith("test_") and f.f_code.co_name.startswith("test_"):
                test = f"{os.path.basename(fn)}:{f.f_lineno} in {f.f_code.co_name}"
                break
        f = f.f_back
    return first if test is None else f"{first} <- {test}"


def _dense(t: torch.Tensor) -> bool:
    """the strides are a permutation of a contiguous tensor's: torch.empty_like keeps such strides"""
    expect = 1
    for size, stride in sorted(((sz, st) for sz, st in zip(t.shape, t.stride()) if sz != 1), key=lambda p: p[1]):
        if stride != expect:
            return False
        expect *= size
    return True


class _Alloc:
    __slots__ = ("outer", "front", "nbytes", "shape", "dtype", "site")

    def __init__(self, outer, front, nbytes, shape, dtype, site):
        self.outer, self.front, self.nbytes, self.shape, self.dtype, self.site = outer, front, nbytes, shape, dtype, site

    def describe(self) -> str:
        return f"{tuple(self.shape)} {self.dtype} on {self.outer.device}, requested at {self.site}"


class Ledger:
    def __init__(self, pattern: int = NAN, band_bytes: int = BAND_BYTES):
        if not 0 <= pattern <= 0xFFFF or band_bytes <= 0 or band_bytes % ALIGN:
            raise ValueError("Ledger: a 16-bit pattern and a band that is a multiple of 512 bytes")
        self.pattern, self.band = pattern, band_bytes
        self.allocs: List[_Alloc] = []

    # ---- allocation
    def _flat(self, nbytes: int, shape, dtype, device, site) -> torch.Tensor:
        """-> the interior as a flat uint8 view of `nbytes` bytes"""
        padded = (nbytes + ALIGN - 1) // ALIGN * ALIGN
        outer = torch.empty(2 * self.band + padded, dtype=torch.uint8, device=device)
        outer.view(torch.int16).fill_(_signed16(self.pattern))
        self.allocs.append(_Alloc(outer, self.band, nbytes, tuple(shape), dtype, site or _call_site()))
        return outer[self.band:self.band + nbytes]

    def empty(self, shape, dtype: Optional[torch.dtype] = None, device=None, _site: Optional[str] = None) -> torch.Tensor:
        shape = (int(shape),) if isinstance(shape, int) else tuple(int(s) for s in shape)
        dtype = torch.get_default_dtype() if dtype is None else dtype
        n = 1
        for s in shape:
            n *= s
        flat = self._flat(n * dtype.itemsize, shape, dtype, "cpu" if device is None else device, _site or _call_site())
        return flat.view(dtype).view(shape)

    def empty_like(self, t: torch.Tensor, dtype: Optional[torch.dtype] = None, device=None, _site: Optional[str] = None) -> torch.Tensor:
        dtype = t.dtype if dtype is None else dtype
        device = t.device if device is None else device
        site = _site or _call_site()
        if t.is_contiguous() or not _dense(t):
            return self.empty(t.shape, dtype, device, _site=site)
        flat = self._flat(t.numel() * dtype.itemsize, t.shape, dtype, device, site)      # torch.empty_like keeps the strides of a dense permuted tensor
        return flat.view(dtype).as_strided(t.shape, t.stride())

    def wrap(self, t: torch.Tensor) -> torch.Tensor:
        """a copy of `t` (same shape, dtype, device and strides) inside a banded buffer: what lies just outside the operand is pattern, not pool memory"""
        v = self.empty_like(t, _site=_call_site())
        v.copy_(t)
        return v

    # ---- checks
    def _pattern_bytes(self, n: int, device) -> torch.Tensor:
        return torch.full(((n + 1) // 2,), _signed16(self.pattern), dtype=torch.int16, device=device).view(torch.uint8)[:n]

    def check(self) -> None:
        """every band of every allocation still holds the pattern bit for bit (the bytes between the interior's end and the next 512-byte boundary belong to
        the back band)"""
        if not self.allocs:
            return
        pat = _signed16(self.pattern)
        flags = []
        for a in self.allocs:
            o = a.outer
            end = a.front + a.nbytes
            odd = end & 1
            bad = (o[:a.front].view(torch.int16) != pat).any() | (o[end + odd:].view(torch.int16) != pat).any()
            if odd:
                bad = bad | (o[end] != (self.pattern >> 8))
            flags.append(bad)
        by_dev = {}
        for i, f in enumerate(flags):
            by_dev.setdefault(f.device, []).append(i)
        dirty = []
        for dev, idx in by_dev.items():
            hit = torch.stack([flags[i] for i in idx]).cpu()
            dirty += [idx[j] for j in range(len(idx)) if bool(hit[j])]
        if not dirty:
            return
        msgs = []
        for i in sorted(dirty):
            a = self.allocs[i]
            o, end = a.outer, a.front + a.nbytes
            exp = self._pattern_bytes(o.numel(), o.device)
            parts = []
            d = (o[:a.front] != exp[:a.front]).nonzero().flatten()
            if d.numel():
                parts.append(f"BEFORE the interior: {d.numel()} bytes modified, offsets {int(d[0]) - a.front} .. {int(d[-1]) - a.front} relative to the interior's start")
            d = (o[end:] != exp[end:]).nonzero().flatten()
            if d.numel():
                parts.append(f"AFTER the interior: {d.numel()} bytes modified, offsets +{int(d[0])} .. +{int(d[-1])} past the interior's end ({a.nbytes} bytes)")
            msgs.append(f"guard band of allocation #{i} {a.describe()} was written -- " + "; ".join(parts))
        raise AssertionError("\n".join(msgs))

    def _owner(self, view: torch.Tensor) -> _Alloc:
        p = view.data_ptr()
        for a in reversed(self.allocs):
            lo = a.outer.data_ptr() + a.front
            if lo <= p < lo + max(a.nbytes, 1) and view.device == a.outer.device:
                return a
        raise ValueError("untouched: not a view into a buffer of this ledger")

    def _pattern_mask(self, view: torch.Tensor, a: _Alloc) -> torch.Tensor:
        """bool tensor of view's shape: the element still holds the pattern"""
        size = view.element_size()
        if size >= 2:
            word = 0
            for _ in range(size // 2):
                word = (word << 16) | self.pattern
            if word >= 1 << (8 * size - 1):
                word -= 1 << (8 * size)
            return view.view(_SAME_SIZE_INT[size]) == word
        # one-byte elements: the pattern's low byte sits at even offsets from the interior's start, its high byte at odd ones
        v = view.view(torch.uint8)
        par = torch.full((1,) * v.dim(), (v.data_ptr() - a.outer.data_ptr() - a.front) & 1, dtype=torch.int64, device=v.device)
        for d in range(v.dim()):
            shp = [1] * v.dim()
            shp[d] = v.shape[d]
            par = par + ((torch.arange(v.shape[d], device=v.device) * v.stride(d)) & 1).view(shp)
        return v == torch.where((par & 1) == 0, self.pattern & 0xFF, self.pattern >> 8).to(torch.uint8)

    def untouched(self, view: torch.Tensor) -> int:
        """how many elements of `view` (any view into an interior of this ledger, strided ones included) still hold the pattern"""
        if view.numel() == 0:
            return 0
        return int(self._pattern_mask(view, self._owner(view)).sum())

    def where(self, view: torch.Tensor, untouched: bool = True) -> str:
        """for a failure message: the allocation `view` lies in, and the first and last byte offset (relative to the interior's start) of its elements that
        still hold the pattern (untouched=True) or no longer do (False)"""
        a = self._owner(view)
        mask = self._pattern_mask(view, a)
        nz = (mask if untouched else ~mask).nonzero()
        what = "untouched" if untouched else "written"
        if nz.numel() == 0:
            return f"allocation {a.describe()}: no {what} element"
        base = view.data_ptr() - a.outer.data_ptr() - a.front
        off = base + (nz * torch.tensor(view.stride(), device=nz.device)).sum(dim=1) * view.element_size()
        return (f"allocation {a.describe()}: {nz.shape[0]} {what} elements of {view.element_size()} bytes, the first at byte offset {int(off.min())} of the "
                f"interior, the last at {int(off.max())} (interior: {a.nbytes} bytes)")

    def release(self) -> None:
        self.allocs.clear()


def scratch(ledger: Ledger, nbytes: int, device="cuda") -> torch.Tensor:
    """a pattern-filled uint8 buffer for `pf.splitk_workspace(...)`: split-K and key-split attention then run on it instead of the stream's cached scratch"""
    return ledger.empty((int(nbytes),), torch.uint8, device, _site=_call_site())


class _TorchProxy:
    """stands in for the `torch` global of a gswm_amd module: `empty` / `empty_like` for a CUDA device come from the ledger, everything else is torch's"""

    def __init__(self, ledger: Ledger):
        object.__setattr__(self, "_ledger", ledger)

    def __getattr__(self, name):
        return getattr(torch, name)

    def __setattr__(self, name, value):
        setattr(torch, name, value)

    @staticmethod
    def _ours(device) -> bool:
        if device is None:
            return False
        if torch.device(device).type != "cuda":
            return False          # "meta" (unet.py's FLOP counters), CPU
        return not torch.cuda.is_current_stream_capturing()

    def empty(self, *size, **kw):
        if "size" in kw or set(kw) - {"dtype", "device"} or not self._ours(kw.get("device")):
            return torch.empty(*size, **kw)
        shape = size[0] if len(size) == 1 and not isinstance(size[0], int) else size
        return self._ledger.empty(shape, kw.get("dtype"), kw["device"], _site=_call_site())

    def empty_like(self, t, **kw):
        if kw.get("memory_format", torch.preserve_format) is torch.contiguous_format and t.is_contiguous():
            kw = {k: v for k, v in kw.items() if k != "memory_format"}
        if set(kw) - {"dtype", "device"} or not self._ours(kw.get("device", t.device)):
            return torch.empty_like(t, **kw)
        return self._ledger.empty_like(t, kw.get("dtype"), kw.get("device"), _site=_call_site())


# buffers the package allocates once and keeps: emptied for the block (so that the ledger serves them) and put back afterwards (so that no ledger buffer outlives it)
_KEPT = (("pf", "_GN_WS"), ("pf", "_WS"))


def _package_modules(package: str):
    return [m for n, m in list(sys.modules.items()) if m is not None and (n == package or n.startswith(package + ".")) and getattr(m, "__dict__", {}).get("torch") is torch]


@contextlib.contextmanager
def poisoned(ledger: Ledger, package: str = "gswm_amd"):
    """Inside the block every torch.empty / torch.empty_like that a module of `package` issues for a CUDA device is a banded, pattern-filled ledger buffer.
    Only those modules' `torch` global is swapped (for a forwarding proxy): nothing outside the package sees it.  Requests for other devices, and requests
    made while the current stream is capturing a graph, pass through.  The previous globals are back on exit, also after an exception."""
    mods = _package_modules(package)
    proxy = _TorchProxy(ledger)
    kept = []
    for m in mods:
        m.__dict__["torch"] = proxy
    for mod, name in _KEPT:
        d = getattr(sys.modules.get(f"{package}.{mod}"), name, None)
        if isinstance(d, dict):
            kept.append((d, dict(d)))
            d.clear()
    try:
        yield ledger
    finally:
        for m in mods:
            m.__dict__["torch"] = torch
        for d, before in kept:
            d.clear()
            d.update(before)
