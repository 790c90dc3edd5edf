"""tests/poison.py on CPU tensors: the views it hands out, what the patterns read as, what check() and untouched() report, and that poisoned() swaps
the package's `torch` globals for the block only."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poison  # noqa: E402
from poison import FINITE, NAN, Ledger, poisoned  # noqa: E402

DTYPES = [torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.uint8, torch.int32]
SHAPES = [(1,), (7,), (3, 5), (2, 3, 7), (0, 4), (1025,)]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("pattern", [NAN, FINITE], ids=["NAN", "FINITE"])
def test_views_have_the_requested_shape_dtype_contiguity_and_alignment(dtype, pattern):
    L = Ledger(pattern)
    for shape in SHAPES:
        v = L.empty(shape, dtype, "cpu")
        assert tuple(v.shape) == shape and v.dtype == dtype and v.is_contiguous() and v.device.type == "cpu"
        a = L.allocs[-1]
        assert v.storage_offset() * v.element_size() == poison.BAND_BYTES and poison.BAND_BYTES % 512 == 0       # the interior sits as the allocator aligned the block
        assert v.numel() == 0 or v.data_ptr() - a.outer.data_ptr() == poison.BAND_BYTES
        assert a.outer.numel() == 2 * poison.BAND_BYTES + (v.numel() * v.element_size() + 511) // 512 * 512
        assert L.untouched(v) == v.numel()
        w = L.empty_like(v)
        assert w.shape == v.shape and w.dtype == v.dtype and w.is_contiguous() and (v.numel() == 0 or w.data_ptr() != v.data_ptr())
    L.check()
    assert L.empty(5, dtype, "cpu").shape == (5,)
    L.release()
    assert L.allocs == []


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64], ids=str)
def test_the_nan_pattern_is_nan_in_every_float_type_and_the_finite_one_is_finite(dtype):
    v = Ledger(NAN).empty((3, 37), dtype, "cpu")
    assert bool(torch.isnan(v).all())
    f = Ledger(FINITE).empty((3, 37), dtype, "cpu")
    assert bool(torch.isfinite(f).all()) and bool((f > 1.0).all())
    assert torch.equal(Ledger(NAN).empty((4,), torch.uint8, "cpu"), torch.tensor([0xFF, 0x7F, 0xFF, 0x7F], dtype=torch.uint8))
    assert abs(float(Ledger(FINITE).empty((1,), torch.float16, "cpu")[0]) - 21.2) < 0.1


def test_wrap_copies_values_and_strides():
    L = Ledger(NAN)
    t = torch.arange(24, dtype=torch.float32).view(2, 3, 4)
    w = L.wrap(t)
    assert torch.equal(w, t) and w.is_contiguous() and w.data_ptr() != t.data_ptr() and L.untouched(w) == 0
    p = t.permute(2, 0, 1)                      # dense, not contiguous: torch.empty_like keeps such strides, and so does the ledger
    wp = L.wrap(p)
    assert torch.equal(wp, p) and wp.stride() == p.stride()
    s = t[:, :, 1:3]                            # not dense: contiguous, as torch.empty_like gives
    ws = L.wrap(s)
    assert torch.equal(ws, s) and ws.is_contiguous()
    L.check()


@pytest.mark.parametrize("dtype,shape", [(torch.float16, (3, 5)), (torch.uint8, (7,)), (torch.uint8, (512,)), (torch.float64, (9,))], ids=str)
def test_a_byte_planted_next_to_the_interior_is_reported_with_side_and_offset(dtype, shape):
    L = Ledger(NAN)
    L.empty((4, 4), torch.float32, "cpu")
    v = L.empty(shape, dtype, "cpu")
    L.check()                                   # a clean run passes
    a = L.allocs[-1]
    nbytes = v.numel() * v.element_size()
    a.outer[a.front - 1] ^= 0x01                # the byte just before the interior
    with pytest.raises(AssertionError) as e:
        L.check()
    msg = str(e.value)
    assert "allocation #1" in msg and str(shape) in msg and str(dtype) in msg and "test_poison_host.py" in msg
    assert "BEFORE the interior: 1 bytes modified, offsets -1 .. -1 " in msg and "AFTER" not in msg
    a.outer[a.front - 1] ^= 0x01
    L.check()
    a.outer[a.front + nbytes] ^= 0x80           # the byte just after it (inside the round-up to 512 bytes where there is one)
    a.outer[a.front + nbytes + 40] = 0
    with pytest.raises(AssertionError) as e:
        L.check()
    msg = str(e.value)
    assert "AFTER the interior: 2 bytes modified, offsets +0 .. +40 " in msg and "BEFORE" not in msg and "allocation #0" not in msg
    v.zero_()                                   # writing the interior is nobody's business
    a.outer[a.front + nbytes] ^= 0x80
    a.outer[a.front + nbytes + 40] = (NAN >> 8) if (nbytes + 40) & 1 else (NAN & 0xFF)
    L.check()
    a.outer[-1] = 0                             # the far ends of both bands
    a.outer[0] = 0
    with pytest.raises(AssertionError) as e:
        L.check()
    assert f"offsets -{poison.BAND_BYTES} .. -{poison.BAND_BYTES} " in str(e.value) and f".. +{a.outer.numel() - a.front - nbytes - 1} past" in str(e.value)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_untouched_counts_pattern_elements_of_any_view(dtype):
    L = Ledger(FINITE)
    v = L.empty((6, 9), dtype, "cpu")
    v[1:3, 2:5] = 1
    assert L.untouched(v) == 54 - 6
    assert L.untouched(v[1:3]) == 18 - 6 and L.untouched(v[:, 3]) == 4 and L.untouched(v[1:3, 2:5]) == 0 and L.untouched(v[0]) == 9
    assert L.untouched(v[:, 1::2]) == 24 - 2 and L.untouched(v[4:, 5:]) == 8
    with pytest.raises(ValueError):
        L.untouched(torch.zeros(3, dtype=dtype))


def test_untouched_bytes_follow_the_pattern_phase():
    L = Ledger(NAN)
    v = L.empty((5, 3), torch.uint8, "cpu")     # odd row length: rows start on alternating pattern bytes
    assert L.untouched(v) == 15 and L.untouched(v[1]) == 3 and L.untouched(v[:, 1]) == 5
    v[1, 0] = 0xFF                              # the pattern's OTHER byte: offset 3 holds 0x7F
    assert L.untouched(v) == 14


def _fake_package():
    """a package of two modules that use `torch` the way the project's wrappers do"""
    src = ("import torch\n"
           "KEEP = {}\n"
           "def alloc(*a, **k):\n    return torch.empty(*a, **k)\n"
           "def like(t, **k):\n    return torch.empty_like(t, **k)\n"
           "def misc(x):\n    assert isinstance(x, torch.Tensor)\n    return torch.zeros(2, dtype=torch.float16), torch.cat([x, x]), torch.float32, torch.nn.functional.relu(x)\n"
           "def boom():\n    raise RuntimeError('boom')\n")
    mods = {}
    for name in ("fakepkg", "fakepkg.inner"):
        m = types.ModuleType(name)
        exec(src, m.__dict__)
        sys.modules[name] = mods[name] = m
    other = types.ModuleType("fakepkg_other")      # not part of the package: keeps its torch
    exec(src, other.__dict__)
    sys.modules["fakepkg_other"] = other
    return mods["fakepkg"], mods["fakepkg.inner"], other


@pytest.fixture
def fake():
    yield _fake_package()
    for n in ("fakepkg", "fakepkg.inner", "fakepkg_other"):
        sys.modules.pop(n, None)


def test_requests_for_other_devices_pass_through_and_the_proxy_forwards(fake):
    pkg, inner, other = fake
    L = Ledger(NAN)
    with poisoned(L, package="fakepkg"):
        assert pkg.torch is not torch and inner.torch is pkg.torch and other.torch is torch
        m = pkg.alloc(1, 4, 8, 8, device="meta", dtype=torch.float16)
        assert m.device.type == "meta" and m.shape == (1, 4, 8, 8)
        assert inner.alloc((3, 4), dtype=torch.float32, device="cpu").shape == (3, 4)
        assert pkg.alloc(1).shape == (1,) and pkg.like(torch.zeros(3)).shape == (3,)
        assert L.allocs == []                                   # nothing of that was the ledger's business
        z, c, dt, r = pkg.misc(torch.ones(3))
        assert z.dtype == torch.float16 and c.shape == (6,) and dt is torch.float32 and float(r.sum()) == 3.0
        assert pkg.torch.Tensor is torch.Tensor and pkg.torch.cuda is torch.cuda and pkg.torch.nn is torch.nn
    assert pkg.torch is torch and inner.torch is torch


def test_cuda_requests_are_routed_to_the_ledger(fake, monkeypatch):
    """no GPU here: the routing decision is `_ours`, and the ledger is asked with the wrapper's arguments"""
    pkg, _, _ = fake
    L = Ledger(NAN)
    calls = []
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: (calls.append(1), capturing[0])[1])
    monkeypatch.setattr(Ledger, "empty", lambda self, shape, dtype=None, device=None, _site=None: ("empty", tuple(shape) if not isinstance(shape, int) else shape, dtype, str(device), _site))
    monkeypatch.setattr(Ledger, "empty_like", lambda self, t, dtype=None, device=None, _site=None: ("like", tuple(t.shape), dtype, device, _site))
    capturing = [False]
    with poisoned(L, package="fakepkg"):
        P = pkg.torch
        assert P._ours("cuda") and P._ours(torch.device("cuda", 0)) and P._ours("cuda:1")
        assert not P._ours("cpu") and not P._ours("meta") and not P._ours(None)
        kind, shape, dt, dev, site = pkg.alloc((3, 5), dtype=torch.float16, device="cuda")
        assert (kind, shape, dt, dev) == ("empty", (3, 5), torch.float16, "cuda") and site.startswith("<string>:")
        assert pkg.alloc(3, 5, dtype=torch.int32, device=torch.device("cuda", 0))[:3] == ("empty", (3, 5), torch.int32)
        assert pkg.alloc(7, dtype=torch.uint8, device="cuda")[1] == (7,)
        meta_cuda = types.SimpleNamespace(device=torch.device("cuda", 0), shape=(2, 2), is_contiguous=lambda: True)
        assert pkg.like(meta_cuda)[:2] == ("like", (2, 2))
        assert pkg.like(meta_cuda, memory_format=torch.contiguous_format)[:2] == ("like", (2, 2))
        capturing[0] = True                                     # while the stream captures a graph the request is torch's
        assert not P._ours("cuda")
    assert calls


def test_globals_and_kept_workspaces_are_restored_after_the_block_raises(fake):
    pkg, inner, _ = fake
    sys.modules["fakepkg.pf"] = pf = types.ModuleType("fakepkg.pf")
    try:
        pf.torch, pf._GN_WS, pf._WS = torch, {"k": 1}, {}
        ws = pf._GN_WS
        with pytest.raises(RuntimeError, match="boom"):
            with poisoned(Ledger(NAN), package="fakepkg"):
                assert pkg.torch is not torch and pf.torch is not torch
                assert pf._GN_WS is ws and ws == {}             # emptied for the block: the package allocates its workspaces anew, from the ledger
                ws["poisoned"] = 2
                pkg.boom()
        assert pkg.torch is torch and inner.torch is torch and pf.torch is torch
        assert pf._GN_WS is ws and ws == {"k": 1}
    finally:
        sys.modules.pop("fakepkg.pf", None)


def test_the_real_package_is_swapped_and_restored():
    import gswm_amd  # noqa: F401
    from gswm_amd import codec, imaging, pf, unet, xattn
    mods = (codec, imaging, pf, unet, xattn)
    with poisoned(Ledger(NAN)):
        assert all(isinstance(m.torch, poison._TorchProxy) for m in mods)
        assert unet.torch.empty(1, 4, 8, 8, device="meta", dtype=torch.float16).device.type == "meta"
        assert unet.nn is torch.nn and pf.torch.Tensor is torch.Tensor
    assert all(m.torch is torch for m in mods)


def test_where_names_the_allocation_and_the_byte_offsets():
    L = Ledger(NAN)
    v = L.empty((6, 9), torch.float16, "cpu")
    v.zero_()
    v[5, 7:] = float("nan")                     # any NaN is not the pattern ...
    v.view(torch.int16)[4, 8] = NAN             # ... this one is
    v.view(torch.int16)[5, 8] = NAN
    msg = L.where(v)
    assert "(6, 9) torch.float16" in msg and "test_poison_host.py" in msg
    assert f"2 untouched elements of 2 bytes, the first at byte offset {(4 * 9 + 8) * 2} of the interior, the last at {(5 * 9 + 8) * 2} (interior: 108 bytes)" in msg
    assert f"1 written elements of 2 bytes, the first at byte offset {(5 * 9 + 7) * 2} of the interior, the last at {(5 * 9 + 7) * 2} " in L.where(v[5, 7:], untouched=False)
    assert "no untouched element" in L.where(v[:4])
    b = L.empty((5, 3), torch.uint8, "cpu")
    b[:] = 0
    b[1, 0] = 0x7F                              # offset 3: odd, the pattern's high byte
    assert "1 untouched elements of 1 bytes, the first at byte offset 3 of the interior, the last at 3 " in L.where(b[:, 0])
