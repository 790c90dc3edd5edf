"""Multi-bit windows (--l 2, 4), host side: the committed threshold table against a fresh bisection on scipy's ndtr, the vote arithmetic
with l, the refusal of unsupported windows wherever l enters, the CLI parsers, the exported symbols.  No GPU."""
import ctypes
import os
import struct
import subprocess
import sys
import types

import numpy as np
import pytest
from scipy.special import ndtr

import gs_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _key(x):
    b = struct.unpack("<q", struct.pack("<d", x))[0]
    return b if b >= 0 else -(b & 0x7FFFFFFFFFFFFFFF)


def _unkey(k):
    b = k if k >= 0 else (-k) | (1 << 63)
    return struct.unpack("<d", struct.pack("<Q", b & 0xFFFFFFFFFFFFFFFF))[0]


def bisect_threshold(l, j):
    """the smallest double t with int(ndtr(t) * 2**l) >= j, over the ordered doubles of [-40, 40]"""
    q = float(2 ** l)
    a, b = _key(-40.0), _key(40.0)
    while b - a > 1:
        m = (a + b) // 2
        if int(ndtr(_unkey(m)) * q) >= j:
            b = m
        else:
            a = m
    return _unkey(b)


@pytest.mark.parametrize("l", [2, 4])
def test_quant_thresholds_equal_a_fresh_bisection(l):
    from gswm_amd import codec
    t = codec.quant_thresholds(l)
    assert t.dtype == np.float64 and t.shape == (2 ** l - 1,)
    want = np.array([bisect_threshold(l, j) for j in range(1, 2 ** l)])
    assert t.tobytes() == want.tobytes()
    assert np.all(np.diff(t) > 0)
    # the step function they stand for, one double either side of every threshold
    for j, x in enumerate(t, start=1):
        assert int(ndtr(x) * 2 ** l) == j and int(ndtr(np.nextafter(x, -np.inf)) * 2 ** l) == j - 1


def test_published_threshold_values():
    from gswm_amd import codec
    t2, t4 = codec.quant_thresholds(2), codec.quant_thresholds(4)
    assert t2.tolist() == [-0.6744897501960818, -6.957291061679417e-17, 0.6744897501960816]
    assert t4[0] == -1.5341205443525463
    # the middle threshold is the l = 1 constant, in every table
    assert t2[1] == O.Y1_THRESHOLD == t4[7] == codec.quant_thresholds(1)[0]
    assert codec.quant_thresholds(1).shape == (1,)


def test_the_committed_table_is_what_the_generator_writes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_quant_thresholds.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_vote_copies_with_l():
    from gswm_amd import codec
    assert codec.vote_copies(16384, 256) == 64 == codec.vote_copies(16384, 256, 1)
    assert codec.vote_copies(16384, 256, 2) == 128
    assert codec.vote_copies(16384, 512, 2) == 64                 # twice the message at the same 64 votes
    assert codec.vote_copies(16384, 256, 4) == 256
    assert codec.vote_copies(36, 72, 2) == 1 and codec.vote_copies(36, 8, 4) == 18
    with pytest.raises(IndexError, match="string index out of range"):
        codec.vote_copies(36, 16, 2)                              # 72 bits
    with pytest.raises(IndexError):
        codec.vote_copies(16384, 3000, 4)
    with pytest.raises(ValueError):
        codec.vote_copies(6, 4, 2)                                # 12 bits do not fill whole bytes


@pytest.mark.parametrize("l", [3, 0, 8, -1, 2.0, "2", None, True])
def test_unsupported_windows_are_refused_everywhere(l):
    """every public entry that takes l refuses it before it touches a device"""
    import torch
    from gswm_amd import codec, extract, gs_insert, pipeline, trace
    key, nonce = bytes(32), bytes(16)
    z = torch.zeros(1, 16)
    ns = types.SimpleNamespace(key=key, nonce=nonce, l=l, message_length=8)
    opt = types.SimpleNamespace(key_hex="00" * 32, nonce_hex="00" * 16)
    reg = trace.Registry(32)
    reg.add("a", b"\x01" * 32)
    calls = [lambda: codec.check_window(l),
             lambda: codec.quant_thresholds(l),
             lambda: codec.vote_copies(16, 8, l),
             lambda: codec.embed_batch(key, nonce, b"\x00", 1, (4, 2, 2), l=l),
             lambda: codec.extract_batch(z, key, nonce, 8, l=l),
             lambda: codec.quant_pack(z, l),
             lambda: extract.recover_exactracted_message(z, ns),
             lambda: extract.recover_exactracted_message_batch(z, ns),
             lambda: gs_insert.gs_watermark_init_noise(opt, "m", log_path=None, l=l),
             lambda: gs_insert.gs_watermark_init_noise_batch(opt, "m", 2, seed=1, l=l),
             lambda: pipeline.GaussianShadingPipeline(lambda *a: None, key, nonce, b"\x00" * 32, l=l),
             lambda: trace.trace_latents(z, key, nonce, reg, l=l),
             ]
    for c in calls:
        with pytest.raises(ValueError, match="l must be one of"):
            c()


def test_keyed_trace_refuses_unsupported_windows():
    import torch
    from gswm_amd import trace
    reg = trace.KeyedRegistry(32)
    reg.add("a", bytes(32), bytes(16), b"\x01" * 32)
    for l in (3, 0, 8):
        with pytest.raises(ValueError, match="l must be one of"):
            trace.trace_latents_keyed(torch.zeros(1, 4, 8, 16), reg, l=l)


def test_c_entry_points_refuse_unsupported_windows_and_ragged_lattices():
    """status codes that need no device: GSW_ERR_UNSUPPORTED for l outside {1, 2, 4} and for windows that do not fill whole bytes,
    GSW_ERR_RAGGED for a message the bits do not tile, GSW_ERR_BAD_ARG for null operands"""
    from gswm_amd import _native as N
    lib = N.lib()
    key, nonce = bytes(32), bytes(16)
    p = ctypes.c_void_p(64)           # never dereferenced: every call below is refused before a launch
    for l in (0, 3, 8, -2, 16):
        assert lib.gsw_embed_l(key, nonce, b"\x00", 1, None, 0, 0, p, N.GSW_F32, 1, 16, 0, l, None) == N.GSW_ERR_UNSUPPORTED
        assert lib.gsw_extract_l(p, N.GSW_F32, key, nonce, 8, p, None, p, 1, 16, l, None) == N.GSW_ERR_UNSUPPORTED
        assert lib.gsw_quant_pack(p, N.GSW_F32, p, p, 1, 16, l, None) == N.GSW_ERR_UNSUPPORTED
    assert lib.gsw_extract_l(p, N.GSW_F32, key, nonce, 8, p, None, p, 1, 3, 2, None) == N.GSW_ERR_UNSUPPORTED      # 6 bits
    assert lib.gsw_quant_pack(p, N.GSW_F32, p, p, 1, 1, 4, None) == N.GSW_ERR_UNSUPPORTED                          # 4 bits
    assert lib.gsw_extract_l(p, N.GSW_F32, key, nonce, 16, p, None, p, 1, 36, 2, None) == N.GSW_ERR_RAGGED         # 72 bits, 16-bit message
    assert lib.gsw_extract_l(None, N.GSW_F32, key, nonce, 8, p, None, p, 1, 16, 2, None) == N.GSW_ERR_BAD_ARG
    assert lib.gsw_extract_l(p, 7, key, nonce, 8, p, None, p, 1, 16, 2, None) == N.GSW_ERR_BAD_ARG
    assert lib.gsw_embed_l(key, nonce, b"\x00", 1, None, 0, 0, None, N.GSW_F32, 1, 16, 0, 2, None) == N.GSW_ERR_BAD_ARG
    assert lib.gsw_embed_l(key, nonce, b"\x00", 1, None, 0, 0, p, N.GSW_F32, 1, 18, 0, 4, None) == N.GSW_ERR_BAD_ARG   # n_elems % 4, as gsw_embed
    assert lib.gsw_quant_pack(p, N.GSW_F32, None, p, 1, 16, 2, None) == N.GSW_ERR_BAD_ARG
    # l == 1 is the entry point without _l: its own refusals come back
    assert lib.gsw_extract_l(p, N.GSW_F32, key, nonce, 7, p, None, p, 1, 16, 1, None) == N.GSW_ERR_RAGGED
    assert lib.gsw_quant_pack(p, N.GSW_F32, p, p, 1, 12, 1, None) == N.GSW_ERR_UNSUPPORTED
    # an empty batch is no work
    assert lib.gsw_extract_l(p, N.GSW_F32, key, nonce, 8, p, None, p, 0, 16, 2, None) == N.GSW_OK
    assert lib.gsw_version() == 500


def test_library_exports_the_three_symbols():
    from gswm_amd import _native as N
    lib = N.lib()
    for name in ("gsw_embed_l", "gsw_extract_l", "gsw_quant_pack"):
        assert name in N.exported_symbols()
        assert getattr(lib, name).argtypes[-2] is ctypes.c_int            # int l, then the stream
        assert getattr(lib, name).argtypes[-1] is ctypes.c_void_p


def test_cli_parsers_carry_l_through():
    from gswm_amd import extract, trace
    ex = [a for a in extract.build_parser()._actions if "--l" in a.option_strings]
    assert len(ex) == 1 and ex[0].type is int and ex[0].default == 1
    base = ["--registry", "r.tsv", "--key_hex", "00" * 32, "--nonce_hex", "00" * 16]
    assert trace.build_parser().parse_args(base).l == 1
    assert trace.build_parser().parse_args(base + ["--l", "4"]).l == 4
    with pytest.raises(SystemExit):
        trace.build_parser().parse_args(base + ["--l", "3"])


def test_wrappers_pass_l_to_the_codec(monkeypatch):
    """the twins of the reference's functions hand their l to codec.embed_batch / extract_batch / quant_pack unchanged"""
    import torch
    from gswm_amd import codec, extract, gs_insert, trace
    seen = []

    def fake_extract(z, key, nonce, m, *, return_counts=False, l=1):
        seen.append(("extract", l))
        B = z.shape[0]
        r = (torch.zeros(B, (m + 7) // 8, dtype=torch.uint8), torch.zeros(B, dtype=torch.int32))
        return (*r, torch.zeros(B, m, dtype=torch.int32)) if return_counts else r

    def fake_embed(key, nonce, k, batch, shape, **kw):
        seen.append(("embed", kw.get("l", 1)))
        return torch.zeros(batch, *shape, dtype=kw.get("dtype", torch.float32))

    monkeypatch.setattr(codec, "extract_batch", fake_extract)
    monkeypatch.setattr(codec, "embed_batch", fake_embed)
    monkeypatch.setattr(codec, "mt19937_uniform", lambda n, rng=None, device="cuda": torch.zeros(n, dtype=torch.float64))
    ns = types.SimpleNamespace(key=bytes(32), nonce=bytes(16), l=4, message_length=8)
    assert extract.recover_exactracted_message(torch.zeros(4, 2, 2), ns, device="cpu") == "0" * 8
    assert extract.recover_exactracted_message_batch(torch.zeros(2, 4, 2, 2), ns) == ["0" * 8] * 2
    del ns.l                                                                              # the reference's default
    extract.recover_exactracted_message(torch.zeros(4, 2, 2), ns, device="cpu")
    opt = types.SimpleNamespace(key_hex="00" * 32, nonce_hex="00" * 16)
    gs_insert.gs_watermark_init_noise(opt, "m", log_path=None, device="cpu", l=2)
    gs_insert.gs_watermark_init_noise_batch(opt, "m", 3, seed=7, device="cpu", l=4)
    gs_insert.gs_watermark_init_noise_batch(opt, "m", 3, seed=7, device="cpu")
    assert seen == [("extract", 4), ("extract", 4), ("extract", 1), ("embed", 2), ("embed", 4), ("embed", 1)]
