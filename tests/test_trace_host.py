"""CPU (no GPU): the host side of tracing -- the NumPy top-k oracle against a pure-Python brute force, registry packing and files,
the exact binomial statistics against an independent rational sum, the argument validation of the two C entry points, the CLI parser."""
import ctypes
import math
import types
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
import pytest

from conftest import README_KEY, README_NONCE

import gswm_amd
from gswm_amd import _native as N, codec, gs_insert, trace as T

INT32_MIN = -2 ** 31


# ------------------------------------------------------------------------------------------------------------ top-k oracle
def brute_force(counts, V, messages, k, soft):
    """three loops, Python integers, explicit bit extraction (bit t -> byte t >> 3, bit 7 - (t & 7))"""
    out_idx, out_score = [], []
    for row in counts:
        scored = []
        for u, msg in enumerate(messages):
            s = 0
            for t, c in enumerate(row):
                c = int(c)
                w = (2 * c - V) if soft else (1 if c > V / 2 else -1)
                r = (msg[t >> 3] >> (7 - (t & 7))) & 1
                s += (2 * r - 1) * w
            scored.append((-s, u))
        scored.sort()
        scored = scored[:k]
        out_idx.append([u for _, u in scored] + [-1] * (k - len(scored)))
        out_score.append([-s for s, _ in scored] + [INT32_MIN] * (k - len(scored)))
    return np.array(out_idx, dtype=np.int32), np.array(out_score, dtype=np.int32)


@pytest.mark.parametrize("soft", [True, False])
@pytest.mark.parametrize("U,M,B,V,k", [(5, 16, 3, 4, 2), (9, 8, 2, 5, 8), (3, 24, 4, 1, 4), (17, 40, 2, 130, 3), (1, 8, 1, 2, 1)])
def test_topk_host_matches_brute_force(U, M, B, V, k, soft):
    rng = np.random.default_rng(U * 100 + M + V)
    reg = rng.integers(0, 256, (U, M // 8), dtype=np.uint8)
    counts = rng.integers(0, V + 1, (B, M))
    idx, score = T.topk_host(counts, V, reg, k, soft)
    want_idx, want_score = brute_force(counts, V, [bytes(r) for r in reg], k, soft)
    assert idx.dtype == np.int32 and score.dtype == np.int32
    assert np.array_equal(idx, want_idx) and np.array_equal(score, want_score)


@pytest.mark.parametrize("soft", [True, False])
def test_topk_host_ties_go_to_the_lower_index(soft):
    V, M = 4, 16
    counts = np.array([[4, 0, 4, 4, 0, 0, 4, 0, 2, 2, 4, 0, 4, 0, 0, 4]])          # bits 8, 9 carry no margin (w = 0 soft; a tie -> 0 hard)
    base = np.packbits(np.array([1, 0, 1, 1, 0, 0, 1, 0, 0, 0, 1, 0, 1, 0, 0, 1], dtype=np.uint8))
    other = base.copy()
    other[1] ^= 0xC0 if soft else 0x00                                             # differs only where w = 0 (soft)
    far = base ^ 0xFF
    reg = np.stack([far, other, base, other] if soft else [far, base, base, far])
    idx, score = T.topk_host(counts, V, reg, 3, soft)
    bi, bs = brute_force(counts, V, [bytes(r) for r in reg], 3, soft)
    assert np.array_equal(idx, bi) and np.array_equal(score, bs)
    assert idx[0].tolist() == ([1, 2, 3] if soft else [1, 2, 0])
    assert score[0, 0] == score[0, 1]


def test_topk_host_pads_past_the_registry():
    idx, score = T.topk_host(np.array([[1, 0, 1, 1, 0, 0, 1, 0]]), 1, np.array([[0xB2], [0x4D]], dtype=np.uint8), 4, True)
    assert idx.tolist() == [[0, 1, -1, -1]] and score.tolist() == [[8, -8, INT32_MIN, INT32_MIN]]


# ------------------------------------------------------------------------------------------------------------ registry
def test_registry_row_is_what_gs_insert_embeds():
    r = T.Registry()
    assert r.add("u", "lthero") == 0
    row = r.packed()[0]
    assert row.tobytes() == codec.pad_message("lthero") == r.message("u")
    bits = codec.bits_to_str(row)
    assert len(bits) == 256 and all(int(bits[t]) == (row[t >> 3] >> (7 - (t & 7))) & 1 for t in range(256))
    assert bits == "".join(str(b) for b in np.unpackbits(row))
    long = T.Registry()
    long.add("v", "x" * 40)
    assert long.message("v") == b"x" * 32                                    # cut like pad_message


def test_registry_tiled_to_a_longer_message_length_keeps_the_soft_scores():
    rng = np.random.default_rng(1)
    r = T.Registry()
    for i in range(20):
        r.add(f"u{i}", bytes(rng.integers(0, 256, 32, dtype=np.uint8)))
    V = 16
    split = rng.integers(0, V + 1, (3, 1024))                                 # votes of the four repeats, counted apart (V each)
    summed = split.reshape(3, 4, 256).sum(axis=1)                             # the same votes counted at 256 bits (4 V each)
    wide = r.packed(1024)
    assert wide.shape == (20, 128) and np.array_equal(wide[:, :32], r.packed()) and np.array_equal(wide[:, 96:], r.packed())
    a = T.topk_host(split, V, wide, 5, True)
    b = T.topk_host(summed, 4 * V, r.packed(), 5, True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    with pytest.raises(ValueError, match="multiple"):
        r.packed(384)


def test_registry_save_load_round_trip(tmp_path):
    r = T.Registry()
    r.add("alice", "lthero")
    r.add("bob smith", bytes(range(32)))
    p = tmp_path / "reg.txt"
    r.save(p)
    assert p.read_text() == f"alice\t{codec.pad_message('lthero').hex()}\nbob smith\t{bytes(range(32)).hex()}\n"
    q = T.Registry.load(p)
    assert q.user_ids == ["alice", "bob smith"] and np.array_equal(q.packed(), r.packed()) and q.message_bits == 256
    assert T.detect_format(p) == "registry"
    assert T.Registry.from_file(p).user_ids == q.user_ids


def test_registry_from_info_data(tmp_path):
    log = tmp_path / "info_data.txt"
    k1, n1 = bytes.fromhex(README_KEY), bytes.fromhex(README_NONCE)
    k2, n2 = bytes(range(32)), bytes(range(16))
    m = [codec.pad_message(s) for s in ("one", "two", "three")]
    gs_insert._write_info(log, k1, n1, m[0])
    gs_insert._write_info(log, k2, n2, m[1])
    gs_insert._write_info(log, k1, n1, m[2], extra=["use_seed: 1"])
    gs_insert._write_info(log, k1, n1, m[0])                                  # the same message issued again
    gs_insert._write_info(log, k1, n2, m[1])                                  # same key, other nonce
    assert T.detect_format(log) == "info_data"
    r = T.Registry.from_info_data(log, key=k1, nonce=n1)
    assert r.user_ids == ["info:1", "info:3"] and [r.message(u) for u in r.user_ids] == [m[0], m[2]]
    assert T.Registry.from_info_data(log, key=k2.hex(), nonce=n2.hex()).user_ids == ["info:2"]
    assert T.Registry.from_file(log, k1, n1).user_ids == ["info:1", "info:3"]
    assert T.Registry.from_info_data(log).user_ids == ["info:1", "info:2", "info:3"]
    with pytest.raises(ValueError, match="no record"):
        T.Registry.from_info_data(log, key=bytes(32), nonce=n1)


def test_registry_refuses_by_name():
    r = T.Registry()
    r.add("alice", "lthero")
    with pytest.raises(ValueError, match="'alice' is already registered"):
        r.add("alice", "something else")
    with pytest.raises(ValueError, match="'bob'.*already registered to 'alice'"):
        r.add("bob", codec.pad_message("lthero"))
    with pytest.raises(ValueError, match="'carol'.*31 bytes"):
        r.add("carol", bytes(31))
    with pytest.raises(ValueError, match="'dave'.*empty"):
        r.add("dave", "")
    with pytest.raises(ValueError):
        r.add("tab\tid", "x")
    assert len(r) == 1


# ------------------------------------------------------------------------------------------------------------ statistics
getcontext().prec = 400


def _log10_exact(p: Fraction) -> float:
    return float((Decimal(p.numerator) / Decimal(p.denominator)).log10())


def _close(a, b):
    return a == b or abs(a - b) <= 1e-12 * abs(b)


def _bin_tail(n, x0, q: Fraction) -> Fraction:
    return sum((Fraction(math.comb(n, x)) * q ** x * (1 - q) ** (n - x) for x in range(max(x0, 0), n + 1)), Fraction(0))


@pytest.mark.parametrize("n", [8, 63, 256])
def test_log10_p_soft_is_the_exact_binomial_tail(n):
    assert T.log10_p_soft(n, n) == -n * math.log10(2) or _close(T.log10_p_soft(n, n), -n * math.log10(2))
    assert T.log10_p_soft(-n, n) == 0.0
    last = 0.0
    for score in range(-n, n + 1, 2):
        got = T.log10_p_soft(score, n)
        assert _close(got, _log10_exact(_bin_tail(n, (score + n) // 2, Fraction(1, 2)))), score
        assert got <= last
        last = got
    assert T.log10_p_soft(n + 2, n) == -math.inf


def test_log10_p_soft_endpoints_and_scale():
    for n in (8, 63, 256, 16384):
        assert _close(T.log10_p_soft(n, n), -n * math.log10(2))
        assert T.log10_p_soft(-n, n) == 0.0
    assert -0.31 < T.log10_p_soft(0, 16384) < -0.29                          # just over one half
    assert T.log10_p_soft(6554, 16384) < -500


@pytest.mark.parametrize("M,V", [(16, 4), (16, 5), (64, 64)])
def test_log10_p_hard_is_the_dominating_binomial_tail(M, V):
    tie = Fraction(math.comb(V, V // 2), 2 ** V) if V % 2 == 0 else Fraction(0)
    q = (1 + tie) / 2
    assert Fraction(*T.hard_match_probability(V)) == q
    last = 0.0
    for agree in range(0, M + 1):
        got = T.log10_p_hard(agree, M, V)
        assert _close(got, _log10_exact(_bin_tail(M, agree, q))), agree
        fair = _log10_exact(_bin_tail(M, agree, Fraction(1, 2)))
        assert got >= fair or _close(got, fair)                              # the conservative side
        assert got <= last
        last = got
    assert T.log10_p_hard(0, M, V) == 0.0


def test_bonferroni_bound():
    assert T.log10_p_any(-10.0, 1000) == -7.0
    assert T.log10_p_any(-2.0, 1000) == 0.0


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_trace_entry_points_validate_before_any_hip_call():
    lib, p = N.lib(), ctypes.c_void_p(16)
    BAD, UNS = N.GSW_ERR_BAD_ARG, N.GSW_ERR_UNSUPPORTED

    def call(counts=p, B=2, M=256, V=64, mode=N.GSW_TRACE_SOFT, reg=p, U=100, k=4, idx=p, score=p, ws=p):
        return lib.gsw_trace_topk(counts, B, M, V, mode, reg, U, k, idx, score, ws, None)

    for name in ("counts", "reg", "idx", "score", "ws"):
        assert call(**{name: None}) == BAD, name
    assert call(B=0) == BAD and call(B=-1) == BAD
    for M in (0, 7, 4, 2049, 2056, 250, -8):
        assert call(M=M) == BAD, M
    assert call(V=0) == BAD and call(V=-3) == BAD
    assert call(k=0) == BAD and call(k=9) == BAD
    assert call(U=0) == BAD and call(U=-5) == BAD and call(U=2 ** 31) == BAD
    assert call(mode=2) == BAD and call(mode=-1) == BAD
    assert call(M=2048, V=2 ** 20) == UNS and call(M=8, V=2 ** 28) == UNS      # msg_bits * copies >= 2^31
    assert call(M=8, V=2 ** 28, mode=N.GSW_TRACE_HARD) == UNS
    assert N.GSW_TRACE_SOFT == 0 and N.GSW_TRACE_HARD == 1
    assert lib.gsw_version() == 500


def test_trace_workspace_is_monotone():
    lib = N.lib()
    f = lib.gsw_trace_workspace_bytes
    assert f(1, 1, 1) > 0
    Bs, Us, ks = (1, 3, 16, 17, 64, 130, 1000), (1, 63, 256, 257, 4097, 2 ** 17 + 3, 2 ** 24, 2 ** 31 - 1), (1, 2, 4, 8)
    for U in Us:
        for k in ks:
            v = [f(B, U, k) for B in Bs]
            assert v == sorted(v) and v[0] > 0
    for B in Bs:
        for k in ks:
            v = [f(B, U, k) for U in Us]
            assert v == sorted(v)
        for U in Us:
            v = [f(B, U, k) for k in ks]
            assert v == sorted(v) and len(set(v)) == len(v)
    assert f(0, 10, 1) == 0 and f(1, 0, 1) == 0 and f(1, 10, 9) == 0 and f(1, 2 ** 31, 1) == 0
    assert f(64, 2 ** 24, 8) <= 4 << 20                                       # a few MiB at the largest benchmark size: partial lists, not scores


def test_vote_copies():
    assert codec.vote_copies(16384, 256) == 64 and codec.vote_copies(16384, 1024) == 16
    assert codec.vote_copies(4 * 96 * 96, 256) == 144 and codec.vote_copies(1021, 8) == 128     # padded to whole bytes
    with pytest.raises(IndexError):
        codec.vote_copies(16384, 1000)
    with pytest.raises(IndexError):
        codec.vote_copies(1700, 32)                                           # 1704 % 32, as gsw_extract refuses it


def test_trace_topk_has_no_cpu_path():
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.trace_topk(torch.zeros(1, 256, dtype=torch.int32), 64, torch.zeros(4, 32, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------------------ CLI
def test_cli_parser(tmp_path):
    P = T.build_parser()
    a = P.parse_args(["--key_hex", README_KEY, "--nonce_hex", "", "--registry", "r.txt"])
    assert (a.fpr, a.top, a.hard, a.message_length, a.batch_size, a.num_inference_steps, a.scheduler) == (1e-6, 1, False, None, 16, 30, "DDIM")
    assert a.model_id == "stabilityai/stable-diffusion-2-1-base" and a.allow_synthetic_weights is False and a.strict_kernels is None
    assert a.images_directory_path == "" and a.single_image_path == "" and int(a.is_traverse_subdirectories) == 0
    assert not hasattr(a, "original_message_hex")
    b = P.parse_args(["--key_hex", "00", "--nonce_hex", "11", "--registry", "x", "--fpr", "1e-9", "--top", "8", "--hard", "--message_length", "1024",
                      "--allow_synthetic_weights", "--strict_kernels", "0", "--batch_size", "64", "--images_directory_path", "d", "--is_traverse_subdirectories", "1"])
    assert (b.fpr, b.top, b.hard, b.message_length, b.batch_size, b.strict_kernels) == (1e-9, 8, True, 1024, 64, 0)
    for bad in (["--key_hex", "00", "--nonce_hex", ""], ["--key_hex", "00", "--nonce_hex", "", "--registry", "x", "--top", "9"]):
        with pytest.raises(SystemExit):
            P.parse_args(bad)
    assert "--gpus" in P.format_help() and "per-user keys" in P.format_help()      # said to be out of scope


def test_format_line():
    c = T.Candidate("alice", 3, 6000, 250, -400.0)
    d = T.Candidate("bob", 5, 10, 130, 0.0)
    assert T.format_line("a.png", T.TraceResult([c, d], "alice"), 256) == f"a.png, user: alice, agreement, {250 / 256}, log10 p, -400.000, next: bob ({130 / 256}, 0.000)"
    assert T.format_line("b.png", T.TraceResult([d], None), 256) == f"b.png, user: none, agreement, {130 / 256}, log10 p, 0.000"
    assert T.format_line("/x/c.png", ValueError("boom"), 256) == "Error processing /x/c.png: boom"


def test_package_lists_the_module():
    assert "trace" in gswm_amd.__all__ and gswm_amd.trace is T
