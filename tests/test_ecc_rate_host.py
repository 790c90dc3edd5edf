"""CPU (no GPU): punctured payload codes -- the sizes, N(T), the host encoder against the restatement of
tests/ecc_rate_reference.py, the unchanged "conv" forms, refusals, the C ABI, the zero-filled equivalence with the two older restatements, and the recorded
outcome of the rate walk with its conditions."""
import inspect
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ecc_list_reference as LR
import ecc_rate_reference as Q
import ecc_reference as R
from conftest import ROOT

PUNCTURED = ("conv23", "conv34")


@pytest.fixture(scope="module")
def E():
    import gswm_amd  # noqa: F401
    from gswm_amd import ecc
    return ecc


# ------------------------------------------------------------------------------------------------ sizes
def test_the_size_table_of_the_issue(E):
    from gswm_amd import codec
    assert E.CODES == Q.CODES == codec.VITERBI_CODES == ("conv", "conv23", "conv34")
    for M, caps in ((64, (1, 2, 3)), (256, (13, 18, 21)), (2048, (125, 167, 189)), (8192, (509, 679, 765))):
        assert tuple(E.capacity(M, c) for c in E.CODES) == caps == tuple(Q.capacity(M, c) for c in Q.CODES)
    for M, code, T, N, spare in ((64, "conv23", 40, 60, 4), (64, "conv34", 48, 64, 0), (80, "conv34", 56, 75, 5), (256, "conv23", 168, 252, 4)):
        assert Q.sizes(M, code) == (T - 6, T, N, T // 8 - 3) and M - N == spare
        assert E.trellis_steps(M, code) == codec.viterbi_steps(M, code) == T and E.kept_bits(T, code) == codec.viterbi_kept_bits(T, code) == N
        assert E.info_bits(M, code) == T - 6 and E.capacity(M, code) == T // 8 - 3
    assert Q.sizes(80, "conv34")[1] % 3 == 2                        # the tail steps fall inside a period
    for M in range(64, 8193, 16):
        for code in E.CODES:
            I, T, N, pb = Q.sizes(M, code)
            assert (E.info_bits(M, code), E.trellis_steps(M, code), E.capacity(M, code)) == (I, T, pb)
            assert T % 8 == 0 and N <= M < Q.kept_bits(code, T + 8) and I - 16 - 8 * pb == 2      # the pad is 2 bits at every M and every code
            if code == "conv":
                assert (I, T, pb) == R.sizes(M) and N == M


def test_kept_bits_against_a_brute_force_count(E):
    from gswm_amd import codec
    for code in E.CODES:
        pat = Q.PATTERN[code]
        assert E.PATTERNS[code] == pat
        n = 0
        for t in range(0, 700):
            assert Q.kept_bits(code, t) == E.kept_bits(t, code) == codec.viterbi_kept_bits(t, code) == n, (code, t)
            n += len(pat[t % len(pat)])
    assert [len(Q.PATTERN[c]) for c in Q.CODES] == [1, 2, 3] and Q.PATTERN["conv34"] == ((0, 1), (1,), (0,))


# ------------------------------------------------------------------------------------------------ the encoder
@pytest.mark.parametrize("M", [64, 80, 256, 2048, 8192])
def test_encode_equals_the_restatement(E, M):
    rng = np.random.default_rng(M)
    for code in E.CODES:
        for _ in range(3):
            p = rng.bytes(Q.capacity(M, code))
            msg = E.encode(p, M, code)
            assert msg == E.encode(p, M, code=code) == Q.encode(p, M, code) and len(msg) == M // 8
            bits = np.unpackbits(np.frombuffer(msg, dtype=np.uint8))
            spare = np.setdiff1d(np.arange(M), Q.layout(M, code)[2])
            assert len(spare) == M - Q.sizes(M, code)[2] and not bits[spare].any()      # spare positions carry 0
        if code == "conv":
            assert msg == R.encode(p, M) == E.encode(p, M)


def test_a_noiseless_codeword_reads_back_in_the_restatement():
    rng = np.random.default_rng(5)
    for M in (64, 80, 256):
        for code in PUNCTURED:
            sent = [rng.bytes(Q.capacity(M, code)) for _ in range(3)]
            sc = np.stack([R.score_of(Q.encode(p, M, code), 3) for p in sent])
            for L in (1, 4):
                d = Q.decode_list(sc, L, code)
                assert Q.payloads(d["info"], M, code) == sent and d["ok"].all() and not d["flips"].any() and not d["rank"].any()
                assert d["metric"].tolist() == [3 * Q.sizes(M, code)[2]] * 3
                assert [bytes(m) for m in d["message"]] == [Q.encode(p, M, code) for p in sent]


# ------------------------------------------------------------------------------------------------ "conv" is today's call
def test_at_conv_every_new_keyword_function_equals_its_old_call(E):
    from gswm_amd import codec, detect as D, issue as I, pipeline as P
    for M in (64, 80, 256, 2048, 8192):
        assert E.info_bits(M, "conv") == E.info_bits(M) == M // 2 - 6 and E.capacity(M, "conv") == E.capacity(M) == R.capacity(M)
        p = bytes(range(256))[:E.capacity(M)] * 1 if E.capacity(M) <= 256 else os.urandom(E.capacity(M))
        assert E.check_payload(p, M, "conv") == E.check_payload(p, M) == p
        assert E.encode(p, M, "conv") == E.encode(p, M) == R.encode(p, M)
        assert E.pad_payload("ab", M, "conv") == E.pad_payload("ab", M) and E.pad_payload(b"x" * 2000, M, code="conv") == E.pad_payload(b"x" * 2000, M)
        for L in (1, 2, 4, 8):
            assert codec.viterbi_list_wave_lds(M, L, "conv") == codec.viterbi_list_wave_lds(M, L) == LR.wave_lds(M, L)
    for fn in (E.info_bits, E.capacity, E.check_payload, E.encode, E.pad_payload, E.read, E.read_list, E.read_any, E.list_read_from_decode, codec.viterbi_decode,
               codec.viterbi_list_decode, codec.viterbi_list_wave_lds):
        assert inspect.signature(fn).parameters["code"].default == "conv", fn.__name__
    assert inspect.signature(D.detect_payloads).parameters["ecc"].default == "conv"
    assert inspect.signature(I.issue_latents).parameters["ecc"].default is None
    assert inspect.signature(P.GaussianShadingPipeline.verify_records).parameters["ecc"].default is None
    # the host side of the reads and their text
    d = LR.decode_list(np.stack([R.score_of(R.encode(b"P" * 13, 256), 2)] * 2), 4)
    ns = SimpleNamespace(**{k: (torch.from_numpy(v) if k == "message" else v) for k, v in d.items()})
    old, new = E.list_read_from_decode(ns, 256), E.list_read_from_decode(ns, 256, "conv")
    assert old[:4] == new[:4] and old[5:] == new[5:] and old.payload == [b"P" * 13] * 2 and type(new) is E.EccListRead
    assert E.EccRead._fields == ("payload", "ok", "flips", "metric", "message") and E.EccListRead._fields == E.EccRead._fields + ("rank", "n_ok")
    assert E.format_read(old, 0, 256) == E.format_read(old, 0, 256, "conv") == f"payload {(b'P' * 13).hex()} crc ok, corrected 0 of 256"
    assert E.format_read_list(old, 1, 256, 4, "conv") == E.format_read_list(old, 1, 256, 4) == LR.format_read_list(d, 1, 256, 4)
    assert E.format_any(old, 0, 256, 4, "conv") == E.format_any(old, 0, 256, 4)
    # a punctured read's text counts over N
    d = Q.decode_list(np.stack([R.score_of(Q.encode(b"Q" * 18, 256, "conv23"), 2)]), 2, "conv23")
    ns = SimpleNamespace(**{k: (torch.from_numpy(v) if k == "message" else v) for k, v in d.items()})
    r = E.list_read_from_decode(ns, 256, "conv23")
    assert r.payload == [b"Q" * 18] and E.format_any(r, 0, 256, 2, "conv23") == Q.format_read(d, 0, 256, "conv23", 2) == \
        f"payload {(b'Q' * 18).hex()} crc ok, corrected 0 of 252, list rank 0 of 2"
    assert E.format_read(r, 0, 256, "conv34").endswith("of 256") and E.format_read(r, 0, 80, "conv34").endswith("of 75")


# ------------------------------------------------------------------------------------------------ refusals
def test_wrong_payload_lengths_and_unknown_codes_are_refused(E):
    from gswm_amd import codec, detect as D, issue as I
    for code in E.CODES:
        cap = E.capacity(256, code)
        for n in (cap - 1, cap + 1, 0):
            with pytest.raises(ValueError, match=f"exactly {cap}"):
                E.encode(b"x" * n, 256, code)
            with pytest.raises(ValueError, match=f"exactly {cap}"):
                E.check_payload(b"x" * n, 256, code)
        assert len(E.pad_payload("a" * 40, 256, code)) == cap == len(E.pad_payload("", 256, code))
        with pytest.raises(ValueError, match="bytes"):
            E.encode("text", 256, code)
    with pytest.raises(ValueError, match="exactly 13"):
        E.encode(b"u" * 18, 256)                                    # a UUID and two bytes: not under "conv"
    assert len(E.encode(b"u" * 18, 256, "conv23")) == 32
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32)
    for bad in ("conv12", "CONV23", "", None, 1, b"conv23", ("conv",)):
        for call in (lambda: E.capacity(256, bad), lambda: E.info_bits(256, bad), lambda: E.encode(b"x" * 13, 256, bad), lambda: E.check_payload(b"x" * 13, 256, bad),
                     lambda: E.pad_payload("x", 256, bad), lambda: E.read(z(2, 256), bad), lambda: E.read_list(z(2, 256), 4, bad), lambda: E.read_any(z(2, 256), 1, bad),
                     lambda: E.read_any(z(2, 256), 8, bad), lambda: codec.viterbi_decode(z(2, 256), bad), lambda: codec.viterbi_list_decode(z(2, 256), 2, bad),
                     lambda: codec.viterbi_list_wave_lds(256, 2, bad)):
            with pytest.raises((ValueError, KeyError), match="code|conv"):
                call()
    for bad in ("conv12", 1, b"conv"):
        with pytest.raises(ValueError, match="ecc"):
            E.check_code(bad)
        with pytest.raises(ValueError, match="ecc"):
            I.encode_requests([], 32, bad)
        with pytest.raises(ValueError, match="ecc"):
            D.detect_payloads(torch.zeros(2, 4, 8, 8), D.Keyring(), 256, ecc=bad)
    assert [E.check_code(c) for c in E.CODES + (None,)] == list(E.CODES) + [None]
    for code in PUNCTURED:
        for M in (48, 72, 8208):
            with pytest.raises(ValueError, match="multiple of 16"):
                E.capacity(M, code)
            with pytest.raises(ValueError, match="multiple of 16"):
                codec.viterbi_decode(z(2, M), code)
        with pytest.raises(ValueError, match="LDS"):
            codec.viterbi_list_decode(z(1, Q.largest_served(4, code) + 16), 4, code)
        with pytest.raises(ValueError, match="8192"):
            E.read_list(z(1, 8208), 1, code)                        # the kernel serves it; a payload is not defined there
        for call in (lambda: E.read(z(2, 256), code), lambda: E.read_list(z(2, 256), 8, code), lambda: E.read_any(z(2, 256), 1, code),
                     lambda: codec.viterbi_list_decode(z(1, Q.largest_served(8, code)), 8, code), lambda: codec.viterbi_decode(z(1, 8192), code)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):    # served: the one thing missing is a device
                call()
    # requests: payloads of the code's capacity
    key, nonce = b"k" * 32, b"n" * 16
    for code, cap in (("conv", 13), ("conv23", 18), ("conv34", 21)):
        out = I.encode_requests([I.Request("u", b"p" * cap, key, nonce), I.Request("v", "text", key, nonce)], 32, code)
        assert [q.message for q in out] == [Q.encode(b"p" * cap, 256, code), Q.encode(b"text" + b"\0" * (cap - 4), 256, code)]
        with pytest.raises(ValueError, match=f"exactly {cap}"):
            I.encode_requests([I.Request("u", b"p" * (cap + 1), key, nonce)], 32, code)
        with pytest.raises(ValueError, match=f"at most {cap}"):
            I.encode_requests([I.Request("u", "p" * (cap + 1), key, nonce)], 32, code)


def test_command_lines_take_the_codes_and_keep_their_refusals(E, capsys):
    from gswm_amd import extract as X, detect as D, issue as I, trace as T
    base = ["--key_hex", "00" * 32, "--nonce_hex", "00" * 16, "--message_length", "256"]
    for code in E.CODES:
        cap = E.capacity(256, code)
        coded = E.encode(b"P" * cap, 256, code).hex()
        for vote in ([], ["--soft", "1"], ["--robust", "1"], ["--robust_soft", "7"], ["--window_soft", "7", "--l", "2"]):
            a = X.build_parser().parse_args(base + ["--original_message_hex", coded, "--ecc", code, "--ecc_list", "4"] + vote)
            assert a.ecc == code and a.ecc_list == 4 and X._ecc_wanted(a) == code
        a = X.build_parser().parse_args(base + ["--original_payload_hex", (b"P" * cap).hex(), "--ecc", code])
        assert a.original_message_hex == coded                      # --original_payload_hex is encoded under the code
        with pytest.raises(SystemExit):
            X.build_parser().parse_args(base + ["--original_payload_hex", (b"P" * (cap + 1)).hex(), "--ecc", code])
        assert f"exactly {cap}" in capsys.readouterr().err           # ... and checked against the code's capacity
        for extra, names in ((["--align", "d4"], ("--ecc", "--align")), (["--align", "flips", "--align_shift", "1"], ("--ecc", "--align")),
                             (["--gpus", "2"], ("--ecc", "--gpus"))):
            with pytest.raises(SystemExit):
                X.build_parser().parse_args(base + ["--original_message_hex", coded, "--ecc", code] + extra)
            err = capsys.readouterr().err
            assert all(n in err for n in names), (extra, err)
        ring = ["--keyring", "k.tsv"]
        for stat in ([], ["--reliability", "15"], ["--window_reliability", "7", "--l", "2"]):
            a = D.build_parser().parse_args(ring + ["--ecc", code, "--ecc_list", "8"] + stat)
            assert a.ecc == code and a.ecc_list == 8 and D.ecc_refusal(a) is None
        for extra, flag in ((["--align", "d4"], "--align"), (["--align_shift", "1"], "--align_shift"), (["--align_reliability", "7"], "--align_reliability")):
            a = D.build_parser().parse_args(ring + ["--ecc", code] + extra)
            assert "--ecc" in D.ecc_refusal(a) and flag in D.ecc_refusal(a)
    for parser, head in ((X.build_parser, base + ["--original_message_hex", "00" * 32]), (D.build_parser, ["--keyring", "k.tsv"])):
        with pytest.raises(SystemExit):
            parser().parse_args(head + ["--ecc", "conv56"])
        assert "--ecc" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        X.build_parser().parse_args(base + ["--original_message_hex", "00" * 32, "--ecc_list", "4"])
    assert "--ecc conv" in capsys.readouterr().err                   # the standing refusal, word for word
    assert "--ecc_list above 1 needs --ecc conv" in D.ecc_refusal(D.build_parser().parse_args(["--keyring", "k.tsv", "--ecc_list", "4"]))
    assert "choices=_ecc.CODES" in open(I.__file__).read()          # issue --ecc takes every code
    assert "--ecc is not a trace flag" in open(T.__file__).read()    # trace has no --ecc


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbols_are_exported_and_prototyped():
    import ctypes
    from gswm_amd import _native as N
    lib = N.lib()
    for name, n, ints in (("gsw_viterbi_decode_rate", 11, (2, 3, 4)), ("gsw_viterbi_list_decode_rate", 14, (2, 3, 4, 5))):
        assert name in N.exported_symbols() and hasattr(lib, name)
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n and fn.argtypes[1] is ctypes.c_int64 and all(fn.argtypes[i] is ctypes.c_int for i in ints)
    assert len(lib.gsw_viterbi_decode.argtypes) == 10 and len(lib.gsw_viterbi_list_decode.argtypes) == 13      # the older symbols are as they were
    hdr = open(os.path.join(ROOT, "include", "gswm.h")).read()
    assert ("int gsw_viterbi_decode_rate(const int32_t* score_dev, int64_t score_stride, int B, int message_bits, int rate, uint8_t* info_dev, "
            "uint8_t* message_dev,\n") in hdr
    assert "int gsw_viterbi_list_decode_rate(const int32_t* score_dev, int64_t score_stride, int B, int message_bits, int rate, int list_size,\n" in hdr
    import __graft_entry__ as G
    assert "gswm_viterbi_rate_plan.h" in G.HEADERS
    csrc = os.path.join(ROOT, "a-watermark-for-diffusion-models_amd", "csrc")
    assert "gswm_viterbi_rate_plan.h" in open(os.path.join(csrc, "Makefile")).read().split("\n\t")[0]
    src = open(os.path.join(csrc, "gswm_kernels.hip")).read()
    assert src.index('#include "gswm_viterbi_plan.h"') < src.index('#include "gswm_viterbi_rate_plan.h"') < src.index('#include "gswm_viterbi.inc"')
    m = open(os.path.join(csrc, "gswm.map")).read()
    assert "gsw_viterbi_decode_rate" in m and "gsw_viterbi_list_decode_rate" in m


# ------------------------------------------------------------------------------------------------ the second restatement, for free
def _noisy_rows(M, code, B, seed):
    rng = np.random.default_rng(seed)
    sc = rng.integers(-12, 13, (B, M)).astype(np.int32)                                          # pure noise
    for b in range(B // 2):                                                                       # codewords of amplitude 6 under uniform noise of -6 .. 6
        sc[b] = R.score_of(Q.encode(rng.bytes(Q.capacity(M, code)), M, code), 6) + rng.integers(-6, 7, M)
    sc[-1] = rng.integers(-1, 2, M)                                                               # ties
    return sc


@pytest.mark.parametrize("code", PUNCTURED)
@pytest.mark.parametrize("M", [64, 80, 256, 272, 2048])
def test_the_zero_filled_row_decodes_the_same_under_the_older_restatements(M, code):
    """Spread the N votes into a row of 2 T entries with zeros at the punctured outputs and no interleaver: `ecc_reference.decode(interleave=False)` gives the
    same info, metric and ok, and `ecc_list_reference.decode_list(interleave=False)` (its restatements do take un-interleaved rows) the same list outputs.
    Wherever 2 T is a length they accept: T >= 32, and 2 T <= 8192 for the plain one."""
    I, T, N, pb = Q.sizes(M, code)
    assert T >= 32 and 2 * T <= 8192 and (2 * T) % 16 == 0
    sc = _noisy_rows(M, code, 6 if M < 2048 else 3, M + len(code))
    row = Q.spread(sc, code)
    assert row.shape == (len(sc), 2 * T) and (row != 0).sum() <= N * len(sc) and np.abs(row).sum() == np.abs(sc[:, Q.layout(M, code)[2]].astype(np.int64)).sum()
    mine, older = Q.decode(sc, code), R.decode(row, interleave=False)
    for k in ("info", "metric", "ok"):
        assert np.array_equal(mine[k], older[k]), (M, code, k)
    assert mine["ok"][:len(sc) // 2].any()                          # some of the noisy codewords do read back: the comparison is not of failures only
    for L in ((2, 8) if M < 2048 else (4,)):
        mine, older = Q.decode_list(sc, L, code), LR.decode_list(row, L, interleave=False)
        for k in ("info", "metric", "ok", "rank", "n_ok"):
            assert np.array_equal(mine[k], older[k]), (M, code, L, k)
    if M <= 80:
        older = LR.decode_list_plain(row[:2], 4, interleave=False)
        mine = Q.decode_list(sc[:2], 4, code)
        for k in ("info", "metric", "ok", "rank", "n_ok"):
            assert np.array_equal(mine[k], older[k]), (M, code, "plain restatement", k)
    # at "conv" the restatement IS the older ones, message and flips included
    mine, older = Q.decode_list(sc, 2, "conv"), LR.decode_list(sc, 2)
    for k in LR.NAMES:
        assert np.array_equal(mine[k], older[k]), (M, k)
    plain = R.decode(sc) if M <= 8192 else None
    for k in Q.PLAIN:
        assert np.array_equal(Q.decode(sc, "conv")[k], plain[k]), (M, k)


def test_votes_at_spare_positions_are_not_read_by_the_restatement():
    for M, code in ((64, "conv23"), (80, "conv34"), (256, "conv23")):
        sc = _noisy_rows(M, code, 4, 3)
        spare = np.setdiff1d(np.arange(M), Q.layout(M, code)[2])
        loud = sc.copy()
        loud[:, spare] = 2 ** 20
        a, b = Q.decode_list(sc, 4, code), Q.decode_list(loud, 4, code)
        assert all(np.array_equal(a[k], b[k]) for k in Q.NAMES)


# ------------------------------------------------------------------------------------------------ the walk
def test_the_rate_walk_fixes_the_end_to_end_noise():
    """Per code the recorded sigma is the LARGEST grid point at which all 20 payloads read back at L = 1; the list point (all 20 at L = 8, fewer at L = 1) does
    not exist for either punctured code under the recorded draws, so the list end-to-end tests run at the L = 1 point.  Conditions on the chosen inputs (not
    tolerances): at no grid point, code or L has an image ok on a wrong payload, and none of the 64 blank latents has ok.  The committed table is what the tool
    writes."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import ecc_rate_sigma_walk as W
    finally:
        sys.path.pop(0)
    walks, uncoded = W.walks_of_all_codes()
    print(walks, uncoded)
    for code in Q.CODES:
        assert sorted(walks[code]) == [1, 2, 4, 8]
        for L, (table, blank_ok) in walks[code].items():
            assert [s for s, _, _ in table] == R.WALK["sigmas"]
            assert all(wrong == 0 for _, _, wrong in table), (code, L, table)
            assert blank_ok == 0, (code, L)
        assert all(a <= b for L, K in ((1, 2), (2, 4), (4, 8)) for (_, a, _), (_, b, _) in zip(walks[code][L][0], walks[code][K][0]))
    assert Q.chosen_sigmas(walks["conv"])[0] == R.WALK["sigma"] == 2.5                            # a fresh payload draw, the same point as section 4.29's
    for code in PUNCTURED:
        rec = Q.RATE_WALK[code]
        assert Q.chosen_sigmas(walks[code]) == (rec["sigma"], rec["list_sigma"]) == (1.75, None)
        at = {L: next(r for s, r, _ in walks[code][L][0] if s == rec["sigma"]) for L in LR.LIST_SIZES}
        assert at == rec["reads"] and at[1] == R.WALK["images"] == 20
        nxt = next(r for s, r, _ in walks[code][1][0] if s == rec["sigma"] + 0.25)
        assert nxt < 20                                             # the next grid point loses images: the chosen one is the largest
    assert uncoded == [u for _, _, u in R.walk()]
    assert open(os.path.join(ROOT, "profiles", "ecc_rate_sigma_walk.txt")).read() == W.report(walks, uncoded)
