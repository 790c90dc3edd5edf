"""CPU (no GPU): the list read of error-corrected payloads before any device is asked -- the two restatements of tests/ecc_list_reference.py against each
other and against tests/ecc_reference.py at L = 1, the properties of a list, a planted case that only a list reads, the refusals of the library, the wrappers
and the command lines, the C prototype, and the walk that fixes the noise level of the end-to-end tests.

The walk (tools/ecc_list_sigma_walk.py, profiles/ecc_list_sigma_walk.txt; the setup of tests/ecc_reference.WALK: 4 x 32 x 32 latents, M = 256, 15 uniform
levels, 20 images per point, seed 20260429), payloads read back exactly with ok:

    sigma   0.50 .. 2.50  2.75  3.00  3.25  3.50  3.75  4.00
    L = 1        20         16    10     6     2     0     0
    L = 2        20         18    12     8     2     0     0
    L = 4        20         20    16     9     2     0     0
    L = 8        20         20    16     9     3     1     0

No image at any point has ok on a wrong payload at any L; none of the 64 blank latents has ok at any L.  Recorded sigma: 2.75, the largest point at which all 20
payloads read back at L = 8 and fewer than 20 (16) at L = 1."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ecc_list_reference as LR
import ecc_reference as R
import test_gpu_viterbi as V
from conftest import ROOT

PATTERNS = ("uniform", "hard", "ternary", "zeros", "code1", "codebig", "burst")
LENGTHS = (64, 80, 256)


@pytest.fixture(scope="module")
def E():
    import gswm_amd  # noqa: F401
    from gswm_amd import ecc
    return ecc


# ------------------------------------------------------------------------------------------------ the two restatements, and what a list is
@pytest.mark.parametrize("pattern", PATTERNS)
def test_the_two_restatements_agree_and_a_list_is_a_list(pattern):
    """`zeros` and `ternary` tie at nearly every merge: they pin the tie rule (d = 0 first, a predecessor's entries in their order) in both restatements"""
    for M in LENGTHS:
        sc = V._scores(pattern, 2, M)
        I, T, pb = LR.sizes(M)
        plain = R.decode(sc)
        pos = R.positions(M)
        for L in LR.LIST_SIZES:
            a, b = LR.decode_list(sc, L, all_ranks=True), LR.decode_list_plain(sc, L, all_ranks=True)
            for name in LR.NAMES + ("metrics", "inputs", "oks"):
                assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), (pattern, M, L, name)
            assert [a[n].dtype for n in LR.NAMES] == [np.uint8, np.uint8] + [np.int32] * 5
            # the L metrics are non-increasing and the L paths pairwise distinct
            assert (np.diff(a["metrics"], axis=1) <= 0).all(), (pattern, M, L)
            for row in a["inputs"]:
                assert len({r.tobytes() for r in row}) == L, (pattern, M, L)
            # each metric is the correlation of its re-encoded codeword with the scores; every path ends in the zero tail
            for r in range(L):
                msg = np.zeros((2, M), dtype=np.int64)
                msg[:, pos] = LR._recode(a["inputs"][:, r])
                assert np.array_equal(((2 * msg - 1) * sc).sum(axis=1), a["metrics"][:, r]), (pattern, M, L, r)
                assert not a["inputs"][:, r, I:].any()
            # rank 0 is the plain decode
            assert np.array_equal(np.packbits(a["inputs"][:, 0], axis=1), plain["info"]) and np.array_equal(a["metrics"][:, 0], plain["metric"])
            assert np.array_equal(a["oks"][:, 0], plain["ok"].astype(bool))
            # rank is the first passing rank, n_ok the count; the outputs describe that rank
            for i in range(2):
                passing = [r for r in range(L) if a["oks"][i, r]]
                assert a["n_ok"][i] == len(passing) and a["rank"][i] == (passing[0] if passing else 0) and a["ok"][i] == bool(passing)
                assert np.array_equal(a["info"][i], np.packbits(a["inputs"][i, a["rank"][i]])) and a["metric"][i] == a["metrics"][i, a["rank"][i]]
            if L == 1:
                for name in ("info", "message", "metric", "flips", "ok"):
                    assert a[name].dtype == plain[name].dtype and np.array_equal(a[name], plain[name]), (pattern, M, name)
                assert not a["rank"].any() and np.array_equal(a["n_ok"], a["ok"])


def test_a_longer_list_starts_with_the_shorter_one():
    """the L best paths through state 0 are the first L of the 2 L best: cutting every state's list to L loses none of them"""
    sc = V._scores("uniform", 3, 80)
    lists = {L: LR.decode_list(sc, L, all_ranks=True) for L in LR.LIST_SIZES}
    for L in (1, 2, 4):
        assert np.array_equal(lists[8]["metrics"][:, :L], lists[L]["metrics"]) and np.array_equal(lists[8]["inputs"][:, :L], lists[L]["inputs"])


def _planted(M=256):
    """votes under which the best path fails the CRC and the second best is what was sent: the sent codeword, with 6 of the 10 positions in which its
    nearest neighbour (one info bit flipped: the generators' impulse response, free distance 10) differs voted the neighbour's way"""
    payload = np.random.default_rng(11).bytes(R.capacity(M))
    info = R.info_word(payload, M)
    near = info.copy()
    near[40] ^= 1
    sent, other = R.encode_bits(info, M), R.encode_bits(near, M)
    diff = np.nonzero(sent != other)[0]
    assert len(diff) == 10
    score = (3 * (2 * sent.astype(np.int32) - 1)).astype(np.int32)
    score[diff[:6]] *= -1
    return payload, score[None, :], np.packbits(near)


def test_a_planted_case_reads_back_only_with_a_list(E):
    M = 256
    payload, score, near_info = _planted(M)
    one = R.decode(score)
    assert one["ok"].tolist() == [0] and np.array_equal(one["info"][0, :len(near_info)], near_info[:M // 16]) and R.payloads(one["info"], M) != [payload]
    assert one["metric"].tolist() == [3 * (M - 8)]                  # the neighbour: 4 of its 256 positions voted against it
    for L in (2, 4, 8):
        for d in (LR.decode_list(score, L), LR.decode_list_plain(score, L)):
            assert d["rank"].tolist() == [1] and d["ok"].tolist() == [1] and d["n_ok"].tolist() == [1] and d["metric"].tolist() == [3 * (M - 12)]
            assert d["flips"].tolist() == [6] and R.payloads(d["info"], M) == [payload]
            read = E.list_read_from_decode(SimpleNamespace(**{k: d[k] for k in LR.NAMES}), M)       # read_list's host side, on the restatement's arrays
            assert type(read).__name__ == "EccListRead" and read._fields == ("payload", "ok", "flips", "metric", "message", "rank", "n_ok")
            assert (read.payload, read.ok, read.flips, read.metric, read.rank, read.n_ok) == ([payload], [True], [6], [3 * (M - 12)], [1], [1])
            text = f"payload {payload.hex()} crc ok, corrected 6 of 256, list rank 1 of {L}"
            assert E.format_read_list(read, 0, M, L) == text == LR.format_read_list(d, 0, M, L)
    d = LR.decode_list(score, 1)
    assert d["rank"].tolist() == [0] and d["ok"].tolist() == [0] and d["n_ok"].tolist() == [0]
    assert LR.format_read_list(d, 0, M, 1) == f"payload {near_info[:13].tobytes().hex()} crc FAILED, corrected 4 of 256, list rank 0 of 1"


def test_the_read_s_text_and_its_parts(E):
    r = E.EccListRead([b"a", b"b", b"c"], [True, False, True], [3, 4, 5], [10, 20, 30], torch.zeros(3, 8, dtype=torch.uint8), [0, 0, 5], [1, 0, 3])
    one = r.image(2)
    assert (one.payload, one.ok, one.flips, one.metric, tuple(one.message.shape), one.rank, one.n_ok) == ([b"c"], [True], [5], [30], (1, 8), [5], [3])
    assert E.format_read_list(r, 0, 64, 8) == "payload 61 crc ok, corrected 3 of 64, list rank 0 of 8"
    assert E.format_read_list(r, 1, 64, 2) == "payload 62 crc FAILED, corrected 4 of 64, list rank 0 of 2"
    assert E.format_read_list(r, 2, 64, 8) == "payload 63 crc ok, corrected 5 of 64, list rank 5 of 8, 3 candidates pass"
    assert E.format_read_list(r, 0, 64, 8).startswith(E.format_read(r, 0, 64) + ", ")               # today's text, then the rank
    plain = E.EccRead([b"a"], [True], [3], [10], torch.zeros(1, 8, dtype=torch.uint8))
    assert E.format_any(plain, 0, 64, 1) == E.format_read(plain, 0, 64) and E.format_any(r, 2, 64, 8) == E.format_read_list(r, 2, 64, 8)
    for bad in (0, 3, 16, -2, True, 2.0, "4", None):
        with pytest.raises(ValueError, match="list size"):
            E.check_list_size(bad)
    assert [E.check_list_size(L) for L in (1, 2, 4, 8, np.int64(8))] == [1, 2, 4, 8, 8] and E.LIST_SIZES == (1, 2, 4, 8)


# ------------------------------------------------------------------------------------------------ refusals
def test_the_wrappers_refuse_before_any_launch(E):
    from gswm_amd import codec
    z = lambda *shape, dtype=torch.int32: torch.zeros(shape, dtype=dtype)
    for L in (0, 3, 16, True, None):
        with pytest.raises(ValueError, match="list_size"):
            codec.viterbi_list_decode(z(2, 256), L)
        with pytest.raises(ValueError, match="list size"):
            E.read_list(z(2, 256), L)
    for M in (48, 72):
        with pytest.raises(ValueError, match="multiple of 16"):
            codec.viterbi_list_decode(z(2, M), 2)
    for M, L in ((3952, 8), (7072, 4), (11616, 2), (17120, 1)):
        with pytest.raises(ValueError, match="LDS"):
            codec.viterbi_list_decode(z(1, M), L)
    for bad in (z(2, 256, dtype=torch.int64), z(256), z(0, 256)):
        with pytest.raises(ValueError):
            codec.viterbi_list_decode(bad, 2)
    for M, L in ((256, 8), (3936, 8), (17104, 1)):                   # served: the one thing missing is a device
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            codec.viterbi_list_decode(z(2, M), L)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.read_list(z(2, 256), 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.read_any(z(2, 256), 1)                                     # list size 1 is `read`
    with pytest.raises(ValueError, match="8192"):
        E.read_list(z(1, 8208), 1)


def test_library_forms_refuse_by_name(E):
    from gswm_amd import detect as D
    ring = D.Keyring()
    z = torch.zeros(2, 4, 8, 8)
    for bad in (0, 3, 16, True):
        with pytest.raises(ValueError, match="list size"):
            D.detect_payloads(z, ring, 256, list_size=bad)
    with pytest.raises(ValueError, match="ecc"):
        D.detect_payloads(z, ring, 256, ecc=None, list_size=8)
    import inspect
    from gswm_amd import pipeline as P
    assert inspect.signature(D.detect_payloads).parameters["list_size"].default == 1
    assert inspect.signature(P.GaussianShadingPipeline.verify_records).parameters["ecc_list"].default == 1


def test_command_lines_parse_the_list_size_and_refuse_by_name(E, capsys):
    from gswm_amd import extract as X, detect as D
    base = ["--key_hex", "00" * 32, "--nonce_hex", "00" * 16, "--message_length", "256"]
    coded = E.encode(b"P" * 13, 256).hex()
    msg = ["--original_message_hex", coded]
    assert X.build_parser().parse_args(base + msg + ["--ecc", "conv"]).ecc_list == 1
    assert X.build_parser().parse_args(base + msg).ecc_list == 1
    for L in (1, 2, 4, 8):
        for vote in ([], ["--soft", "1"], ["--robust", "1"], ["--robust_soft", "7"], ["--window_soft", "7", "--l", "2"]):
            a = X.build_parser().parse_args(base + msg + ["--ecc", "conv", "--ecc_list", str(L)] + vote)
            assert a.ecc == "conv" and a.ecc_list == L
    assert X.build_parser().parse_args(base + msg + ["--ecc_list", "1"]).ecc is None         # the default, spelled out, needs no code
    for extra, names in ((msg + ["--ecc_list", "8"], ("--ecc_list", "--ecc conv")),
                         (msg + ["--ecc_list", "2", "--soft", "1"], ("--ecc_list", "--ecc conv")),
                         (msg + ["--ecc", "conv", "--ecc_list", "3"], ("--ecc_list",)),
                         (msg + ["--ecc", "conv", "--ecc_list", "16"], ("--ecc_list",)),
                         (msg + ["--ecc", "conv", "--ecc_list", "0"], ("--ecc_list",)),
                         (msg + ["--ecc", "conv", "--ecc_list", "8", "--align", "d4"], ("--ecc", "--align")),
                         (msg + ["--ecc", "conv", "--ecc_list", "8", "--align", "flips", "--align_shift", "1"], ("--ecc", "--align")),
                         (msg + ["--ecc", "conv", "--ecc_list", "8", "--gpus", "2"], ("--ecc", "--gpus"))):
        with pytest.raises(SystemExit):
            X.build_parser().parse_args(base + extra)
        err = capsys.readouterr().err
        assert all(n in err for n in names), (extra, err)
    # the library form
    with pytest.raises(ValueError, match="--ecc_list"):
        X._ecc_wanted(SimpleNamespace(ecc=None, ecc_list=4, message_length=256))
    with pytest.raises(ValueError, match="list size"):
        X._ecc_wanted(SimpleNamespace(ecc="conv", ecc_list=3, message_length=256))
    assert X._ecc_wanted(SimpleNamespace(ecc="conv", ecc_list=8, message_length=256)) == "conv"
    assert X._ecc_wanted(SimpleNamespace(ecc="conv", message_length=256)) == "conv" and X._ecc_wanted(SimpleNamespace(ecc=None, message_length=250)) is None
    # detect: the three statistics
    ring = ["--keyring", "k.tsv"]
    assert D.build_parser().parse_args(ring).ecc_list == 1 and D.build_parser().parse_args(ring + ["--ecc", "conv"]).ecc_list == 1
    for stat in ([], ["--reliability", "15"], ["--window_reliability", "7", "--l", "2"]):
        a = D.build_parser().parse_args(ring + ["--ecc", "conv", "--ecc_list", "8"] + stat)
        assert a.ecc_list == 8 and D.ecc_refusal(a) is None
    a = D.build_parser().parse_args(ring + ["--ecc_list", "4"])
    assert "--ecc_list" in D.ecc_refusal(a) and "--ecc conv" in D.ecc_refusal(a)
    with pytest.raises(SystemExit, match="--ecc_list"):
        D.main(ring + ["--ecc_list", "4"])
    assert D.ecc_refusal(D.build_parser().parse_args(ring + ["--ecc_list", "1"])) is None
    for bad in ("0", "3", "16"):
        with pytest.raises(SystemExit):
            D.build_parser().parse_args(ring + ["--ecc", "conv", "--ecc_list", bad])
        assert "--ecc_list" in capsys.readouterr().err
    for extra, flag in ((["--align", "d4"], "--align"), (["--align_shift", "1"], "--align_shift"), (["--align_reliability", "7"], "--align_reliability")):
        a = D.build_parser().parse_args(ring + ["--ecc", "conv", "--ecc_list", "8"] + extra)
        assert "--ecc" in D.ecc_refusal(a) and flag in D.ecc_refusal(a)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbol_is_exported_and_prototyped():
    import ctypes
    from gswm_amd import _native as N
    lib = N.lib()
    assert "gsw_viterbi_list_decode" in N.exported_symbols() and hasattr(lib, "gsw_viterbi_list_decode")
    fn = lib.gsw_viterbi_list_decode
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 13 and fn.argtypes[4] is ctypes.c_int
    assert len(lib.gsw_viterbi_decode.argtypes) == 10                # the plain read's symbol is as it was
    hdr = open(os.path.join(ROOT, "include", "gswm.h")).read()
    assert ("int gsw_viterbi_list_decode(const int32_t* score_dev, int64_t score_stride, int B, int message_bits, int list_size,\n"
            "                            uint8_t* info_dev, uint8_t* message_dev, int32_t* metric_dev, int32_t* flips_dev,\n"
            "                            int32_t* ok_dev, int32_t* rank_dev, int32_t* n_ok_dev, void* stream);") in hdr
    import __graft_entry__ as G
    assert {"gswm_viterbi_list.inc", "gswm_viterbi_list_plan.h"} <= set(G.HEADERS)
    csrc = os.path.join(ROOT, "a-watermark-for-diffusion-models_amd", "csrc")
    rule = open(os.path.join(csrc, "Makefile")).read().split("\n\t")[0]
    assert "gswm_viterbi_list.inc" in rule and "gswm_viterbi_list_plan.h" in rule
    src = open(os.path.join(csrc, "gswm_kernels.hip")).read()
    assert src.index('#include "gswm_viterbi.inc"') < src.index('#include "gswm_viterbi_list_plan.h"') < src.index('#include "gswm_viterbi_list.inc"')
    assert "gsw_viterbi_list_decode" in open(os.path.join(csrc, "gswm.map")).read()


# ------------------------------------------------------------------------------------------------ the walk
def test_the_list_walk_fixes_the_end_to_end_noise():
    """The recorded sigma is the LARGEST grid point at which all 20 payloads read back at L = 8 and fewer than 20 at L = 1; the committed table is what the
    tool writes.  Conditions on the chosen inputs (not tolerances): at every grid point and every L no image has ok on a wrong payload, and none of the 64
    blank latents has ok at L = 8 (nor at any smaller L)."""
    walks = LR.walk_lists()
    print(walks)
    assert sorted(walks) == [1, 2, 4, 8]
    for L, (table, blank_ok) in walks.items():
        assert [s for s, _, _ in table] == R.WALK["sigmas"]
        assert all(wrong == 0 for _, _, wrong in table), (L, table)
        assert blank_ok == 0, L
    assert [r for _, r, _ in walks[1][0]] == [20, 20, 20, 20, 20, 20, 20, 20, 20, 16, 10, 6, 2, 0, 0]       # L = 1 is the walk of section 4.29
    assert all(a <= b for L, K in ((1, 2), (2, 4), (4, 8)) for (_, a, _), (_, b, _) in zip(walks[L][0], walks[K][0]))   # a longer list never reads fewer
    assert LR.chosen_sigma(walks) == LR.LIST_WALK["sigma"] == 2.75
    at = {L: next(r for s, r, _ in walks[L][0] if s == LR.LIST_WALK["sigma"]) for L in walks}
    assert at == LR.LIST_WALK["reads"] and at[8] == R.WALK["images"] == 20 and at[1] < 20
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import ecc_list_sigma_walk as W
    finally:
        sys.path.pop(0)
    assert open(os.path.join(ROOT, "profiles", "ecc_list_sigma_walk.txt")).read() == W.report(walks)
