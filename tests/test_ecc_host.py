"""CPU (no GPU): error-corrected payloads before any device is asked -- the code's known answers, the restatement of tests/ecc_reference.py against the
package's host encoder, what the decoder corrects, the refusals of the library, the wrappers and the command lines, the C prototype, and the sigma walk that
fixes the noise level of the end-to-end tests.

The walk (tools/ecc_sigma_walk.py, profiles/ecc_sigma_walk.txt; 4 x 32 x 32 latents, M = 256, 15 uniform levels, 20 images per point, seed 20260429):

    sigma   0.50 0.75 1.00 1.25 1.50 1.75 2.00 2.25 2.50 2.75 3.00 3.25 3.50 3.75 4.00
    coded     20   20   20   20   20   20   20   20   20   16   10    6    2    0    0
    uncoded   20   20   20   19   17   11    6    1    1    0    0    0    0    0    0

Recorded sigma: 2.50, the largest point at which all 20 coded payloads read back with ok; the uncoded alternative reads 1 of 20 there."""
import itertools
import math
import os

import numpy as np
import pytest
import torch

import ecc_reference as R
from conftest import ROOT

SIGMA = R.WALK["sigma"]
assert SIGMA == 2.5


@pytest.fixture(scope="module")
def E():
    import gswm_amd  # noqa: F401
    from gswm_amd import ecc
    return ecc


# ------------------------------------------------------------------------------------------------ known answers
def test_encoder_impulse_response_is_the_generators():
    out = R.conv_encode([1, 0, 0, 0, 0, 0, 0]).reshape(-1, 2)
    assert out[:, 0].tolist() == [1, 1, 1, 1, 0, 0, 1] and out[:, 1].tolist() == [1, 0, 1, 1, 0, 1, 1]
    assert [(R.G0 >> (6 - k)) & 1 for k in range(7)] == out[:, 0].tolist() and [(R.G1 >> (6 - k)) & 1 for k in range(7)] == out[:, 1].tolist()


def test_crc_known_answer(E):
    assert R.crc16(b"123456789") == 0x29B1 == E.crc16(b"123456789")
    assert R.crc16(b"") == 0xFFFF == E.crc16(b"")


def test_capacity_table(E):
    for M, want in ((64, 1), (256, 13), (2048, 125), (80, 2), (8192, 509)):
        assert R.capacity(M) == want == E.capacity(M)
        I, T, pb = R.sizes(M)
        assert (I, T) == (M // 2 - 6, M // 2) and I - 16 - 8 * pb == 2 and E.info_bits(M) == I     # 16 CRC bits and 2 pad bits, at every M


def test_the_interleaver_is_a_permutation_for_every_length(E):
    assert R.interleaver_step(256) == 17 == E.interleaver_step(256)
    for M in range(64, 8192 + 1, 16):
        S = R.interleaver_step(M)
        assert S % 2 == 1 and S >= (math.isqrt(M) | 1) and math.gcd(S, M) == 1
        assert all(math.gcd(s, M) != 1 for s in range(math.isqrt(M) | 1, S, 2))                  # the smallest such
        pos = R.positions(M)
        assert np.array_equal(np.sort(pos), np.arange(M)), M
    for M in (64, 80, 272, 720, 8192):
        assert E.interleaver_step(M) == R.interleaver_step(M)


# ------------------------------------------------------------------------------------------------ encoder and decoder
@pytest.mark.parametrize("M", [64, 80, 256, 2048])
def test_round_trip_of_random_payloads(E, M):
    rng = np.random.default_rng(M)
    pb = R.capacity(M)
    pls = [rng.bytes(pb) for _ in range(5)]
    msgs = [R.encode(p, M) for p in pls]
    assert [E.encode(p, M) for p in pls] == msgs and all(len(m) == M // 8 for m in msgs)       # the package's host encoder is the restatement's
    for mag in (1, 7):
        d = R.decode(np.stack([R.score_of(m, mag) for m in msgs]))
        assert R.payloads(d["info"], M) == pls and d["ok"].tolist() == [1] * 5 and d["flips"].tolist() == [0] * 5
        assert d["metric"].tolist() == [mag * M] * 5
        assert [row.tobytes() for row in d["message"]] == msgs
        assert not (d["info"][:, -1]).any()                                                     # pad bits and the tail


def test_four_flipped_positions_are_corrected():
    """free distance 10: any 4 errors on unit scores lie strictly closer to the sent codeword than to any other, so no tie decides"""
    M = 256
    rng = np.random.default_rng(4)
    payload = rng.bytes(R.capacity(M))
    msg = R.encode(payload, M)
    base = R.score_of(msg)
    patterns = [rng.choice(M, 4, replace=False) for _ in range(300)]
    patterns += [np.array(c) for c in itertools.islice(itertools.combinations(range(0, M, 17), 4), 60)]      # neighbours in the code sequence
    patterns += [np.arange(s, s + 4) for s in range(0, M - 4, 9)]                                          # adjacent message positions
    score = np.stack([base] * len(patterns))
    for i, p in enumerate(patterns):
        score[i, p] *= -1
    d = R.decode(score)
    assert d["flips"].tolist() == [4] * len(patterns) and d["ok"].all()
    assert all(row.tobytes() == msg for row in d["message"]) and R.payloads(d["info"], M) == [payload] * len(patterns)
    assert d["metric"].tolist() == [M - 8] * len(patterns)


def test_all_zero_scores_decode_to_the_zero_word():
    """every metric ties at every step: the lower predecessor wins, which is the all-zero path"""
    for M in (64, 256):
        d = R.decode(np.zeros((2, M), dtype=np.int32))
        assert not d["info"].any() and not d["message"].any() and d["metric"].tolist() == [0, 0] and d["flips"].tolist() == [0, 0]
        assert d["ok"].tolist() == [0, 0]                                                       # CRC of zero bytes is not zero


def test_ok_is_zero_when_a_payload_bit_is_altered():
    M = 256
    payload = np.random.default_rng(5).bytes(R.capacity(M))
    info = R.info_word(payload, M)
    for bit in (0, 37, 8 * R.capacity(M) - 1, 8 * R.capacity(M) + 3, R.sizes(M)[0] - 1):        # payload bits, a CRC bit, a pad bit
        bad = info.copy()
        bad[bit] ^= 1
        d = R.decode(R.score_of(np.packbits(R.encode_bits(bad, M)).tobytes())[None, :])
        assert d["ok"].tolist() == [0] and d["flips"].tolist() == [0], bit
        assert np.array_equal(np.unpackbits(d["info"][0])[:info.size], bad)


def test_the_interleaver_is_what_reads_through_an_erased_stripe():
    """24 adjacent message positions zeroed: without the interleaver that is a burst of 12 trellis steps, which free distance 10 does not bridge"""
    M = 256
    rng = np.random.default_rng(6)
    lost_plain = 0
    for _ in range(8):
        payload = rng.bytes(R.capacity(M))
        for start in range(0, M - 24, 29):
            for il in (True, False):
                sc = R.score_of(R.encode(payload, M, interleave=il))
                sc[start:start + 24] = 0
                d = R.decode(sc[None, :], interleave=il)
                good = R.payloads(d["info"], M) == [payload] and bool(d["ok"][0])
                assert good or not il
                lost_plain += (not good)
    assert lost_plain > 0


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("M", [0, 48, 63, 72, 250, 8200, 8208, 16384, -256, 256.0, True, None])
def test_lengths_outside_the_domain_are_refused(E, M):
    for f in (E.capacity, E.check_length, E.interleaver_step, R.check_length):
        with pytest.raises((ValueError, TypeError)):
            f(M)
    with pytest.raises((ValueError, TypeError)):
        E.encode(b"x", M)


def test_a_payload_of_the_wrong_length_is_refused(E):
    for pl in (b"", b"x" * 12, b"x" * 14, "thirteen bytes", None):
        with pytest.raises(ValueError):
            E.encode(pl, 256)
    with pytest.raises(ValueError):
        R.encode(b"x" * 12, 256)
    assert len(E.encode(b"x" * 13, 256)) == 32
    assert E.pad_payload("ab", 256) == b"ab" + bytes(11) and E.pad_payload(b"x" * 20, 256) == b"x" * 13


def test_the_wrapper_refuses_before_any_launch(E):
    from gswm_amd import codec
    for M in (48, 72, 8208):
        with pytest.raises(ValueError, match="multiple of 16"):
            codec.viterbi_decode(torch.zeros(2, M, dtype=torch.int32))
    with pytest.raises(ValueError):
        codec.viterbi_decode(torch.zeros(2, 256, dtype=torch.int64))
    with pytest.raises(ValueError):
        codec.viterbi_decode(torch.zeros(256, dtype=torch.int32))
    with pytest.raises(ValueError):
        codec.viterbi_decode(torch.zeros(0, 256, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.viterbi_decode(torch.zeros(2, 256, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.read(torch.zeros(2, 256, dtype=torch.int32))


def test_issue_encodes_payloads_before_anything_else(E):
    from gswm_amd import issue as I, trace as T
    reqs = [I.Request("alice", b"A" * 13, bytes(32), bytes(16)), I.Request("bob", "bob's id", bytes(range(32)), bytes(16))]
    coded = I.encode_requests(reqs, 32, "conv")
    assert [r.message for r in coded] == [E.encode(b"A" * 13, 256), E.encode(b"bob's id" + bytes(5), 256)]
    assert [(r.user_id, r.key, r.nonce) for r in coded] == [(r.user_id, r.key, r.nonce) for r in reqs]
    assert I.encode_requests(reqs, 32, None) == reqs
    reg = T.KeyedRegistry(32)
    for bad in ([I.Request("carol", b"C" * 12)], [I.Request("carol", b"C" * 32)], [I.Request("carol", "a string of more than thirteen bytes")]):
        with pytest.raises(ValueError, match="payload"):
            I.issue_latents(bad, (4, 32, 32), registry=reg, ecc="conv")                        # raises before the registry changes or a device is touched
    assert len(reg) == 0
    with pytest.raises(ValueError, match="ecc"):
        I.encode_requests(reqs, 32, "hamming")
    with pytest.raises(ValueError, match="multiple of 16"):
        I.encode_requests(reqs, 6, "conv")                                                      # 48-bit messages carry no coded payload
    assert I.build_parser().parse_args(["--requests", "r", "--registry", "g", "--ecc", "conv"]).ecc == "conv"
    assert I.build_parser().parse_args(["--requests", "r", "--registry", "g"]).ecc is None


def test_command_lines_refuse_by_name(E, capsys):
    from gswm_amd import extract as X, detect as D
    base = ["--key_hex", "00" * 32, "--nonce_hex", "00" * 16, "--message_length", "256"]
    coded = E.encode(b"P" * 13, 256).hex()
    a = X.build_parser().parse_args(base + ["--original_message_hex", coded, "--ecc", "conv", "--soft", "1"])
    assert a.ecc == "conv" and a.original_message_hex == coded
    a = X.build_parser().parse_args(base + ["--original_payload_hex", (b"P" * 13).hex(), "--ecc", "conv"])
    assert a.original_message_hex == coded                                                      # the convenience encodes it first
    assert X.build_parser().parse_args(base + ["--original_message_hex", coded]).ecc is None
    for extra, names in ((["--original_message_hex", coded, "--ecc", "conv", "--align", "d4"], ("--ecc", "--align")),
                         (["--original_message_hex", coded, "--ecc", "conv", "--align", "flips", "--align_shift", "1"], ("--ecc", "--align")),
                         (["--original_message_hex", coded, "--ecc", "conv", "--gpus", "2"], ("--ecc", "--gpus")),
                         (["--original_payload_hex", "00" * 13], ("--original_payload_hex", "--ecc")),
                         (["--original_payload_hex", "00" * 13, "--original_message_hex", coded, "--ecc", "conv"], ("--original_payload_hex", "--original_message_hex")),
                         (["--original_payload_hex", "00" * 12, "--ecc", "conv"], ("--original_payload_hex", "12 bytes")),
                         (["--ecc", "conv"], ("--original_message_hex",)),
                         ([], ("--original_message_hex",)),
                         (["--original_message_hex", coded, "--ecc", "conv", "--message_length", "250"], ("multiple of 16",)),
                         (["--original_message_hex", coded, "--ecc", "hamming"], ("--ecc",))):
        with pytest.raises(SystemExit):
            X.build_parser().parse_args(base + extra)                                           # (a flag given twice: the last one counts)
        err = capsys.readouterr().err
        assert all(n in err for n in names), (extra, err)
    # the library form refuses the same combinations
    from types import SimpleNamespace
    for kw, name in ((dict(align="d4"), "--align"), (dict(align_shift=2), "--align_shift"), (dict(gpus=4), "--gpus")):
        with pytest.raises(ValueError, match=name):
            X._ecc_wanted(SimpleNamespace(ecc="conv", message_length=256, **kw))
    assert X._ecc_wanted(SimpleNamespace(ecc=None, message_length=250, align="d4")) is None
    # detect
    ring = ["--keyring", "k.tsv"]
    assert D.build_parser().parse_args(ring + ["--ecc", "conv", "--reliability", "15"]).ecc == "conv"
    assert D.build_parser().parse_args(ring).ecc is None and D.ecc_refusal(D.build_parser().parse_args(ring + ["--align", "d4"])) is None
    for extra, flag in ((["--align", "d4"], "--align"), (["--align_shift", "1"], "--align_shift"), (["--align", "d4", "--align_reliability", "7"], "--align"),
                        (["--align_reliability", "7"], "--align_reliability"), (["--align_window_reliability", "7"], "--align_window_reliability")):
        a = D.build_parser().parse_args(ring + ["--ecc", "conv"] + extra)
        assert "--ecc" in D.ecc_refusal(a) and flag in D.ecc_refusal(a)
        with pytest.raises(SystemExit, match="--ecc"):
            D.main(ring + ["--ecc", "conv"] + extra)
    with pytest.raises(ValueError, match="multiple of 16"):
        D.main(ring + ["--ecc", "conv", "--message_length", "72"])
    # trace: the registries hold coded messages and read them back unchanged, so --ecc is refused there -- next to --pool and --align by both names
    from gswm_amd import trace as T
    keyed = ["--registry", "r.tsv", "--per_record_keys"]
    assert T.build_parser().parse_args(keyed).ecc is None
    for extra, names in ((["--pool", "all"], ("--ecc", "--pool")), (["--align", "d4"], ("--ecc", "--align")), ([], ("--ecc", "extract --ecc conv"))):
        with pytest.raises(SystemExit):
            T.build_parser().parse_args(keyed + extra + ["--ecc", "conv"])
        err = capsys.readouterr().err
        assert all(n in err for n in names), (extra, err)


def test_library_forms_refuse_by_name(E):
    from gswm_amd import detect as D
    ring = D.Keyring()
    z = torch.zeros(2, 4, 8, 8)
    with pytest.raises(ValueError, match="ecc"):
        D.detect_payloads(z, ring, 256, ecc=None)
    with pytest.raises(ValueError, match="multiple of 16"):
        D.detect_payloads(z, ring, 72)
    with pytest.raises(ValueError, match="window_reliability"):
        D.detect_payloads(z, ring, 256, reliability=7, window_reliability=7)
    with pytest.raises(ValueError, match="reliability"):
        D.detect_payloads(z, ring, 256, reliability=7, l=2)
    with pytest.raises(ValueError, match="window_reliability"):
        D.detect_payloads(z, ring, 256, window_reliability=7, l=1)
    with pytest.raises(TypeError):
        D.detect_payloads(z, ring, 256, align=[(0, 0, 0)])                                      # alignments are not an argument of this step
    r = E.EccRead([b"a", b"b"], [True, False], [3, 4], [10, 20], torch.zeros(2, 8, dtype=torch.uint8))
    one = r.image(1)
    assert (one.payload, one.ok, one.flips, one.metric, tuple(one.message.shape)) == ([b"b"], [False], [4], [20], (1, 8))
    assert E.format_read(r, 0, 64) == "payload 61 crc ok, corrected 3 of 64" and E.format_read(r, 1, 64) == "payload 62 crc FAILED, corrected 4 of 64"


# ------------------------------------------------------------------------------------------------ the C ABI
def test_symbol_is_exported_and_prototyped():
    import ctypes
    from gswm_amd import _native as N
    lib = N.lib()
    assert "gsw_viterbi_decode" in N.exported_symbols() and hasattr(lib, "gsw_viterbi_decode")
    fn = lib.gsw_viterbi_decode
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 10
    hdr = open(os.path.join(ROOT, "include", "gswm.h")).read()
    assert ("int gsw_viterbi_decode(const int32_t* score_dev, int64_t score_stride, int B, int message_bits, uint8_t* info_dev, uint8_t* message_dev, "
            "int32_t* metric_dev,\n                       int32_t* flips_dev, int32_t* ok_dev, void* stream);") in hdr
    import __graft_entry__ as G
    assert {"gswm_viterbi.inc", "gswm_viterbi_plan.h"} <= set(G.HEADERS)
    csrc = os.path.join(ROOT, "a-watermark-for-diffusion-models_amd", "csrc")
    rule = open(os.path.join(csrc, "Makefile")).read().split("\n\t")[0]
    assert "gswm_viterbi.inc" in rule and "gswm_viterbi_plan.h" in rule
    src = open(os.path.join(csrc, "gswm_kernels.hip")).read()
    assert src.index('#include "gswm_codec_soft_l.inc"') < src.index('#include "gswm_viterbi_plan.h"') < src.index('#include "gswm_viterbi.inc"')
    assert "gsw_viterbi_decode" in open(os.path.join(csrc, "gswm.map")).read()


# ------------------------------------------------------------------------------------------------ the sigma walk
def test_the_sigma_walk_fixes_the_end_to_end_noise():
    """SIGMA is the LARGEST grid point at which all 20 coded payloads read back with ok, and the uncoded alternative reads at most half of its images there (a
    condition on the choice of input, not a tolerance); the committed table is what the tool writes; none of the 64 blank latents of the seed has ok set."""
    import sys
    table = R.walk()
    print(table)
    assert [s for s, _, _ in table] == [0.5 + 0.25 * i for i in range(15)]
    assert R.chosen_sigma(table) == SIGMA
    coded, uncoded = next((c, u) for s, c, u in table if s == SIGMA)
    assert coded == R.WALK["images"] == 20 and 2 * uncoded <= 20
    assert all(c == 20 for s, c, _ in table if s <= SIGMA) and all(c < 20 for s, c, _ in table if s > SIGMA)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import ecc_sigma_walk as W
    finally:
        sys.path.pop(0)
    assert open(os.path.join(ROOT, "profiles", "ecc_sigma_walk.txt")).read() == W.report(table)
    setup = R.walk_setup()
    import gs_oracle as O
    import soft_reference as SR
    z = setup["blank"]
    ks = np.frombuffer(O.chacha20_keystream(setup["keys"][0], setup["nonces"][0], z.shape[1] // 8), dtype=np.uint8)
    score = np.stack([SR.soft_vote(row, ks, R.uniform_thresholds32(row), 256)["score"] for row in z]).astype(np.int32)
    assert not R.decode(score)["ok"].any()
