"""Host: the soft-decision vote for multi-bit windows -- `soft.window_thresholds` against a float64 restatement, the
restatement (tests/soft_l_reference.py) against the oracle's l-bit sign vote, the new flags and refusals, the old refusals, the C-ABI rows."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import gs_oracle as O  # noqa: E402
import soft_l_reference as RL  # noqa: E402
from scipy.special import ndtr  # noqa: E402


# ------------------------------------------------------------------------------------------------ threshold tables
@pytest.mark.parametrize("l", [2, 4])
def test_window_thresholds_equal_the_float64_restatement(l):
    from gswm_amd import codec, soft
    rs = np.random.RandomState(l)
    z = rs.standard_normal((3, 4, 8, 8)) * np.array([0.05, 1.0, 3.0])[:, None, None, None]
    z[2, 0, 0, 0], z[2, 0, 0, 1] = np.nan, np.inf                                   # left out of the RMS, as `uniform_thresholds`
    for levels, clip in ((15, 2.5), (3, 1.0), (1, 2.5)):
        got = soft.window_thresholds(torch.from_numpy(z).float(), l, levels, clip)
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, l, levels) and got.is_contiguous()
        want = RL.window_thresholds(torch.from_numpy(z).float().double().reshape(3, -1).numpy(), l, levels, clip)
        # fp32 RMS over 256 elements, one fp32 product per entry: a few 2^-24 relative
        assert np.allclose(got.numpy(), want, rtol=1e-5, atol=0.0)
        assert torch.equal(got[:, 0], soft.uniform_thresholds(torch.from_numpy(z).float(), levels, clip))      # bit 0 is the l = 1 table
    # the gaps: w = 0 has one flip boundary, w > 0 the largest distance between neighbouring multiples of s
    T = codec.quant_thresholds(l)
    g = soft.window_gaps(l)
    assert g[0] == float("inf") and g[l - 1] == float(np.max(np.diff(T)))
    if l == 4:
        assert g[1] == float(max(T[7] - T[3], T[11] - T[7])) and g[2] == float(max(T[i + 2] - T[i] for i in range(1, 12, 2)))
    # the small image is capped by its own RMS, the large one by half the gap
    t = soft.window_thresholds(torch.from_numpy(z).float(), l, 15, 2.5).numpy()
    assert abs(t[0, l - 1, -1] / t[0, 0, -1] - 1) < 1e-6 and t[0, 0, -1] < (14.5 / 15) * g[l - 1] / 2 and abs(t[2, l - 1, -1] - (14.5 / 15) * g[l - 1] / 2) < 1e-6 < t[2, 0, -1] - t[2, l - 1, -1]
    with pytest.raises(ValueError, match="levels must be"):
        soft.window_thresholds(torch.zeros(1, 8), l, 16)
    with pytest.raises(ValueError, match="l must be one of"):
        soft.window_thresholds(torch.zeros(1, 8), 3)


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("l", [2, 4])
def test_restatement_with_one_level_at_zero_is_the_oracle_sign_vote(l):
    """levels = 1, thr = 0: every bit of a non-NaN element has level 1, score = 2 counts - copies of the l-bit vote, computed here straight from
    int(norm.cdf(z) * 2^l) and the oracle's ChaCha20"""
    rs = np.random.RandomState(10 + l)
    n, mb = 192, 3
    key, nonce = bytes(rs.randint(0, 256, 32, dtype=np.uint8)), bytes(rs.randint(0, 256, 16, dtype=np.uint8))
    Z = rs.standard_normal(n) * 1.3
    T = RL.boundaries(l)[1:-1]
    Z[:T.size] = T                                                              # on every boundary ...
    Z[T.size:2 * T.size] = np.nextafter(T, -np.inf)                             # ... and just below it
    ks = np.frombuffer(O.chacha20_keystream(key, nonce, n * l // 8), dtype=np.uint8)
    y = np.floor(ndtr(Z) * (1 << l)).astype(np.int64)                           # the oracle's quantiser, l bits
    assert np.array_equal(y, RL.windows(Z, l)[0])
    ybits = ((y[:, None] >> np.arange(l - 1, -1, -1)[None, :]) & 1).reshape(-1)
    p = ybits ^ np.unpackbits(ks).astype(np.int64)
    M = 8 * mb
    counts, copies = p.reshape(-1, M).sum(axis=0), n * l // M
    r = RL.soft_vote(Z, ks, np.zeros((l, 1), dtype=np.float32), M, l)
    assert np.array_equal(r["score"], 2 * counts - copies) and np.array_equal(r["wsum"], np.full(M, copies)) and r["wsq"] == n * l
    assert np.array_equal(r["bits"], np.packbits((2 * counts > copies).astype(np.uint8))) and r["flags"] == 0
    assert np.array_equal(RL.hard_counts(Z, ks, M, l), counts)


def test_restatement_levels_on_hand_worked_values():
    """l = 2, thresholds T = (-0.674, ~0, 0.674): bit 0 flips at T_2 only, bit 1 at T_1, T_2 and T_3"""
    T = RL.boundaries(2)
    thr = np.array([[0.0, 0.25, 0.5], [0.0, 0.25, 0.5]], dtype=np.float32)
    Z = np.array([0.3, -0.3, 1.5, -1.5, T[1] + 0.25, T[3] - 0.25, np.nan, np.inf, -np.inf, 0.0, T[2]])
    y, flags = RL.windows(Z, 2)
    assert y.tolist() == [2, 1, 3, 0, 1, 2, 0, 3, 0, 2, 2] and flags == (RL.FLAG_SATURATED | RL.FLAG_NAN)
    lv = RL.levels_of(Z, y, thr, 2)
    # bit 0: distance from the median; bit 1: distance from the nearer of its neighbours (0.3: the median 0.3 below, T_3 0.37 above)
    assert lv[0].tolist() == [2, 2] and lv[1].tolist() == [2, 2]
    assert lv[2].tolist() == [3, 3] and lv[3].tolist() == [3, 3]                   # in the tails: far from everything
    assert lv[4].tolist() == [2, 2] and lv[5].tolist() == [2, 2]                   # exactly T_1 + 0.25 and T_3 - 0.25: the middle level counts
    assert lv[6].tolist() == [0, 0]                                                # NaN
    assert lv[7].tolist() == [3, 3] and lv[8].tolist() == [3, 3]                   # +-inf: every finite threshold
    assert lv[9].tolist() == [1, 1] and lv[10].tolist() == [1, 1]                  # at the median: both bits flip just below
    odd = np.array([[0.5, np.nan, -1.0, 0.25], [0.25, 0.25, np.nan, 0.0]], dtype=np.float32)    # unsorted, repeated, negative, NaN
    lv = RL.levels_of(Z, y, odd, 2)
    assert lv[0].tolist() == [2, 3] and lv[6].tolist() == [0, 0] and lv[7].tolist() == [3, 3] and lv[9].tolist() == [1, 1]


# ------------------------------------------------------------------------------------------------ ABI
def test_symbols_are_exported_and_prototyped():
    from gswm_amd import _native as N
    lib = N.lib()
    hdr = open(os.path.join(ROOT, "include", "gswm.h")).read()
    for name, nargs in (("gsw_extract_soft_l", 18), ("gsw_level_pack_l", 14)):
        assert name in N.exported_symbols()
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs
        assert fn.argtypes[-3] is ctypes.c_int and fn.argtypes[-2] is ctypes.c_int64 and fn.argtypes[-1] is ctypes.c_void_p
        assert f"int {name}(" in hdr
    assert lib.gsw_extract_soft_l.argtypes[6] is ctypes.c_int64 and lib.gsw_extract_soft_l.argtypes[8] is ctypes.c_int
    assert lib.gsw_level_pack_l.argtypes[3] is ctypes.c_int64 and lib.gsw_level_pack_l.argtypes[5] is ctypes.c_int
    assert lib.gsw_version() == 500
    # refusals that need no device: they happen before any launch
    assert lib.gsw_extract_soft_l(None, 0, None, 64, 1, None, 0, 1, 2, None, None, None, None, None, None, 1, 8, None) == N.GSW_ERR_BAD_ARG
    assert lib.gsw_level_pack_l(None, 0, None, 0, 1, 2, None, None, None, None, None, 1, 8, None) == N.GSW_ERR_BAD_ARG


# ------------------------------------------------------------------------------------------------ wrappers
def test_python_wrappers_refuse_before_any_launch():
    from gswm_amd import codec, detect, pipeline, soft, trace
    z = torch.zeros(2, 4, 8, 8)
    rows = torch.zeros(2, 64, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP device"):
        codec.extract_soft_l(z, rows, 2, torch.zeros(2, 3), 2)
    with pytest.raises(RuntimeError, match="HIP device"):
        codec.level_pack_l(z, torch.zeros(2, 3), 2)
    with pytest.raises(ValueError, match="use `level_pack`"):
        codec.level_pack_l(z, torch.zeros(1, 3), 1)
    with pytest.raises(ValueError, match="l must be one of"):
        codec.level_pack_l(z, torch.zeros(3, 3), 3)
    with pytest.raises(ValueError, match="message_length"):
        soft.extract_soft_l(z, bytes(32), bytes(16), 12, 2)
    with pytest.raises(ValueError, match="32 bytes"):
        soft.extract_soft_l(z, bytes(31), bytes(16), 8, 4)
    with pytest.raises(ValueError, match="l must be one of"):
        soft.extract_soft_l(z, bytes(32), bytes(16), 8, 3)
    kreg = trace.KeyedRegistry(1)
    kreg.add("a", bytes(32), bytes(16), b"\x01")
    with pytest.raises(ValueError, match="trace_latents_keyed_soft"):
        trace.trace_latents_keyed_soft_l(z, kreg, 1)
    with pytest.raises(ValueError, match="l must be one of"):
        trace.trace_latents_keyed_soft_l(z, kreg, 3)
    ring = detect.Keyring()
    ring.add("k", bytes(32), bytes(16))
    with pytest.raises(ValueError, match="reliability="):
        detect.detect_latents_soft_l(z, ring, 8, 1)
    with pytest.raises(ValueError, match="levels"):
        detect.detect_latents_soft_l(z, ring, 8, 2, levels=0)
    with pytest.raises(ValueError, match="levels|reliability"):
        detect.detect_latents_soft_l(z, ring, 8, 2, levels=16)
    pipe = pipeline.GaussianShadingPipeline(lambda *a: None, bytes(32), bytes(16), b"\x00" * 32, l=1)
    with pytest.raises(ValueError, match="window_levels needs a pipeline with l = 2 or 4"):
        pipe.verify_records(z, rows, 2, window_levels=15)
    pipe = pipeline.GaussianShadingPipeline(lambda *a: None, bytes(32), bytes(16), b"\x00" * 32, l=2)
    with pytest.raises(ValueError, match="window_levels cannot be combined with soft=True|soft=True cannot be combined"):
        pipe.verify_records(z, rows, 2, soft=True, window_levels=15)
    with pytest.raises(ValueError, match="levels must be"):
        pipe.verify_records(z, rows, 2, window_levels=16)
    with pytest.raises(ValueError, match="soft=True cannot be combined with l = 2"):                   # the old refusal stands
        pipe.verify_records(z, rows, 2, soft=True)


def test_l1_delegates_to_extract_soft(monkeypatch):
    from gswm_amd import soft
    seen = []
    monkeypatch.setattr(soft, "extract_soft", lambda *a, **k: seen.append((a, k)) or "vote")
    assert soft.extract_soft_l("z", b"k", b"n", 16, 1, levels=3, clip=2.0) == "vote"
    assert seen == [(("z", b"k", b"n", 16), {"levels": 3, "clip": 2.0, "thresholds": None})]


# ------------------------------------------------------------------------------------------------ command lines
def test_extract_cli_carries_window_soft_and_refuses_the_named_combinations(capsys, monkeypatch):
    from gswm_amd import codec, extract, soft
    base = ["--key_hex", "00" * 32, "--nonce_hex", "00" * 16, "--original_message_hex", "00"]
    assert extract.build_parser().parse_args(base).window_soft == 0
    a = extract.build_parser().parse_args(base + ["--window_soft", "15", "--l", "4"])
    assert (a.window_soft, a.l) == (15, 4)
    act = [x for x in extract.build_parser()._actions if "--window_soft" in x.option_strings]
    assert len(act) == 1 and "(not a reference flag)" in act[0].help
    for extra, name in ((["--window_soft", "3", "--l", "2", "--soft", "1"], "--soft 1"), (["--window_soft", "3", "--l", "2", "--robust", "1"], "--robust 1"),
                        (["--window_soft", "3", "--l", "2", "--align", "flips"], "--align"), (["--window_soft", "3"], "--l 2"),
                        (["--window_soft", "16", "--l", "2"], "--window_soft")):
        with pytest.raises(SystemExit):
            extract.build_parser().parse_args(base + extra)
        assert name in capsys.readouterr().err
    # the old refusals stand
    for extra, name in ((["--soft", "1", "--l", "2"], "--l 2"), (["--soft", "1", "--l", "4"], "--l 4"), (["--soft", "1", "--robust", "1"], "--robust 1")):
        with pytest.raises(SystemExit):
            extract.build_parser().parse_args(base + extra)
        assert name in capsys.readouterr().err
    # a namespace built by hand meets the same refusals, before anything touches a device
    z = torch.zeros(1, 4, 8, 8)
    ns = types.SimpleNamespace(key=bytes(32), nonce=bytes(16), l=2, message_length=8, window_soft=3, soft=1)
    with pytest.raises(ValueError, match="--window_soft cannot be combined with --soft 1"):
        extract.recover_exactracted_message_batch(z, ns)
    ns = types.SimpleNamespace(key=bytes(32), nonce=bytes(16), l=2, message_length=8, window_soft=3, robust=1)
    with pytest.raises(ValueError, match="--window_soft cannot be combined with --robust 1"):
        extract.recover_exactracted_message_batch(z, ns)
    ns = types.SimpleNamespace(key=bytes(32), nonce=bytes(16), l=2, message_length=8, window_soft=3, align="d4")
    with pytest.raises(ValueError, match="--window_soft cannot be combined with --align"):
        extract.recover_exactracted_message_batch(z, ns)
    ns = types.SimpleNamespace(key=bytes(32), nonce=bytes(16), l=1, message_length=8, window_soft=3)
    with pytest.raises(ValueError, match="--window_soft needs --l 2 or --l 4"):
        extract.recover_exactracted_message_batch(z, ns)
    ns = types.SimpleNamespace(key=bytes(32), nonce=bytes(16), l=2, message_length=8, soft=1)
    with pytest.raises(ValueError, match="--soft 1 cannot be combined with --l 2"):
        extract.recover_exactracted_message_batch(z, ns)
    # and the vote is routed to soft.extract_soft_l
    seen = []

    def fake(z, key, nonce, m, l, *, levels=15, clip=2.5, thresholds=None):
        seen.append((tuple(z.shape), m, l, levels, clip))
        B = z.shape[0]
        return codec.SoftVote(torch.zeros(B, m // 8, dtype=torch.uint8), torch.zeros(B, dtype=torch.int32), None, None, None, None)

    monkeypatch.setattr(soft, "extract_soft_l", fake)
    ns = types.SimpleNamespace(key=bytes(32), nonce=bytes(16), l=4, message_length=16, window_soft=3, soft_clip=2.0)
    assert extract.recover_exactracted_message_batch(torch.zeros(2, 4, 2, 2), ns) == ["0" * 16] * 2
    assert seen == [((2, 4, 2, 2), 16, 4, 3, 2.0)]


def test_trace_cli_carries_window_reliability_and_refuses_the_named_combinations(capsys):
    from gswm_amd import trace
    base = ["--registry", "r.tsv"]
    shared = base + ["--key_hex", "00" * 32, "--nonce_hex", "00" * 16]
    keyed = base + ["--per_record_keys"]
    assert trace.build_parser().parse_args(keyed).window_reliability is None
    a = trace.build_parser().parse_args(keyed + ["--window_reliability", "15", "--l", "2"])
    assert (a.window_reliability, a.l) == (15, 2) and trace._statistic_name(a) == "soft, 15 reliability levels per window bit"
    for extra, name in ((shared + ["--window_reliability", "3", "--l", "2"], "--per_record_keys"), (keyed + ["--window_reliability", "3"], "--l 2"),
                        (keyed + ["--window_reliability", "3", "--l", "4", "--hard"], "--hard"),
                        (keyed + ["--window_reliability", "3", "--l", "4", "--tamper_map", "d"], "--tamper_map"),
                        (keyed + ["--window_reliability", "0", "--l", "4"], "--window_reliability"),
                        (keyed + ["--window_reliability", "16", "--l", "4"], "--window_reliability")):
        with pytest.raises(SystemExit):
            trace.build_parser().parse_args(extra)
        assert name in capsys.readouterr().err
    # the old refusals stand
    for extra, name in ((shared + ["--reliability", "3", "--l", "2"], "--l 2"), (keyed + ["--keyed_reliability", "3", "--l", "4"], "--l 4")):
        with pytest.raises(SystemExit):
            trace.build_parser().parse_args(extra)
        assert name in capsys.readouterr().err
    key, nonce, z = bytes(32), bytes(16), torch.zeros(1, 4, 8, 8)
    reg = trace.Registry(1)
    reg.add("a", b"\x01")
    with pytest.raises(ValueError, match="reliability cannot be combined with l = 2"):
        trace.trace_latents(z, key, nonce, reg, l=2, reliability=3)


def test_detect_cli_carries_window_reliability_and_refuses_the_named_combinations():
    from gswm_amd import detect
    base = ["--keyring", "does-not-exist.tsv"]
    assert detect.build_parser().parse_args(base).window_reliability == 0
    a = detect.build_parser().parse_args(base + ["--window_reliability", "7", "--l", "4"])
    assert (a.window_reliability, a.l) == (7, 4)
    for extra in (["--window_reliability", "3"], ["--window_reliability", "3", "--l", "2", "--align", "flips"],
                  ["--window_reliability", "3", "--l", "2", "--reliability", "3"],
                  ["--window_reliability", "3", "--l", "2", "--align", "d4", "--align_reliability", "3"]):
        with pytest.raises(SystemExit) as e:
            detect.main(base + extra)
        assert "--window_reliability" in str(e.value) or "--reliability" in str(e.value) or "--align_reliability" in str(e.value)
    with pytest.raises(SystemExit, match="--window_reliability needs --l 2 or --l 4"):
        detect.main(base + ["--window_reliability", "3"])
    with pytest.raises(SystemExit, match="--window_reliability needs"):
        detect.main(base + ["--window_reliability", "3", "--l", "2", "--align", "flips"])
    with pytest.raises(SystemExit):
        detect.build_parser().parse_args(base + ["--window_reliability", "16"])
    # the old refusals stand
    with pytest.raises(SystemExit, match="--reliability needs --l 1"):
        detect.main(base + ["--reliability", "3", "--l", "2"])
    with pytest.raises(SystemExit, match="--align_reliability needs"):
        detect.main(base + ["--align", "flips", "--align_reliability", "3", "--l", "2"])
    ring = detect.Keyring()
    ring.add("k", bytes(32), bytes(16))
    with pytest.raises(ValueError, match="reliability cannot be combined with l = 2"):
        detect.detect_latents(torch.zeros(1, 4, 8, 8), ring, 8, l=2, reliability=3)
