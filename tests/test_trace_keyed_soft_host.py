"""CPU (no GPU): the host side of the keyed registry search ranked by reliability-weighted margins -- the NumPy
restatement trace.keyed_soft_topk_host against the definition by brute force, its identities with the sign search and with the soft vote
under one shared key, ties and padding, the CLI surface, and the argument validation of the two C entry points and their wrappers."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import README_KEY, README_NONCE

import gs_oracle as O
import keyed_soft_reference as KR
import soft_reference as SR
from gswm_amd import _native as N, codec, trace as T

INT32_MIN = -2 ** 31
K1, N1 = bytes.fromhex(README_KEY), bytes.fromhex(README_NONCE)


def _table(rng, levels):
    """a strictly increasing float32 table inside the bulk of a standard normal"""
    return np.sort(rng.uniform(0.05, 2.2, levels)).astype(np.float32)


@pytest.mark.parametrize("n", [8, 256, 520])
@pytest.mark.parametrize("levels", [1, 3, 7, 15])
def test_restatement_equals_the_definition_by_brute_force(n, levels):
    rng = np.random.default_rng(1000 * n + levels)
    B, U, k = 4, 11, 8
    z = rng.standard_normal((B, n)).astype(np.float32)
    z[0] = 0.0                                                                # all level 0 (no threshold is <= 0): every score 0
    z[1] *= 10.0                                                              # nearly all at the top level
    thr = np.stack([_table(rng, levels) for _ in range(B)])
    rows = KR.level_rows(z, thr)
    assert rows["planes"].shape == (B, levels.bit_length(), n // 8) and int(rows["levels"].max()) <= levels
    cw = rng.integers(0, 256, (U, n // 8), dtype=np.uint8)
    cw[3] = rows["signs"][2]                                                  # a perfect match for image 2
    scores = KR.brute_scores(rows["signs"], rows["levels"], cw)
    assert scores[2, 3] == rows["wsum"][2] and (scores[0] == 0).all()
    want = KR.brute_topk(scores, k)
    got = T.keyed_soft_topk_host(rows["signs"], rows["planes"], rows["wsum"], cw, k)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    with pytest.raises(ValueError, match="wsum"):
        T.keyed_soft_topk_host(rows["signs"], rows["planes"], rows["wsum"] + 1, cw, k)
    with pytest.raises(ValueError):
        T.keyed_soft_topk_host(rows["signs"], rows["planes"][:, :, :-1] if n > 8 else rows["planes"][:1], rows["wsum"], cw, k)


@pytest.mark.parametrize("n", [8, 256, 520, 16384])
def test_one_level_at_threshold_zero_is_the_sign_search(n):
    rng = np.random.default_rng(n)
    B, U = 5, 70
    z = rng.standard_normal((B, n)).astype(np.float32)
    z[0, ::2] = 0.0
    z[0, 1::4] = -0.0                                                         # |+-0| >= 0: level 1 as well
    rows = KR.level_rows(z, SR.sign_thresholds())
    assert (rows["levels"] == 1).all() and rows["wsum"].tolist() == [n] * B
    cw = rng.integers(0, 256, (U, n // 8), dtype=np.uint8)
    for k in (1, 8):
        a = T.keyed_soft_topk_host(rows["signs"], rows["planes"], rows["wsum"], cw, k)
        b = T.keyed_topk_host(rows["signs"], cw, k)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("n,M,levels", [(256, 8, 3), (520, 40, 15), (16384, 256, 15), (4608, 64, 7)])
def test_shared_key_scores_are_the_soft_votes_scores(n, M, levels):
    """for records of one key: score[b, u] = sum_t (2 r_t - 1) score[t] of the soft vote (tests/soft_reference.py)"""
    rng = np.random.default_rng(n + M + levels)
    U, B = 30, 4
    msgs = rng.integers(0, 256, (U, M // 8), dtype=np.uint8)
    z = (rng.standard_normal((B, n)) * 1.3).astype(np.float32)
    thr = _table(rng, levels)
    ks = np.frombuffer(O.chacha20_keystream(K1, N1, n // 8), dtype=np.uint8)
    rows = KR.level_rows(z, thr)
    cw = np.stack([np.packbits(O.cipher_bits(msgs[u].tobytes(), K1, N1, n)) for u in range(U)])
    r = np.unpackbits(msgs, axis=1).astype(np.int64)
    total = np.stack([(2 * r - 1) @ SR.soft_vote(z[b], ks, thr, M)["score"] for b in range(B)])       # [B, U]
    want = KR.brute_topk(total, 8)
    got = T.keyed_soft_topk_host(rows["signs"], rows["planes"], rows["wsum"], cw, 8)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert [SR.soft_vote(z[b], ks, thr, M)["wsq"] for b in range(B)] == rows["wsq"].tolist()


def test_ties_go_to_the_lower_row_and_a_short_registry_pads():
    n = 64
    rng = np.random.default_rng(5)
    z = rng.standard_normal((1, n)).astype(np.float32)
    rows = KR.level_rows(z, np.array([0.1, 0.5, 1.0], dtype=np.float32))
    one = rows["signs"][0].copy()
    top = int(np.argmax(rows["levels"][0]))
    one[top >> 3] ^= 0x80 >> (top & 7)                                        # one differing bit, at an element of the highest level present
    other = rng.integers(0, 256, n // 8, dtype=np.uint8)
    cw = np.stack([other, one, one, ~rows["signs"][0], one])                  # rows 1, 2, 4: one codeword; row 3: the complement
    idx, score = T.keyed_soft_topk_host(rows["signs"], rows["planes"], rows["wsum"], cw, 8)
    W, lv = int(rows["wsum"][0]), int(rows["levels"][0, top])
    assert lv >= 1 and idx[0, :3].tolist() == [1, 2, 4] and score[0, :3].tolist() == [W - 2 * lv] * 3
    assert idx[0, 4] == 3 and score[0, 4] == -W
    assert idx[0, 5:].tolist() == [-1] * 3 and score[0, 5:].tolist() == [INT32_MIN] * 3


def test_the_chosen_seed_separates_the_two_statistics_on_the_cpu():
    """The experiment of test_gpu_trace_keyed_soft.py::test_what_it_buys on the restatement alone, so that the seed is known to satisfy the
    inequality before anything runs on a GPU: half-normal latents on the side of each owner's codeword (drawn here, not by the embed kernel),
    the same noise.  Seed 2024: the sign statistic attributes 32 of 40 images, the 15-level statistic 39, neither a wrong one."""
    from gswm_amd import soft as S
    recs, owners, cw, noise = KR.buys_setup()
    B, n, U = KR.BUYS["B"], cw.shape[1] * 8, KR.BUYS["U"]
    rng = np.random.default_rng(KR.BUYS["seed"] + 1)
    bits = np.unpackbits(cw[owners], axis=1).astype(np.float64)
    z = torch.from_numpy((2 * bits - 1) * np.abs(rng.standard_normal((B, n)))).half()
    zn = ((z.float() + KR.BUYS["sigma"] * noise) / (1.0 + KR.BUYS["sigma"] ** 2) ** 0.5).half()       # back to unit variance, as the GPU test does
    zw = SR.widen(zn)
    rows = KR.level_rows(zw, S.uniform_thresholds(zn, KR.BUYS["levels"], KR.BUYS["clip"]).numpy())
    si, ss = T.keyed_topk_host(rows["signs"], cw, 1)
    wi, ws = T.keyed_soft_topk_host(rows["signs"], rows["planes"], rows["wsum"], cw, 1)
    sign = KR.attributions(si[:, 0], [T.log10_p_any(T.log10_p_soft(int(ss[b, 0]), n), U) for b in range(B)], owners, KR.BUYS["fpr"])
    soft = KR.attributions(wi[:, 0], [T.log10_p_any(S.log10_p(int(ws[b, 0]), int(rows["wsq"][b])), U) for b in range(B)], owners, KR.BUYS["fpr"])
    print("sign statistic (right, wrong):", sign, " 15-level statistic:", soft)
    assert soft[0] > sign[0] and soft[1] == 0 and sign[1] == 0


# ------------------------------------------------------------------------------------------------------------ CLI
def test_cli_parser_keyed_reliability(capsys):
    P = T.build_parser
    keyed = ["--per_record_keys", "--registry", "info_data.txt"]
    shared = ["--registry", "r.tsv", "--key_hex", "00" * 32, "--nonce_hex", "00" * 16]
    a = P().parse_args(keyed + ["--keyed_reliability", "15", "--top", "3", "--fpr", "1e-9"])
    assert a.keyed_reliability == 15 and a.per_record_keys is True and a.reliability is None and (a.top, a.fpr) == (3, 1e-9)
    assert P().parse_args(keyed).keyed_reliability is None and P().parse_args(shared).keyed_reliability is None
    assert T._statistic_name(a) == "soft, 15 reliability levels" and T._statistic_name(P().parse_args(keyed)) == "soft"
    for extra, name in ((shared + ["--keyed_reliability", "3"], "--per_record_keys"), (keyed + ["--keyed_reliability", "3", "--hard"], "--hard"),
                        (keyed + ["--keyed_reliability", "3", "--l", "2"], "--l 2"), (keyed + ["--keyed_reliability", "3", "--l", "4"], "--l 4"),
                        (keyed + ["--keyed_reliability", "3", "--reliability", "3"], "--reliability"),
                        (keyed + ["--keyed_reliability", "0"], "--keyed_reliability"), (keyed + ["--keyed_reliability", "16"], "--keyed_reliability")):
        with pytest.raises(SystemExit):
            P().parse_args(extra)
        err = capsys.readouterr().err
        assert name in err and "--keyed_reliability" in err, (extra, err)


def test_the_pinned_refusals_still_raise_and_point_at_the_new_names(capsys):
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(["--registry", "r.tsv", "--per_record_keys", "--reliability", "3"])
    err = capsys.readouterr().err
    assert "--reliability cannot be combined with --per_record_keys" in err and "--keyed_reliability" in err
    kreg = T.KeyedRegistry(1)
    kreg.add("a", bytes(32), bytes(16), b"\x01")
    with pytest.raises(ValueError, match="reliability cannot be combined with trace_latents_keyed.*trace_latents_keyed_soft"):
        T.trace_latents_keyed(torch.zeros(1, 4, 8, 8), kreg, reliability=3)


# ------------------------------------------------------------------------------------------------------------ wrappers, C ABI
def test_wrappers_refuse_host_tensors_before_any_launch():
    z, thr = torch.zeros(2, 4, 8, 8), torch.zeros(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.level_pack(z, thr)
    rows = codec.LevelRows(torch.zeros(2, 32, dtype=torch.uint8), torch.zeros(2, 2, 32, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32),
                           torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.trace_keyed_soft_topk(rows, 256, torch.zeros(4, 80, dtype=torch.uint8), 32)
    kreg = T.KeyedRegistry(32)
    kreg.add("a", bytes(32), bytes(16), bytes(32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.trace_latents_keyed_soft(z, kreg, thresholds=thr)
    with pytest.raises(ValueError, match="fpr"):
        T.trace_latents_keyed_soft(z, kreg, fpr=0.0)
    with pytest.raises(IndexError):
        T.trace_latents_keyed_soft(torch.zeros(1, 4, 10, 10), kreg)           # 400 lattice bits, 256-bit messages
    assert [codec.level_planes(t) for t in (1, 2, 3, 4, 7, 8, 15)] == [1, 2, 2, 3, 3, 4, 4]
    for bad in (0, 16, True, 1.5):
        with pytest.raises(ValueError, match="levels"):
            codec.level_planes(bad)


def test_entry_points_validate_before_any_hip_call():
    lib, p = N.lib(), ctypes.c_void_p(16)
    BAD, UNS, RAG = N.GSW_ERR_BAD_ARG, N.GSW_ERR_UNSUPPORTED, N.GSW_ERR_RAGGED

    def pack(z=p, dt=N.GSW_F16, thr=p, ts=0, levels=15, signs=p, planes=p, wsum=p, wsq=p, flags=p, B=2, n=16384):
        return lib.gsw_level_pack(z, dt, thr, ts, levels, signs, planes, wsum, wsq, flags, B, n, None)

    for name in ("z", "thr", "signs", "planes", "wsum", "wsq", "flags"):
        assert pack(**{name: None}) == BAD, name
    assert pack(dt=4) == BAD and pack(dt=-1) == BAD and pack(B=0) == BAD and pack(B=-1) == BAD and pack(n=0) == BAD and pack(n=-8) == BAD
    assert pack(levels=0) == BAD and pack(levels=16) == BAD and pack(ts=14) == BAD and pack(ts=-1) == BAD
    assert pack(z=ctypes.c_void_p(8)) == BAD and pack(thr=ctypes.c_void_p(18)) == BAD
    assert pack(n=16383) == UNS and pack(n=4) == UNS and pack(n=2 ** 20 + 8) == UNS

    def call(signs=p, planes=p, wsum=p, levels=15, B=2, n=16384, rec=p, stride=80, mb=32, U=100, k=4, idx=p, score=p, ws=p):
        return lib.gsw_trace_keyed_soft_topk(signs, planes, wsum, levels, B, n, rec, stride, mb, U, k, idx, score, ws, None)

    for name in ("signs", "planes", "wsum", "rec", "idx", "score", "ws"):
        assert call(**{name: None}) == BAD, name
    assert call(B=0) == BAD and call(k=0) == BAD and call(k=9) == BAD and call(levels=0) == BAD and call(levels=16) == BAD
    assert call(mb=0) == BAD and call(mb=257, stride=320) == BAD and call(U=0) == BAD and call(U=2 ** 31) == BAD
    assert call(stride=79) == BAD and call(stride=64) == BAD and call(rec=ctypes.c_void_p(8)) == BAD and call(wsum=ctypes.c_void_p(18)) == BAD
    assert call(n=0) == BAD
    for n in (16384 + 8, 250, 16384 + 128):
        assert call(n=n) == RAG, n
    # the domain: n_bits (1 + P) <= 1 048 576, P the bit length of levels
    for levels, n_max in ((1, 524288), (2, 349440), (3, 349440), (4, 262144), (7, 262144), (8, 209664), (15, 209664)):
        assert call(levels=levels, n=n_max + 256) == UNS, (levels, n_max)
    assert call(levels=15, n=196608 + 256 * 52) == UNS and call(B=65536) == UNS
    assert lib.gsw_version() == 500
