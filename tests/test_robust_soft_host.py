"""CPU (no GPU): the robust decode with reliability levels on its NumPy restatement, tests/robust_soft_reference.py -- the identities
with the two decoders it joins (tests/tamper_reference.py, tests/soft_reference.py), the decoder's claim on synthetic latents before any GPU is involved,
`tamper.soft_weights`, and every refusal of the new Python names and flags that is decided without a device."""
import math
import types

import numpy as np
import pytest
import torch

from conftest import README_KEY, README_NONCE

import gs_oracle as O
import robust_soft_reference as R
import soft_reference as SR
import tamper_reference as TR

KEY, NONCE = bytes.fromhex(README_KEY), bytes.fromhex(README_NONCE)
SHAPE, M = (4, 64, 64), 256
MSG = bytes(np.random.default_rng(5).integers(0, 256, M // 8, dtype=np.uint8))
MSG_BITS = np.unpackbits(np.frombuffer(MSG, dtype=np.uint8))


# ===================================================================================================================== identities
@pytest.mark.parametrize("shape,l,tile,msg_bits", [((4, 16, 24), 1, 8, 64), ((4, 16, 24), 2, 8, 64), ((2, 32, 32), 4, 16, 128)])
@pytest.mark.parametrize("iters", [0, 1, 2, 3])
def test_unit_levels_are_the_tile_weighted_decode(shape, l, tile, msg_bits, iters):
    rng = np.random.default_rng(100 * l + iters)
    nb = int(np.prod(shape)) * l
    msg = bytes(rng.integers(0, 256, msg_bits // 8, dtype=np.uint8))
    q = TR.codeword(msg, KEY, NONCE, nb) ^ (rng.random(nb) < 0.3).astype(np.uint8)
    q[: nb // 3] = rng.integers(0, 2, nb // 3)                           # a destroyed part: some weights fall to 0
    bits, score, wsum, agree = TR.robust(q, KEY, NONCE, msg_bits, shape, l, tile, iters)
    n_t = shape[0] * tile * tile * l
    for W in (0, 1):
        got = R.decode(q, KEY, NONCE, None, msg_bits, shape, l, tile, iters, W)
        assert np.array_equal(got["bits"], bits) and np.array_equal(got["score"], score) and np.array_equal(got["wsum"], wsum)
        assert np.array_equal(got["excess"] + n_t, 2 * agree) and bool((got["wsq"] == n_t).all())
    if iters == 0:
        assert bool((got["weights"] == 1).all())


@pytest.mark.parametrize("seed", [0, 1])
def test_no_iterations_are_the_soft_vote(seed):
    z = TR.synthetic_latents(MSG, KEY, NONCE, SHAPE, 1.5, seed, 1, 16).astype(np.float32).reshape(-1)
    thr = R.uniform_thresholds32(z)
    ks_bytes = np.frombuffer(O.chacha20_keystream(KEY, NONCE, z.size // 8), dtype=np.uint8)
    want = SR.soft_vote(z, ks_bytes, thr, M)
    lev = R.levels_of(z, thr)
    assert set(np.unique(lev)) == set(range(16))
    got = R.decode(R.sign_bits(z), KEY, NONCE, lev, M, SHAPE, 1, 8, 0, 0)
    assert np.array_equal(got["score"], want["score"]) and np.array_equal(got["wsum"], want["wsum"])
    assert np.array_equal(np.packbits(got["bits"]), want["bits"]) and int(got["wsq"].sum()) == want["wsq"]
    plain = R.decode(R.sign_bits(z), KEY, NONCE, lev, M, SHAPE, 1, 8, 0, 1)          # the only round at unit levels: the plain vote
    assert np.array_equal(plain["score"], TR.vote(R.sign_bits(z), O.keystream_bits(KEY, NONCE, z.size), np.ones((8, 8)), M, SHAPE, 1, 8)[1])


def test_planes_round_trip():
    lev = np.random.default_rng(0).integers(0, 16, 4096)
    assert np.array_equal(R.levels_from_planes(R.planes_from_levels(lev, 4)), lev)


def test_soft_weights_is_the_default_rule_at_unit_levels_and_the_exact_floor_root():
    from gswm_amd import tamper
    rng = np.random.default_rng(1)
    for n_t in (64, 256, 1000, 4096, 16384):
        agree = rng.integers(0, n_t + 1, (3, 4, 5))
        want = tamper.default_weights(agree, n_t).astype(np.int64)
        got = tamper.soft_weights(2 * agree - n_t, np.full(agree.shape, n_t))
        assert got.dtype == np.int32 and np.array_equal(got, want)
        got_t = tamper.soft_weights(torch.from_numpy(2 * agree - n_t), torch.full(agree.shape, n_t))
        assert got_t.dtype == torch.int32 and np.array_equal(got_t.numpy(), want)
    wsq = np.array([0, 1, 2, 3, 4, 8, 9, 15, 16, 24, 25, 15 * 15 * 16384 - 1, 15 * 15 * 16384, 15 * 15 * 16384 + 1, 2**31 - 1, 46340**2 - 1, 46340**2])
    top = np.full(wsq.shape, 2**31 - 1)
    want = top - np.array([math.isqrt(int(v)) for v in wsq])
    assert np.array_equal(tamper.soft_weights(top, wsq), want) and np.array_equal(tamper.soft_weights(torch.from_numpy(top), torch.from_numpy(wsq)).numpy(), want)
    assert np.array_equal(R.soft_weights(top, wsq), want)
    assert np.array_equal(tamper.soft_weights(np.array([-5, 3]), np.array([4, 16])), [0, 0])
    for bad in (np.array([-1]), np.array([2**31])):
        with pytest.raises(ValueError, match="wsq"):
            tamper.soft_weights(np.array([1]), bad)
        with pytest.raises(ValueError, match="wsq"):
            tamper.soft_weights(torch.tensor([1]), torch.from_numpy(bad))


# ===================================================================================================================== the decoder's claim
def _recovered(sigma, rows, seed, loud, decoders):
    """bits of 20 x 256 decoded correctly by each of `decoders` = {name: (with levels, iters, sign_rounds)} on 20 synthetic images"""
    z = TR.synthetic_latents(MSG, KEY, NONCE, SHAPE, sigma, seed, 20, rows).astype(np.float32)
    z[:, :, :rows, :] *= np.float32(loud)
    ks = np.asarray(O.keystream_bits(KEY, NONCE, z[0].size)).astype(np.uint8)
    got = dict.fromkeys(decoders, 0)
    for zi in z:
        p = R.sign_bits(zi) ^ ks
        lev = R.levels_of(zi, R.uniform_thresholds32(zi, 15, 2.5))
        for name, (with_levels, iters, W) in decoders.items():
            got[name] += int((R.decode_p(p, lev if with_levels else None, M, SHAPE, 1, 8, iters, W)["bits"] == MSG_BITS).sum())
    return got


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_levels_and_tiles_together_beat_either_alone_under_noise_and_a_large_edit(seed):
    """sigma 1.5, 56 of 64 rows replaced, sign_rounds = 0: at least 500 of 5120 bits more than the tile-weighted decode and than the soft vote
    (this restatement: 4686 / 4684 / 4708 against 3829 / 3777 / 3920 and 3802 / 3825 / 3865)"""
    got = _recovered(1.5, 56, seed, 1.0, {"robust": (False, 2, 0), "soft": (True, 0, 0), "both": (True, 2, 0)})
    print(seed, got)
    assert got["both"] >= got["robust"] + 500 and got["both"] >= got["soft"] + 500, got


def test_a_first_round_at_unit_levels_survives_a_loud_paste():
    """sigma 1.0, 48 rows replaced by noise at 3 x unit scale: the paste takes the top levels.  sign_rounds = 1 recovers at least as many bits as the
    tile-weighted decode over the three seeds together, and at least 300 more than sign_rounds = 0 (this restatement: 15255 against 15099 and 13523)"""
    tot = dict.fromkeys(("robust", "both0", "both1"), 0)
    for seed in (0, 1, 2):
        got = _recovered(1.0, 48, seed, 3.0, {"robust": (False, 2, 0), "both0": (True, 2, 0), "both1": (True, 2, 1)})
        print(seed, got)
        for k in tot:
            tot[k] += got[k]
    assert tot["both1"] >= tot["robust"] and tot["both1"] >= tot["both0"] + 300, tot


# ===================================================================================================================== refusals that need no GPU
def _cpu_operands(B=2, shape=(4, 16, 24), l=1, P=2):
    nbytes = int(np.prod(shape)) * l // 8
    return torch.zeros((B, nbytes), dtype=torch.uint8), torch.zeros((B, P, nbytes), dtype=torch.uint8), torch.zeros((B, 48), dtype=torch.uint8)


@pytest.mark.parametrize("kw,match", [({"iters": -1}, "iters"), ({"iters": 9}, "iters"), ({"iters": 1.0}, "iters"), ({"iters": True}, "iters"),
                                      ({"sign_rounds": 2}, "sign_rounds"), ({"sign_rounds": -1}, "sign_rounds"), ({"sign_rounds": False}, "sign_rounds"),
                                      ({"l": 3}, "l must be"), ({"tile": 4}, "tile must be"), ({"tile": True}, "tile must be")])
def test_decode_robust_checks_its_small_arguments_before_its_tensors(kw, match):
    from gswm_amd import codec
    signs, planes, keys = _cpu_operands()
    with pytest.raises(ValueError, match=match):
        codec.decode_robust(signs, planes, keys, 64, (4, 16, 24), **kw)


def test_decode_robust_has_no_cpu_fallback():
    from gswm_amd import codec
    signs, planes, keys = _cpu_operands()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.decode_robust(signs, planes, keys, 64, (4, 16, 24))
    with pytest.raises(ValueError, match="whole number of 8 x 8 tiles"):
        codec.decode_robust(signs, planes, keys, 64, (4, 12, 32))
    with pytest.raises(ValueError, match="msg_bits"):
        codec.decode_robust(signs, planes, keys, 60, (4, 16, 24))


def test_robust_lds_bytes_is_the_layout_of_the_plan():
    from gswm_amd import codec
    assert codec.robust_lds_bytes(16384, 0, 64, 256, False) == 2048 + 256 + 32
    assert codec.robust_lds_bytes(16384, 4, 64, 256, True) == 2048 + 4 * 2048 + 3 * 256 + 32
    assert codec.robust_lds_bytes(1536, 1, 6, 24, True) == 192 + 192 + 72 + 4           # a row of 192 bytes is three whole blocks; 3 message bytes pad to 4


@pytest.mark.parametrize("kw,exc,match", [({"levels": 16}, ValueError, "levels"), ({"levels": -1}, ValueError, "levels"), ({"levels": 2.0}, ValueError, "levels"),
                                          ({"iters": 9}, ValueError, "iters"), ({"sign_rounds": 2}, ValueError, "sign_rounds"), ({"l": 3}, ValueError, "l must be"),
                                          ({"levels": 0, "thresholds": torch.zeros(3)}, ValueError, "takes no thresholds"),
                                          ({"message_length": 100}, IndexError, "string index out of range")])
def test_extract_robust_soft_checks_its_arguments_before_the_device(kw, exc, match):
    from gswm_amd import tamper
    z = torch.zeros((1, 4, 16, 24))
    kw = dict({"message_length": 64}, **kw)
    with pytest.raises(exc, match=match):
        tamper.extract_robust_soft(z, KEY, NONCE, kw.pop("message_length"), **kw)


def test_extract_robust_soft_wants_a_lattice_and_a_key():
    from gswm_amd import tamper
    with pytest.raises(ValueError, match=r"\[B, C, h, w\]"):
        tamper.extract_robust_soft(torch.zeros((1, 1536)), KEY, NONCE, 64)
    with pytest.raises(ValueError, match="key must be 32 bytes"):
        tamper.extract_robust_soft(torch.zeros((1, 4, 16, 24)), KEY[:31], NONCE, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tamper.extract_robust_soft(torch.zeros((1, 4, 16, 24)), KEY, NONCE, 64, levels=0)


def _args(**kw):
    base = dict(key=KEY, nonce=NONCE, message_length=64, l=1, soft=0, robust=0, window_soft=0, align="none", tile=8, robust_soft=15)
    base.update(kw)
    return types.SimpleNamespace(**base)


@pytest.mark.parametrize("kw,match", [({"soft": 1}, "--robust_soft cannot be combined with --soft 1"), ({"robust": 1}, "--robust_soft cannot be combined with --robust 1"),
                                      ({"window_soft": 7, "l": 2}, "--robust_soft cannot be combined with --window_soft"),
                                      ({"align": "flips"}, "--robust_soft cannot be combined with --align"),
                                      ({"soft": 1, "robust": 1}, "--robust_soft cannot be combined with --soft 1"),          # in front of the existing checks
                                      ({"robust_soft": 16}, "levels in 1..15"), ({"robust_soft": -1}, "levels in 1..15"), ({"robust_soft": 2.5}, "levels in 1..15")])
def test_extract_refuses_robust_soft_next_to_the_other_decoders_by_name(kw, match):
    from gswm_amd import extract as E
    z = torch.zeros((1, 4, 16, 24))
    with pytest.raises(ValueError, match=match):
        E.recover_exactracted_message_batch(z, _args(**kw))
    with pytest.raises(ValueError, match=match):
        E.recover_exactracted_message(z.numpy(), _args(**kw), device="cpu")


def test_extract_without_robust_soft_keeps_its_refusals():
    from gswm_amd import extract as E
    with pytest.raises(ValueError, match="level weights and tile weights are separate votes"):
        E.recover_exactracted_message_batch(torch.zeros((1, 4, 16, 24)), _args(robust_soft=0, soft=1, robust=1))


CLI = ["--key_hex", README_KEY, "--nonce_hex", README_NONCE, "--original_message_hex", "00"]


@pytest.mark.parametrize("extra,match", [(["--soft", "1"], "--robust_soft cannot be combined with --soft 1"), (["--robust", "1"], "--robust_soft cannot be combined with --robust 1"),
                                         (["--window_soft", "7", "--l", "2"], "--robust_soft cannot be combined with --window_soft"),
                                         (["--align", "d4"], "--robust_soft cannot be combined with --align"),
                                         (["--soft", "1", "--robust", "1"], "--robust_soft cannot be combined with --soft 1")])
def test_the_parser_refuses_the_same_combinations(extra, match, capsys):
    from gswm_amd import extract as E
    with pytest.raises(SystemExit):
        E.build_parser().parse_args(CLI + ["--robust_soft", "15"] + extra)
    assert match in capsys.readouterr().err


@pytest.mark.parametrize("extra", [["--robust_soft", "0", "--iters", "2"], ["--robust_soft", "16"], ["--robust_soft", "15", "--iters", "9"],
                                   ["--robust_soft", "15", "--sign_rounds", "2"], ["--robust_soft", "15", "--tile", "4"]])
def test_the_parser_checks_the_ranges(extra, capsys):
    from gswm_amd import extract as E
    if extra[1] == "0":
        a = E.build_parser().parse_args(CLI + extra)
        assert a.robust_soft == 0 and a.iters == 2 and a.sign_rounds == 1
        return
    with pytest.raises(SystemExit):
        E.build_parser().parse_args(CLI + extra)
    assert "invalid choice" in capsys.readouterr().err


def test_the_parser_accepts_robust_soft_at_every_window():
    from gswm_amd import extract as E
    for l in ("1", "2", "4"):
        a = E.build_parser().parse_args(CLI + ["--robust_soft", "15", "--l", l, "--tile", "16", "--iters", "3", "--sign_rounds", "0"])
        assert (a.robust_soft, a.l, a.tile, a.iters, a.sign_rounds) == (15, int(l), 16, 3, 0)
    a = E.build_parser().parse_args(CLI + ["--soft", "1"])
    assert a.robust_soft == 0
    with pytest.raises(SystemExit):
        E.build_parser().parse_args(CLI + ["--soft", "1", "--robust", "1"])


def test_verify_records_refuses_robust_levels_next_to_the_other_votes():
    from gswm_amd.pipeline import GaussianShadingPipeline
    pipe = GaussianShadingPipeline(lambda *a, **k: None, KEY, NONCE, MSG, height=128, width=192, device="cpu", ctx_uncond=torch.zeros(1, 1, 1))
    x0, records = torch.zeros((1, 4, 16, 24)), torch.zeros((1, 80), dtype=torch.uint8)
    with pytest.raises(ValueError, match="robust_levels cannot be combined with soft=True"):
        pipe.verify_records(x0, records, 32, soft=True, robust_levels=15)
    with pytest.raises(ValueError, match="robust_levels cannot be combined with window_levels"):
        pipe.verify_records(x0, records, 32, window_levels=7, robust_levels=15)
    for kw, match in (({"robust_levels": 16}, "levels"), ({"robust_levels": 0}, "levels"), ({"robust_levels": 15, "iters": 9}, "iters"),
                      ({"robust_levels": 15, "sign_rounds": 2}, "sign_rounds"), ({"robust_levels": 15, "tile": 4}, "tile must be")):
        with pytest.raises(ValueError, match=match):
            pipe.verify_records(x0, records, 32, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pipe.verify_records(x0, records, 32, robust_levels=15)
