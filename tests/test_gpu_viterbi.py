"""GPU: error-corrected payloads -- codec.viterbi_decode against the NumPy restatement of tests/ecc_reference.py on poisoned,
guard-banded buffers, then the read end to end: issue with ecc="conv", noise, extract_soft + ecc.read, detect.detect_payloads, verify_records and the extract
line.  EXACT equality of every output everywhere; no tolerance.

The end-to-end noise is the sigma tools/ecc_sigma_walk.py finds (profiles/ecc_sigma_walk.txt, asserted by tests/test_ecc_host.py): 2.50, the largest grid
point at which all 20 coded payloads read back with ok (20 / 16 / 10 of 20 at sigma 2.5 / 2.75 / 3.0), where the uncoded alternative reads 1 of 20."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ecc_reference as R
from poison import FINITE, NAN, Ledger, poisoned

pytestmark = pytest.mark.gpu

SIGMA = R.WALK["sigma"]
COPIES = 16                     # votes per message bit the random scores stand for: |score| <= 15 COPIES


@pytest.fixture(scope="module")
def G():
    import gswm_amd  # noqa: F401
    from gswm_amd import codec, detect, ecc, extract, issue, pipeline, soft, tamper, trace
    return SimpleNamespace(codec=codec, detect=detect, ecc=ecc, extract=extract, issue=issue, pipeline=pipeline, soft=soft, tamper=tamper, trace=trace)


# ------------------------------------------------------------------------------------------------ the kernel against the restatement
def _codewords(rng, B, M):
    return np.stack([R.score_of(R.encode(rng.bytes(R.capacity(M)), M)) for _ in range(B)])


def _scores(pattern, B, M):
    rng = np.random.default_rng(M * 1009 + B * 17 + sum(map(ord, pattern)))
    if pattern == "uniform":
        return rng.integers(-15 * COPIES, 15 * COPIES + 1, (B, M)).astype(np.int32)
    if pattern == "hard":
        return (2 * rng.integers(0, 2, (B, M)) - 1).astype(np.int32)
    if pattern == "ternary":                                        # ties at most steps
        return rng.integers(-1, 2, (B, M)).astype(np.int32)
    if pattern == "zeros":
        return np.zeros((B, M), dtype=np.int32)
    if pattern == "code1":
        return _codewords(rng, B, M)
    if pattern == "codebig":                                        # sum |score| just under 2^30
        return _codewords(rng, B, M) * ((2 ** 30 - 1) // M)
    assert pattern == "burst"                                       # 24 adjacent MESSAGE positions erased
    sc = _codewords(rng, B, M)
    for b in range(B):
        start = (b * 7) % (M - 24)
        sc[b, start:start + 24] = 0
    return sc


# (M, B, pad of the row stride, pattern): every value of each axis appears -- M in {64, 80, 256, 272, 2048, 8192} (+ 4096: the two-wave workgroup), B in
# {1, 3, 70, 257}, strides M and M + 16, the seven patterns; 1-, 2- and 4-wave workgroups, batches that fill the last workgroup and batches that do not
CASES = [(64, 1, 0, "uniform"), (64, 257, 16, "ternary"), (80, 3, 16, "hard"), (80, 70, 0, "codebig"), (256, 70, 16, "uniform"), (256, 257, 0, "burst"),
         (256, 3, 0, "zeros"), (272, 3, 0, "code1"), (272, 70, 16, "ternary"), (2048, 3, 16, "uniform"), (2048, 70, 0, "burst"), (2048, 1, 0, "codebig"),
         (4096, 3, 16, "uniform"), (4096, 1, 0, "ternary"), (8192, 1, 16, "uniform"), (8192, 3, 0, "hard"), (256, 2, 16, "code1")]
_WANT = {}


def _want(M, B, pattern):
    """the restatement of a case, computed once and shared by both poison patterns"""
    key = (M, B, pattern)
    if key not in _WANT:
        sc = _scores(pattern, B, M)
        sc.setflags(write=False)
        _WANT[key] = (sc, R.decode(sc))
    return _WANT[key]


def _assert_decode(got, want, where):
    assert (got.info.dtype, got.message.dtype, got.metric.dtype, got.flips.dtype, got.ok.dtype) == (torch.uint8, torch.uint8, torch.int32, torch.int32, torch.int32), where
    for name in ("info", "message", "metric", "flips", "ok"):
        g, w = getattr(got, name).cpu().numpy(), want[name]
        assert g.shape == w.shape, (where, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            rows = np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0]
            raise AssertionError(f"{where}: {name} differs in rows {rows[:8].tolist()} ({len(rows)} of {len(g)})")


@pytest.mark.parametrize("M,B,pad,pattern", CASES)
@pytest.mark.parametrize("poison", [NAN, FINITE])
def test_viterbi_decode_matches_the_restatement_on_poisoned_buffers(G, M, B, pad, pattern, poison):
    sc, want = _want(M, B, pattern)
    wide = np.full((B, M + pad), 2 ** 31 - 1, dtype=np.int32)       # what lies between the rows must not be read: it would break the bound at once
    wide[:, :M] = sc
    led = Ledger(poison)
    with poisoned(led):
        got = G.codec.viterbi_decode(led.wrap(torch.from_numpy(wide).cuda())[:, :M])
    led.check()
    _assert_decode(got, want, (M, B, pad, pattern))


def test_every_output_element_is_written(G):
    """all-zero votes decode to zeros everywhere (metric 0, flips 0, ok 0: the CRC of zero bytes is not zero), which no pattern byte equals"""
    for M, B in ((64, 1), (80, 70), (256, 3), (272, 257), (2048, 5), (4096, 3), (8192, 2)):
        for poison in (NAN, FINITE):
            led = Ledger(poison)
            with poisoned(led):
                got = G.codec.viterbi_decode(torch.zeros((B, M), dtype=torch.int32, device="cuda"))
            led.check()
            assert all(led.untouched(t) == 0 for t in got), [led.where(t) for t in got if led.untouched(t)]
            assert all(not bool(t.any()) for t in got), (M, B)
            assert tuple(got.info.shape) == (B, M // 16) and tuple(got.message.shape) == (B, M // 8) and all(tuple(t.shape) == (B,) for t in got[2:])


def test_the_interleaver_is_why_an_erased_stripe_reads():
    """the CPU side of the burst cases: the same payloads and stripes WITHOUT the interleaver lose at least one row, the shipped code reads every one"""
    M, B = 256, 257
    sc, want = _want(M, B, "burst")
    assert want["ok"].all() and (want["flips"] <= 24).all()         # (an erased position whose code bit is 1 counts as a flip: score > 0 is false there)
    rng = np.random.default_rng(M * 1009 + B * 17 + sum(map(ord, "burst")))
    payloads = [rng.bytes(R.capacity(M)) for _ in range(B)]
    assert R.payloads(want["info"], M) == payloads
    plain = np.stack([R.score_of(R.encode(p, M, interleave=False)) for p in payloads])
    for b in range(B):
        start = (b * 7) % (M - 24)
        plain[b, start:start + 24] = 0
    d = R.decode(plain, interleave=False)
    lost = [b for b in range(B) if R.payloads(d["info"], M)[b] != payloads[b] or not d["ok"][b]]
    assert lost, "the stripe never broke the un-interleaved code: the case shows nothing"


def test_the_wrapper_refuses_before_any_launch(G):
    z = lambda *shape, dtype=torch.int32: torch.zeros(shape, dtype=dtype, device="cuda")
    for M in (48, 72, 250, 8208):
        with pytest.raises(ValueError, match="multiple of 16"):
            G.codec.viterbi_decode(z(2, M))
    for bad in (z(2, 256, dtype=torch.int64), z(2, 256, dtype=torch.float32), z(256), z(2, 2, 256), z(0, 256), z(2, 512)[:, ::2], z(1, 256).expand(3, 256)):
        with pytest.raises(ValueError):
            G.codec.viterbi_decode(bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.codec.viterbi_decode(torch.zeros(2, 256, dtype=torch.int32))
    with pytest.raises(ValueError):
        G.codec.viterbi_decode(None)


# ------------------------------------------------------------------------------------------------ end to end at the recorded sigma
@pytest.fixture(scope="module")
def E2E(G):
    """20 latents of 4 x 32 x 32 issued with ecc="conv" under their own records (12 keys), noise of the recorded sigma added; the restatement's votes and decode"""
    s = R.walk_setup()
    B, M, shape = R.WALK["images"], R.WALK["M"], R.WALK["shape"]
    reg = G.trace.KeyedRegistry(M // 8)
    reqs = [G.issue.Request(f"user{b}", s["payloads"][b], s["keys"][b], s["nonces"][b]) for b in range(B)]
    np.random.seed(R.WALK["seed"])                                  # issue_latents(seed=None) draws NumPy's global MT19937 stream: the walk's uniforms
    z, rows = G.issue.issue_latents(reqs, shape, registry=reg, ecc="conv")
    coded = [R.encode(p, M) for p in s["payloads"]]
    held = R.held(z.cpu().numpy().reshape(B, -1), s["noise"], SIGMA)
    score, thr = R.walk_scores(s, held, M)
    return SimpleNamespace(s=s, B=B, M=M, reg=reg, rows=rows, z=z, coded=coded, held=held, held_dev=torch.from_numpy(held).cuda().view(B, *shape), score=score,
                           thr=thr, want=R.decode(score))


def _assert_read(read, want, where, M=256):
    assert read.payload == R.payloads(want["info"], M), where
    assert read.ok == [bool(v) for v in want["ok"]] and read.flips == want["flips"].tolist() and read.metric == want["metric"].tolist(), where
    assert np.array_equal(read.message.cpu().numpy(), want["message"]), where


def test_issue_registers_the_coded_message(G, E2E):
    e = E2E
    assert [e.reg.record(f"user{b}")[2] for b in range(e.B)] == e.coded                                     # trace reads them back unchanged
    assert e.rows[:, 48:48 + 32].cpu().numpy().tobytes() == b"".join(e.coded)
    bits, flags, matches = G.codec.extract_records(e.z, e.rows, 32)
    assert matches.cpu().tolist() == [256] * e.B and not bool(flags.any())
    u_z = R.walk_latents(e.s, e.coded)                                                                      # the walk's latents, by the oracle's embed
    assert float(np.abs(e.z.cpu().numpy().reshape(e.B, -1) - u_z).max()) <= 1e-5


def test_payloads_read_back_through_extract_soft_and_ecc_read(G, E2E):
    e = E2E
    vote = G.codec.extract_soft(e.held_dev, e.rows, 32, torch.from_numpy(e.thr).cuda())
    assert np.array_equal(vote.score.cpu().numpy(), e.score)
    read = G.ecc.read(vote.score)
    _assert_read(read, e.want, "extract_soft + ecc.read")
    assert read.payload == e.s["payloads"] and all(read.ok), [b for b in range(e.B) if read.payload[b] != e.s["payloads"][b]]
    assert read.message.cpu().numpy().tobytes() == b"".join(e.coded)
    hard = int((np.unpackbits(vote.bits.cpu().numpy(), axis=1) != np.unpackbits(read.message.cpu().numpy(), axis=1)).sum())
    assert hard == sum(read.flips) > 0                                                                      # the vote alone had wrong bits in it
    # the plain vote's 2 counts - copies is a score as well: the device decodes it as the restatement does
    bits, flags, counts = G.codec.extract_batch(e.held_dev[:1], e.s["keys"][0], e.s["nonces"][0], 256, return_counts=True)
    sc = G.ecc.score_from_counts(counts, 16)
    _assert_read(G.ecc.read(sc), R.decode(sc.cpu().numpy()), "2 counts - copies")


def test_detect_payloads_names_the_key_and_reads_the_payload(G, E2E):
    e = E2E
    ring = G.detect.Keyring()
    for i, (key, nonce) in enumerate(e.s["ring"]):
        ring.add(f"key{i}", key, nonce)
    plain = G.detect.detect_latents(e.held_dev, ring, 256, reliability=15)
    results, reads = G.detect.detect_payloads(e.held_dev, ring, 256, reliability=15)
    assert results == plain                                                                                  # the unchanged DetectResult
    assert [r.key_id for r in results] == [f"key{b % 12}" for b in range(e.B)]
    vote = G.codec.extract_soft(e.held_dev, e.rows, 32, G.soft.uniform_thresholds(e.held_dev, 15, 2.5))      # the read's own table, the image's own key
    want = R.decode(vote.score.cpu().numpy())
    for b in range(e.B):
        one = {k: v[b:b + 1] for k, v in want.items()}
        _assert_read(reads[b], one, f"detect_payloads image {b}")
        assert reads[b].payload == [e.s["payloads"][b]] and reads[b].ok == [True]
        assert results[b].message == vote.bits[b].cpu().numpy().tobytes()
    # the sign statistic: 2 counts - copies under the named key
    results, reads = G.detect.detect_payloads(e.held_dev, ring, 256)
    assert [r.key_id for r in results] == [f"key{b % 12}" for b in range(e.B)]
    _, _, _, counts = G.codec.extract_records(e.held_dev, e.rows, 32, return_counts=True)
    want = R.decode((2 * counts - 16).cpu().numpy())
    for b in range(e.B):
        _assert_read(reads[b], {k: v[b:b + 1] for k, v in want.items()}, f"detect_payloads (signs) image {b}")


def test_unwatermarked_latents_equal_the_restatement_and_none_is_ok(G, E2E):
    """a false ok has probability 2^-18 per image at M = 256 (16 CRC bits, 2 pad bits); none occurs under the committed seed (tests/test_ecc_host.py checks it on the CPU)"""
    e = E2E
    blank = e.s["blank"]
    import gs_oracle as O
    import soft_reference as SR
    thr = np.stack([R.uniform_thresholds32(row) for row in blank])
    ks = np.frombuffer(O.chacha20_keystream(e.s["keys"][0], e.s["nonces"][0], blank.shape[1] // 8), dtype=np.uint8)
    score = np.stack([SR.soft_vote(blank[b], ks, thr[b], 256)["score"] for b in range(64)]).astype(np.int32)
    vote = G.soft.extract_soft(torch.from_numpy(blank).cuda().view(64, 4, 32, 32), e.s["keys"][0], e.s["nonces"][0], 256, thresholds=torch.from_numpy(thr).cuda())
    assert np.array_equal(vote.score.cpu().numpy(), score)
    want = R.decode(score)
    read = G.ecc.read(vote.score)
    _assert_read(read, want, "blank latents")
    assert not any(read.ok)
    ring = G.detect.Keyring()
    for i, (key, nonce) in enumerate(e.s["ring"]):
        ring.add(f"key{i}", key, nonce)
    results, reads = G.detect.detect_payloads(torch.from_numpy(blank[:8]).cuda().view(8, 4, 32, 32), ring, 256, reliability=15)
    assert all(r.key_id is None for r in results) and reads == [None] * 8


def _zero_eps(x, t, ctx):
    return torch.zeros_like(x)


def test_verify_records_returns_the_read_next_to_what_it_returns_today(G, E2E):
    e = E2E
    ctx = torch.zeros(1, 1, 1, device="cuda", dtype=torch.float32)
    pipe = G.pipeline.GaussianShadingPipeline(_zero_eps, e.s["keys"][0], e.s["nonces"][0], e.coded[0], height=256, width=256, num_inference_steps=10,
                                              dtype=torch.float32, ctx_uncond=ctx)
    today = pipe.verify_records(e.held_dev, e.rows, 32, soft=True)
    res, read, zi = pipe.verify_records(e.held_dev, e.rows, 32, soft=True, ecc="conv", return_latents=True)
    assert all(torch.equal(a, b) for a, b in zip(res, today)) and torch.equal(zi, pipe.invert(e.held_dev))
    _assert_read(read, R.decode(res.score.cpu().numpy()), "verify_records(soft=True)")
    (bits, flags, matches), read = pipe.verify_records(e.held_dev, e.rows, 32, ecc="conv")
    eb, ef, em, counts = G.codec.extract_records(zi, e.rows, 32, return_counts=True)
    assert torch.equal(bits, eb) and torch.equal(flags, ef) and torch.equal(matches, em)
    _assert_read(read, R.decode((2 * counts - 16).cpu().numpy()), "verify_records()")
    res, read = pipe.verify_records(e.held_dev, e.rows, 32, robust_levels=15, ecc="conv")
    _assert_read(read, R.decode(res.score.cpu().numpy()), "verify_records(robust_levels=15)")
    with pytest.raises(ValueError, match="ecc"):
        pipe.verify_records(e.held_dev, e.rows, 32, ecc="hamming")


def test_the_extract_line_carries_the_payload(G, E2E, capsys):
    """every decoder of `extract` with --ecc conv: the bit string is the vote's, the note the decode of that vote's own score"""
    e, X = E2E, G.extract
    own = [0, 12]                                                                                            # the images under key 0
    z = e.held_dev[own].contiguous()
    base = dict(key=e.s["keys"][0], nonce=e.s["nonces"][0], message_length=256, l=1, ecc="conv", soft_levels=15, soft_clip=2.5, tile=8, iters=2, sign_rounds=1)
    for extra in (dict(soft=1), dict(), dict(robust=1), dict(robust_soft=7), dict(window_soft=7, l=2)):
        args = SimpleNamespace(**{**base, **extra})
        out = X.recover_exactracted_message_batch(z, args)
        bits, flags, score = X._vote_scored(z, SimpleNamespace(**{**base, **extra, "ecc": None}), 256, args.l)
        want = R.decode(score.cpu().numpy())
        without = X.recover_exactracted_message_batch(z, SimpleNamespace(**{**base, **extra, "ecc": None}))
        for i in range(2):
            assert isinstance(out[i], str) and out[i] == without[i] and not hasattr(without[i], "note"), extra
            assert out[i].note == f"payload {R.payloads(want['info'], 256)[i].hex()} crc {'ok' if want['ok'][i] else 'FAILED'}, corrected {want['flips'][i]} of 256", extra
        if extra == dict(soft=1):
            vote = G.soft.extract_soft(z, base["key"], base["nonce"], 256, levels=15, clip=2.5)
            assert torch.equal(vote.score, score)
            assert [o.note for o in out] == [f"payload {e.s['payloads'][b].hex()} crc ok, corrected {want['flips'][i]} of 256" for i, b in enumerate(own)]
            one = X.recover_exactracted_message(z[1].cpu().numpy(), args)
            assert one == out[1] and one.note == out[1].note and X._ecc_note(one) == "\n" + out[1].note
        if extra == dict():
            _, _, counts = G.codec.extract_batch(z, base["key"], base["nonce"], 256, return_counts=True)
            assert torch.equal(2 * counts - 16, score)
    with pytest.raises(ValueError, match="--align"):
        X.recover_exactracted_message_batch(z, SimpleNamespace(**{**base, "align": "d4"}))
