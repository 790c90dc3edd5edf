"""GPU: punctured payload codes -- codec.viterbi_decode(code=) and codec.viterbi_list_decode(code=) against the NumPy restatement
of tests/ecc_rate_reference.py on poisoned, guard-banded buffers, then the read end to end at the rate walk's sigma: issue with ecc="conv23" / "conv34",
noise, extract_soft + ecc.read, detect.detect_payloads, verify_records and the extract line with --ecc_list 4.  EXACT equality of every output everywhere;
no tolerance.

The end-to-end noise is the sigma tools/ecc_rate_sigma_walk.py finds (profiles/ecc_rate_sigma_walk.txt, asserted by tests/test_ecc_rate_host.py): 1.75 for
both codes, the largest grid point at which all 20 payloads read back at L = 1.  No grid point separates L = 8 from L = 1 under the recorded draws, so the
list reads run at the same point."""
import uuid
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ecc_list_reference as LR
import ecc_rate_reference as Q
import ecc_reference as R
from poison import FINITE, NAN, Ledger, poisoned

pytestmark = pytest.mark.gpu

PUNCTURED = ("conv23", "conv34")
COPIES = 16


@pytest.fixture(scope="module")
def G():
    import gswm_amd  # noqa: F401
    from gswm_amd import _native, codec, detect, ecc, extract, issue, pipeline, soft, trace
    return SimpleNamespace(N=_native, codec=codec, detect=detect, ecc=ecc, extract=extract, issue=issue, pipeline=pipeline, soft=soft, trace=trace)


# ------------------------------------------------------------------------------------------------ the kernels against the restatement
def _codewords(rng, B, M, code):
    return np.stack([R.score_of(Q.encode(rng.bytes(Q.capacity(M, code)), M, code)) for _ in range(B)])


def _scores(pattern, B, M, code):
    rng = np.random.default_rng(M * 1009 + B * 17 + sum(map(ord, pattern + code)))
    if pattern == "noise":                                          # pure noise
        return rng.integers(-15 * COPIES, 15 * COPIES + 1, (B, M)).astype(np.int32)
    if pattern == "hard":                                           # +-1 rows
        return (2 * rng.integers(0, 2, (B, M)) - 1).astype(np.int32)
    if pattern == "ternary":                                        # ties at most steps
        return rng.integers(-1, 2, (B, M)).astype(np.int32)
    if pattern == "zeros":                                          # every branch ties
        return np.zeros((B, M), dtype=np.int32)
    if pattern == "codebig":                                        # sum |score| just under 2^30
        return _codewords(rng, B, M, code) * ((2 ** 30 - 1) // M)
    assert pattern == "noisy"                                       # codewords of amplitude 40 under noise of the same order
    return (_codewords(rng, B, M, code) * 40 + rng.integers(-60, 61, (B, M))).astype(np.int32)


# (code, M, L, B, pad of the row stride, pattern); L = 0 is the plain read.  M = 64 (both codes: 4 and 0 spare positions), M = 80 at conv34 (the tail inside a
# period, 5 spare positions), 256, 2048 (several waves per workgroup at the plain read and L = 1, 2), 8192 at conv34 plain (the LDS maximum); B in {1, 3, 5, 64}
# (a wave past the batch at 3 and 5); strides M and M + 16; the six row patterns at both codes and at the plain and the list reads.
CASES = [("conv23", 64, 0, 1, 0, "noisy"), ("conv23", 64, 2, 3, 16, "zeros"), ("conv23", 64, 4, 5, 0, "ternary"), ("conv23", 64, 8, 64, 0, "noise"),
         ("conv34", 64, 0, 5, 16, "ternary"), ("conv34", 64, 2, 64, 0, "noisy"), ("conv34", 64, 4, 1, 0, "codebig"), ("conv34", 64, 8, 3, 16, "zeros"),
         ("conv34", 80, 0, 3, 0, "noisy"), ("conv34", 80, 0, 64, 16, "zeros"), ("conv34", 80, 2, 5, 0, "hard"), ("conv34", 80, 4, 64, 16, "noisy"),
         ("conv34", 80, 8, 1, 0, "ternary"), ("conv23", 80, 0, 5, 0, "codebig"), ("conv23", 80, 8, 3, 0, "noisy"),
         ("conv23", 256, 0, 64, 16, "noisy"), ("conv23", 256, 0, 3, 0, "zeros"), ("conv23", 256, 2, 5, 16, "noise"), ("conv23", 256, 4, 64, 0, "noisy"),
         ("conv23", 256, 8, 3, 0, "hard"), ("conv34", 256, 0, 5, 0, "hard"), ("conv34", 256, 0, 1, 16, "codebig"), ("conv34", 256, 2, 64, 0, "ternary"),
         ("conv34", 256, 4, 3, 16, "zeros"), ("conv34", 256, 8, 64, 16, "noisy"), ("conv34", 256, 8, 5, 0, "codebig"),
         ("conv23", 2048, 0, 5, 16, "noisy"), ("conv23", 2048, 2, 3, 0, "noise"), ("conv23", 2048, 8, 3, 0, "noisy"), ("conv34", 2048, 0, 64, 0, "noise"),
         ("conv34", 2048, 1, 5, 0, "noisy"), ("conv34", 2048, 4, 5, 16, "noisy"), ("conv34", 2048, 8, 1, 0, "ternary"),
         ("conv34", 8192, 0, 1, 16, "noisy"), ("conv34", 8192, 0, 3, 0, "ternary"), ("conv23", 8192, 0, 1, 0, "noise")]
# the largest M the plan serves at each (code, L): one wave with up to the whole LDS of a compute unit
CASES += [(code, Q.largest_served(L, code), L, 1 if L < 8 else 3, 16 * (L & 1), "noisy") for code in PUNCTURED for L in LR.LIST_SIZES]
_WANT = {}


def _want(code, M, L, B, pattern):
    """the restatement of a case, computed once and shared by both poison patterns"""
    key = (code, M, L, B, pattern)
    if key not in _WANT:
        sc = _scores(pattern, B, M, code)
        sc.setflags(write=False)
        _WANT[key] = (sc, Q.decode_list(sc, L, code) if L else Q.decode(sc, code))
    return _WANT[key]


def _assert_decode(got, want, where):
    names = Q.NAMES if "rank" in want else Q.PLAIN
    assert [t.dtype for t in got] == [torch.uint8, torch.uint8] + [torch.int32] * (len(names) - 2), where
    for name in names:
        g, w = getattr(got, name).cpu().numpy(), want[name]
        assert g.shape == w.shape, (where, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            rows = np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0]
            raise AssertionError(f"{where}: {name} differs in rows {rows[:8].tolist()} ({len(rows)} of {len(g)})")


def _run(G, sc, L, code):
    return G.codec.viterbi_list_decode(sc, L, code=code) if L else G.codec.viterbi_decode(sc, code=code)


@pytest.mark.parametrize("code,M,L,B,pad,pattern", CASES)
@pytest.mark.parametrize("poison", [NAN, FINITE])
def test_punctured_decode_matches_the_restatement_on_poisoned_buffers(G, code, M, L, B, pad, pattern, poison):
    assert Q.served(M, L or 1, code) and (L or M <= 8192)
    sc, want = _want(code, M, L, B, pattern)
    wide = np.full((B, M + pad), 2 ** 31 - 1, dtype=np.int32)       # what lies between the rows must not be read: it would break the bound at once
    wide[:, :M] = sc
    led = Ledger(poison)
    with poisoned(led):
        got = _run(G, led.wrap(torch.from_numpy(wide).cuda())[:, :M], L, code)
    led.check()
    _assert_decode(got, want, (code, M, L, B, pad, pattern))
    assert tuple(got.info.shape) == (B, Q.sizes(M, code)[1] // 8)


def test_every_output_element_is_written(G):
    """all-zero votes decode to zeros everywhere (the zero word at rank 0, no rank passes: the CRC of zero bytes is not zero), which no pattern byte equals"""
    for code, M, L, B in (("conv23", 64, 0, 1), ("conv34", 64, 8, 5), ("conv34", 80, 0, 64), ("conv34", 80, 2, 3), ("conv23", 256, 4, 5), ("conv34", 2048, 0, 5),
                          ("conv23", 2048, 8, 3), ("conv34", 8192, 0, 2)):
        for poison in (NAN, FINITE):
            led = Ledger(poison)
            with poisoned(led):
                got = _run(G, torch.zeros((B, M), dtype=torch.int32, device="cuda"), L, code)
            led.check()
            assert all(led.untouched(t) == 0 for t in got), [led.where(t) for t in got if led.untouched(t)]
            assert all(not bool(t.any()) for t in got), (code, M, L, B)
            assert tuple(got.info.shape) == (B, Q.sizes(M, code)[1] // 8) and tuple(got.message.shape) == (B, M // 8) and all(tuple(t.shape) == (B,) for t in got[2:])


def test_codewords_at_the_int32_bound_read_back(G):
    """`codebig`: sum |score| just under 2^30 over M positions; the metric is the sum over the N code positions, every payload reads back at rank 0"""
    for code, M, L in (("conv34", 64, 4), ("conv34", 256, 0), ("conv34", 256, 8), ("conv23", 80, 0)):
        B = {("conv34", 64, 4): 1, ("conv34", 256, 0): 1, ("conv34", 256, 8): 5, ("conv23", 80, 0): 5}[(code, M, L)]
        sc, want = _want(code, M, L, B, "codebig")
        pos = Q.layout(M, code)[2]
        assert 2 ** 30 - M <= int(np.abs(sc.astype(np.int64)).sum(axis=1).min()) < 2 ** 30
        assert want["ok"].all() and not want["flips"].any() and (want["metric"] == np.abs(sc.astype(np.int64))[:, pos].sum(axis=1)).all()


def test_votes_at_spare_positions_change_no_output_byte(G):
    """the M - N spare positions overwritten with +-2^20: every output stays what it was (and what the restatement gives)"""
    for code, M, L, B, pattern in (("conv23", 64, 0, 1, "noisy"), ("conv34", 80, 4, 64, "noisy"), ("conv34", 80, 0, 3, "noisy"), ("conv23", 256, 4, 64, "noisy"),
                                   ("conv23", 2048, 8, 3, "noisy")):
        sc, want = _want(code, M, L, B, pattern)
        spare = np.setdiff1d(np.arange(M), Q.layout(M, code)[2])
        assert len(spare) == M - Q.sizes(M, code)[2] > 0
        loud = sc.copy()
        loud[:, spare] = np.where(np.arange(len(spare)) % 2, 2 ** 20, -2 ** 20).astype(np.int32)
        _assert_decode(_run(G, torch.from_numpy(loud).cuda(), L, code), want, ("spare", code, M, L))


def test_rate_zero_through_the_new_entry_points_is_the_old_entry_points(G):
    import test_gpu_viterbi as V
    lib = G.N.lib()
    for M, B, pattern in ((64, 5, "ternary"), (80, 3, "uniform"), (256, 64, "burst"), (2048, 3, "uniform"), (8192, 1, "hard")):
        sc = torch.from_numpy(V._scores(pattern, B, M)).cuda()
        new = lambda *n: [torch.full((B * k,), 0x5A, dtype=torch.uint8, device="cuda") for k in n]
        old = G.codec.viterbi_decode(sc)
        outs = new(M // 16, M // 8, 4, 4, 4)
        assert lib.gsw_viterbi_decode_rate(sc.data_ptr(), M, B, M, 0, *[t.data_ptr() for t in outs], None) == 0
        torch.cuda.synchronize()
        for a, b in zip(old, outs):
            assert torch.equal(a.contiguous().view(torch.uint8).reshape(-1), b), (M, B, pattern)
        for L in (1, 2, 4, 8):
            if M > LR.largest_served(L):
                continue
            old = G.codec.viterbi_list_decode(sc, L)
            outs = new(M // 16, M // 8, 4, 4, 4, 4, 4)
            assert lib.gsw_viterbi_list_decode_rate(sc.data_ptr(), M, B, M, 0, L, *[t.data_ptr() for t in outs], None) == 0
            torch.cuda.synchronize()
            for a, b in zip(old, outs):
                assert torch.equal(a.contiguous().view(torch.uint8).reshape(-1), b), (M, B, pattern, L)


def test_refusals_return_before_any_launch_and_write_nothing(G):
    N, lib = G.N, G.N.lib()
    z = lambda *shape, dtype=torch.int32: torch.zeros(shape, dtype=dtype, device="cuda")
    B = 2
    cases = [(256, 3, 1, N.GSW_ERR_BAD_ARG), (256, -1, 4, N.GSW_ERR_BAD_ARG), (256, 1, 3, N.GSW_ERR_BAD_ARG), (72, 1, 2, N.GSW_ERR_BAD_ARG)]
    cases += [(Q.largest_served(L, code) + 16, Q.CODES.index(code), L, N.GSW_ERR_UNSUPPORTED) for code in PUNCTURED for L in LR.LIST_SIZES]
    for M, rate, L, want in cases:
        score = z(B, M)
        outs = [torch.full((B * n,), 0x5A, dtype=torch.uint8, device="cuda") for n in (M // 8, M // 8, 4, 4, 4, 4, 4)]
        st = lib.gsw_viterbi_list_decode_rate(score.data_ptr(), M, B, M, rate, L, *[t.data_ptr() for t in outs], None)
        torch.cuda.synchronize()
        assert st == want and all(bool((t == 0x5A).all()) for t in outs), (M, rate, L, st)
    for M, rate, want in ((256, 3, N.GSW_ERR_BAD_ARG), (256, -1, N.GSW_ERR_BAD_ARG), (8208, 2, N.GSW_ERR_UNSUPPORTED), (8208, 1, N.GSW_ERR_UNSUPPORTED),
                          (8208, 7, N.GSW_ERR_BAD_ARG), (250, 1, N.GSW_ERR_BAD_ARG)):
        score = z(B, M)
        outs = [torch.full((B * n,), 0x5A, dtype=torch.uint8, device="cuda") for n in (M // 8, M // 8, 4, 4, 4)]
        st = lib.gsw_viterbi_decode_rate(score.data_ptr(), M, B, M, rate, *[t.data_ptr() for t in outs], None)
        torch.cuda.synchronize()
        assert st == want and all(bool((t == 0x5A).all()) for t in outs), (M, rate, st)
    for code in ("conv12", None, 1, b"conv"):
        with pytest.raises(ValueError, match="code"):
            G.codec.viterbi_decode(z(2, 256), code=code)
        with pytest.raises(ValueError, match="code"):
            G.codec.viterbi_list_decode(z(2, 256), 4, code=code)
    for code in PUNCTURED:
        with pytest.raises(ValueError, match="multiple of 16"):
            G.codec.viterbi_decode(z(2, 8208), code=code)
        with pytest.raises(ValueError, match="LDS"):
            G.codec.viterbi_list_decode(z(1, Q.largest_served(8, code) + 16), 8, code=code)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            G.codec.viterbi_decode(torch.zeros(2, 256, dtype=torch.int32), code=code)


# ------------------------------------------------------------------------------------------------ end to end at the rate walk's sigma
@pytest.fixture(scope="module", params=PUNCTURED)
def E2E(G, request):
    """the 20 walk latents issued with ecc=code under their own records (12 keys), noise of the walk's sigma added; the restatement's votes"""
    code = request.param
    s = R.walk_setup()
    B, M, shape = R.WALK["images"], R.WALK["M"], R.WALK["shape"]
    sent = Q.walk_payloads(code)
    reg = G.trace.KeyedRegistry(M // 8)
    reqs = [G.issue.Request(f"user{b}", sent[b], s["keys"][b], s["nonces"][b]) for b in range(B)]
    np.random.seed(R.WALK["seed"])                                  # issue_latents(seed=None) draws NumPy's global MT19937 stream: the walk's uniforms
    z, rows = G.issue.issue_latents(reqs, shape, registry=reg, ecc=code)
    held = R.held(z.cpu().numpy().reshape(B, -1), s["noise"], Q.RATE_WALK[code]["sigma"])
    score, thr = R.walk_scores(s, held, M)
    ring = G.detect.Keyring()
    for i, (key, nonce) in enumerate(s["ring"]):
        ring.add(f"key{i}", key, nonce)
    return SimpleNamespace(code=code, s=s, B=B, M=M, sent=sent, rows=rows, held_dev=torch.from_numpy(held).cuda().view(B, *shape), score=score, thr=thr, ring=ring,
                           want={L: Q.decode_list(score, L, code) for L in LR.LIST_SIZES})


def _assert_read(read, want, where, code, M=256):
    lst = "rank" in want
    assert type(read).__name__ == ("EccListRead" if lst else "EccRead"), where
    assert read.payload == Q.payloads(want["info"], M, code), where
    assert read.ok == [bool(v) for v in want["ok"]] and read.flips == want["flips"].tolist() and read.metric == want["metric"].tolist(), where
    if lst:
        assert read.rank == want["rank"].tolist() and read.n_ok == want["n_ok"].tolist(), where
    assert np.array_equal(read.message.cpu().numpy(), want["message"]), where


def _row(want, b):
    return {k: v[b:b + 1] for k, v in want.items()}


def _plain(want):
    return {k: want[k] for k in Q.PLAIN}


def test_payloads_read_back_through_extract_soft_and_read(G, E2E):
    e = E2E
    vote = G.codec.extract_soft(e.held_dev, e.rows, 32, torch.from_numpy(e.thr).cuda())
    assert np.array_equal(vote.score.cpu().numpy(), e.score)       # the device votes are the CPU walk's votes
    read = G.ecc.read(vote.score, code=e.code)
    _assert_read(read, _plain(e.want[1]), "read", e.code)
    assert read.payload == e.sent and all(read.ok)                  # all 20 payloads read back
    for L in (2, 4, 8):
        rl = G.ecc.read_list(vote.score, L, code=e.code)
        _assert_read(rl, e.want[L], f"read_list L = {L}", e.code)
        assert rl.payload == e.sent and all(rl.ok) and Q.RATE_WALK[e.code]["reads"][L] == e.B
    assert type(G.ecc.read_any(vote.score, 1, e.code)).__name__ == "EccRead" and G.ecc.read_any(vote.score, 4, e.code)[:4] == G.ecc.read_list(vote.score, 4, e.code)[:4]


def test_detect_payloads_reads_the_punctured_payloads(G, E2E):
    e = E2E
    plain = G.detect.detect_latents(e.held_dev, e.ring, 256, reliability=15)
    results, reads = G.detect.detect_payloads(e.held_dev, e.ring, 256, ecc=e.code, reliability=15)
    assert results == plain and [r.key_id for r in results] == [f"key{b % 12}" for b in range(e.B)]
    vote = G.codec.extract_soft(e.held_dev, e.rows, 32, G.soft.uniform_thresholds(e.held_dev, 15, 2.5))      # the read's own table, the image's own key
    want = Q.decode(vote.score.cpu().numpy(), e.code)
    for b in range(e.B):
        _assert_read(reads[b], _row(want, b), f"detect_payloads image {b}", e.code)
    assert [r.payload[0] for r in reads] == e.sent and all(r.ok == [True] for r in reads)
    results, reads = G.detect.detect_payloads(e.held_dev, e.ring, 256, ecc=e.code, reliability=15, list_size=4)
    want = Q.decode_list(vote.score.cpu().numpy(), 4, e.code)
    for b in range(e.B):
        _assert_read(reads[b], _row(want, b), f"detect_payloads(list_size=4) image {b}", e.code)
    # the sign statistic: 2 counts - copies under the named key
    results, reads = G.detect.detect_payloads(e.held_dev, e.ring, 256, ecc=e.code)
    _, _, _, counts = G.codec.extract_records(e.held_dev, e.rows, 32, return_counts=True)
    want = Q.decode((2 * counts - 16).cpu().numpy(), e.code)
    named = [b for b in range(e.B) if results[b].key_id is not None]
    assert named and all(results[b].key_id == f"key{b % 12}" for b in named)
    for b in range(e.B):
        if b in named:
            _assert_read(reads[b], _row(want, b), f"detect_payloads (signs) image {b}", e.code)
        else:
            assert reads[b] is None


def _zero_eps(x, t, ctx):
    return torch.zeros_like(x)


def test_verify_records_reads_the_punctured_payloads(G, E2E):
    e = E2E
    ctx = torch.zeros(1, 1, 1, device="cuda", dtype=torch.float32)
    pipe = G.pipeline.GaussianShadingPipeline(_zero_eps, e.s["keys"][0], e.s["nonces"][0], Q.encode(e.sent[0], 256, e.code), height=256, width=256,
                                              num_inference_steps=10, dtype=torch.float32, ctx_uncond=ctx)
    without = pipe.verify_records(e.held_dev, e.rows, 32, soft=True)
    res, read = pipe.verify_records(e.held_dev, e.rows, 32, soft=True, ecc=e.code)
    assert all(torch.equal(a, b) for a, b in zip(res, without))
    _assert_read(read, Q.decode(res.score.cpu().numpy(), e.code), "verify_records(soft=True)", e.code)
    res, read = pipe.verify_records(e.held_dev, e.rows, 32, soft=True, ecc=e.code, ecc_list=8)
    _assert_read(read, Q.decode_list(res.score.cpu().numpy(), 8, e.code), "verify_records(soft=True, ecc_list=8)", e.code)
    (bits, flags, matches), read = pipe.verify_records(e.held_dev, e.rows, 32, ecc=e.code, ecc_list=2)
    _, _, _, counts = G.codec.extract_records(pipe.invert(e.held_dev), e.rows, 32, return_counts=True)
    _assert_read(read, Q.decode_list((2 * counts - 16).cpu().numpy(), 2, e.code), "verify_records(ecc_list=2)", e.code)
    with pytest.raises(ValueError, match="ecc"):
        pipe.verify_records(e.held_dev, e.rows, 32, soft=True, ecc="conv56")


def test_the_extract_line_carries_the_punctured_payload(G, E2E):
    """every decoder of `extract` with --ecc <code> --ecc_list 4: the bit string is the vote's, the note the list decode of that vote's own score"""
    e, X = E2E, G.extract
    own = [0, 12]                                                                                            # the images under key 0
    z = e.held_dev[own].contiguous()
    base = dict(key=e.s["keys"][0], nonce=e.s["nonces"][0], message_length=256, l=1, ecc=e.code, ecc_list=4, soft_levels=15, soft_clip=2.5, tile=8, iters=2,
                sign_rounds=1)
    for extra in (dict(soft=1), dict(), dict(robust=1), dict(robust_soft=7), dict(window_soft=7, l=2)):
        args = SimpleNamespace(**{**base, **extra})
        out = X.recover_exactracted_message_batch(z, args)
        bits, flags, score = X._vote_scored(z, SimpleNamespace(**{**base, **extra, "ecc": None, "ecc_list": 1}), 256, args.l)
        want4, want1 = Q.decode_list(score.cpu().numpy(), 4, e.code), Q.decode(score.cpu().numpy(), e.code)
        one = X.recover_exactracted_message_batch(z, SimpleNamespace(**{**base, **extra, "ecc_list": 1}))
        for i in range(2):
            assert isinstance(out[i], str) and out[i] == one[i], extra
            assert out[i].note == Q.format_read(want4, i, 256, e.code, 4), extra
            assert one[i].note == Q.format_read(want1, i, 256, e.code), extra
        if extra == dict(soft=1):
            assert [o.note.split(",")[0] for o in out] == [f"payload {e.sent[b].hex()} crc ok" for b in own]
            assert all(f"of {Q.sizes(256, e.code)[2]}, list rank 0 of 4" in o.note for o in out)
            single = X.recover_exactracted_message(z[1].cpu().numpy(), args)
            assert single == out[1] and single.note == out[1].note
    with pytest.raises(ValueError, match="--align"):
        X.recover_exactracted_message_batch(z, SimpleNamespace(**{**base, "align": "d4"}))
    with pytest.raises(ValueError, match="--gpus"):
        X.recover_exactracted_message_batch(z, SimpleNamespace(**{**base, "gpus": 2}))


def test_a_uuid_and_two_bytes_round_trip_in_a_256_bit_message(G):
    """conv23 carries 18 bytes in 256 bits: a 16-byte UUID plus 2 bytes goes issue -> noise -> read; under "conv" the same request is refused (13 bytes)"""
    s = R.walk_setup()
    shape, n = R.WALK["shape"], int(np.prod(R.WALK["shape"]))
    payload = uuid.UUID("6f1d2c3b-4a59-4e87-9b0a-c1d2e3f4a5b6").bytes + b"\x07\xe9"
    assert len(payload) == 18 == G.ecc.capacity(256, "conv23") > G.ecc.capacity(256)
    reg = G.trace.KeyedRegistry(32)
    req = [G.issue.Request("user0", payload, s["keys"][0], s["nonces"][0])]
    with pytest.raises(ValueError, match="13"):
        G.issue.issue_latents(req, shape, registry=G.trace.KeyedRegistry(32), ecc="conv")
    np.random.seed(R.WALK["seed"])
    z, rows = G.issue.issue_latents(req, shape, registry=reg, ecc="conv23")
    held = R.held(z.cpu().numpy().reshape(1, n), s["noise"][:1], 1.5)
    held_dev = torch.from_numpy(held).cuda().view(1, *shape)
    vote = G.codec.extract_soft(held_dev, rows, 32, G.soft.uniform_thresholds(held_dev, 15, 2.5))
    read = G.ecc.read(vote.score, code="conv23")
    want = Q.decode(vote.score.cpu().numpy(), "conv23")
    _assert_read(read, want, "uuid", "conv23")
    assert read.ok == [True] and read.payload == [payload] and uuid.UUID(bytes=read.payload[0][:16]) == uuid.UUID("6f1d2c3b-4a59-4e87-9b0a-c1d2e3f4a5b6")
    assert np.array_equal(read.message.cpu().numpy()[0], np.frombuffer(Q.encode(payload, 256, "conv23"), dtype=np.uint8))
    assert G.ecc.format_read(read, 0, 256, "conv23") == Q.format_read(want, 0, 256, "conv23") and " of 252" in G.ecc.format_read(read, 0, 256, "conv23")
