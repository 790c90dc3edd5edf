"""GPU: the list read of error-corrected payloads -- codec.viterbi_list_decode against the NumPy restatement of
tests/ecc_list_reference.py on poisoned, guard-banded buffers, then the read end to end at the list walk's sigma: issue with ecc="conv", noise,
extract_soft + ecc.read_list, detect.detect_payloads(list_size=), verify_records(ecc_list=) and the extract line.  EXACT equality of all seven outputs
everywhere; no tolerance.

The end-to-end noise is the sigma tools/ecc_list_sigma_walk.py finds (profiles/ecc_list_sigma_walk.txt, asserted by tests/test_ecc_list_host.py): 2.75, the
largest grid point at which all 20 payloads read back at L = 8 and fewer at L = 1 (16 / 18 / 20 / 20 of 20 at L = 1 / 2 / 4 / 8)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ecc_list_reference as LR
import ecc_reference as R
import test_gpu_viterbi as V
from poison import FINITE, NAN, Ledger, poisoned

pytestmark = pytest.mark.gpu

SIGMA = LR.LIST_WALK["sigma"]
NAMES = LR.NAMES


@pytest.fixture(scope="module")
def G():
    import gswm_amd  # noqa: F401
    from gswm_amd import _native, codec, detect, ecc, extract, issue, pipeline, soft, trace
    return SimpleNamespace(N=_native, codec=codec, detect=detect, ecc=ecc, extract=extract, issue=issue, pipeline=pipeline, soft=soft, trace=trace)


# ------------------------------------------------------------------------------------------------ the kernel against the restatement
# (M, L, B, pad of the row stride, pattern).  Every (M, L) pair of M in {64, 80, 256, 272, 2048} x L in {1, 2, 4, 8} appears; B in {1, 3, 70} (and one B = 2):
# workgroups of four waves (the short messages), two (M = 2048 at L = 2; B = 2) and one (M = 2048 at L = 4 and 8; B = 1), the last workgroup filled (B = 1,
# B = 2, one-wave workgroups) and not filled (3 of 4, 70 = 17 x 4 + 2, 3 = 2 + 1); strides M and M + 16; the seven patterns of tests/test_gpu_viterbi.py,
# `zeros` and `ternary` (ties at nearly every merge) at every L; then the largest M the plan serves at each L, one wave with up to the whole LDS of a CU.
CASES = [(64, 1, 70, 16, "ternary"), (64, 2, 3, 0, "zeros"), (64, 4, 1, 0, "uniform"), (64, 8, 70, 0, "ternary"),
         (80, 1, 3, 0, "hard"), (80, 2, 70, 16, "ternary"), (80, 4, 70, 0, "zeros"), (80, 8, 3, 16, "codebig"),
         (256, 1, 3, 16, "zeros"), (256, 2, 70, 0, "burst"), (256, 4, 3, 16, "ternary"), (256, 8, 70, 16, "uniform"), (256, 8, 3, 0, "zeros"),
         (272, 1, 70, 0, "code1"), (272, 2, 1, 16, "uniform"), (272, 4, 70, 16, "hard"), (272, 8, 1, 0, "burst"),
         (2048, 1, 1, 0, "codebig"), (2048, 2, 3, 16, "hard"), (2048, 4, 3, 0, "code1"), (2048, 8, 70, 0, "uniform"), (2048, 8, 3, 16, "ternary"),
         (256, 4, 2, 0, "code1")]
CASES += [(LR.largest_served(L), L, 1 if L < 8 else 3, 16 * (L & 1), "uniform") for L in LR.LIST_SIZES]
_WANT = {}


def _want(M, L, B, pattern):
    """the restatement of a case, computed once and shared by both poison patterns"""
    key = (M, L, B, pattern)
    if key not in _WANT:
        sc = V._scores(pattern, B, M) if M <= 8192 else np.random.default_rng(M + L).integers(-240, 241, (B, M)).astype(np.int32)
        sc.setflags(write=False)
        _WANT[key] = (sc, LR.decode_list(sc, L))
    return _WANT[key]


def _assert_decode(got, want, where):
    assert [t.dtype for t in got] == [torch.uint8, torch.uint8] + [torch.int32] * 5, where
    for name in NAMES:
        g, w = getattr(got, name).cpu().numpy(), want[name]
        assert g.shape == w.shape, (where, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            rows = np.nonzero((g != w).reshape(len(g), -1).any(axis=1))[0]
            raise AssertionError(f"{where}: {name} differs in rows {rows[:8].tolist()} ({len(rows)} of {len(g)})")


@pytest.mark.parametrize("M,L,B,pad,pattern", CASES)
@pytest.mark.parametrize("poison", [NAN, FINITE])
def test_list_decode_matches_the_restatement_on_poisoned_buffers(G, M, L, B, pad, pattern, poison):
    assert LR.served(M, L)
    sc, want = _want(M, L, B, pattern)
    wide = np.full((B, M + pad), 2 ** 31 - 1, dtype=np.int32)       # what lies between the rows must not be read: it would break the bound at once
    wide[:, :M] = sc
    led = Ledger(poison)
    with poisoned(led):
        got = G.codec.viterbi_list_decode(led.wrap(torch.from_numpy(wide).cuda())[:, :M], L)
    led.check()
    _assert_decode(got, want, (M, L, B, pad, pattern))


def test_every_output_element_is_written(G):
    """all-zero votes decode to zeros everywhere (rank 0 is the zero word, no rank passes: the CRC of zero bytes is not zero), which no pattern byte equals"""
    for M, L, B in ((64, 8, 1), (80, 2, 70), (256, 4, 3), (272, 1, 5), (2048, 8, 5)):
        for poison in (NAN, FINITE):
            led = Ledger(poison)
            with poisoned(led):
                got = G.codec.viterbi_list_decode(torch.zeros((B, M), dtype=torch.int32, device="cuda"), L)
            led.check()
            assert all(led.untouched(t) == 0 for t in got), [led.where(t) for t in got if led.untouched(t)]
            assert all(not bool(t.any()) for t in got), (M, L, B)
            assert tuple(got.info.shape) == (B, M // 16) and tuple(got.message.shape) == (B, M // 8) and all(tuple(t.shape) == (B,) for t in got[2:])


def test_list_size_one_is_the_plain_decode(G):
    for M, B, pattern in ((256, 70, "uniform"), (80, 3, "ternary"), (2048, 3, "burst"), (64, 5, "zeros")):
        sc = torch.from_numpy(V._scores(pattern, B, M)).cuda()
        plain, one = G.codec.viterbi_decode(sc), G.codec.viterbi_list_decode(sc, 1)
        for a, b in zip(plain, one[:5]):
            assert a.dtype == b.dtype and torch.equal(a, b), (M, B, pattern)
        assert not bool(one.rank.any()) and torch.equal(one.n_ok, one.ok)


def test_metrics_just_under_the_int32_bound_do_not_wrap(G):
    """`codebig`: sum |score| just under 2^30 -- every one of the 8 metrics of a state, and every candidate of a merge, stays inside int32"""
    for M, B in ((64, 3), (256, 3)):
        sc = V._scores("codebig", B, M)
        assert 2 ** 30 - M <= int(np.abs(sc.astype(np.int64)).sum(axis=1).min()) < 2 ** 30
        want = LR.decode_list(sc, 8)
        _assert_decode(G.codec.viterbi_list_decode(torch.from_numpy(sc).cuda(), 8), want, ("codebig", M))
        assert want["ok"].all() and (want["metric"] == np.abs(sc.astype(np.int64)).sum(axis=1)).all() and not want["rank"].any()


def test_a_length_beyond_the_lds_bound_is_unsupported_and_writes_nothing(G):
    N = G.N
    for L in LR.LIST_SIZES:
        M, B = LR.largest_served(L) + 16, 2
        assert not LR.served(M, L)
        score = torch.zeros((B, M), dtype=torch.int32, device="cuda")
        with pytest.raises(ValueError, match="LDS"):
            G.codec.viterbi_list_decode(score, L)
        outs = [torch.full((B * n,), 0x5A, dtype=torch.uint8, device="cuda") for n in (M // 16, M // 8, 4, 4, 4, 4, 4)]
        st = N.lib().gsw_viterbi_list_decode(score.data_ptr(), M, B, M, L, *[t.data_ptr() for t in outs], None)
        torch.cuda.synchronize()
        assert st == N.GSW_ERR_UNSUPPORTED
        assert all(bool((t == 0x5A).all()) for t in outs)


def test_the_wrapper_refuses_before_any_launch(G):
    z = lambda *shape, dtype=torch.int32: torch.zeros(shape, dtype=dtype, device="cuda")
    for L in (0, 3, 16, -1, True, 2.0, None, "8"):
        with pytest.raises(ValueError, match="list_size"):
            G.codec.viterbi_list_decode(z(2, 256), L)
    for M in (48, 72, 250):
        with pytest.raises(ValueError, match="multiple of 16"):
            G.codec.viterbi_list_decode(z(2, M), 4)
    for bad in (z(2, 256, dtype=torch.int64), z(256), z(0, 256), z(2, 512)[:, ::2], z(1, 256).expand(3, 256), None):
        with pytest.raises(ValueError):
            G.codec.viterbi_list_decode(bad, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        G.codec.viterbi_list_decode(torch.zeros(2, 256, dtype=torch.int32), 4)
    with pytest.raises(ValueError, match="8192"):
        G.ecc.read_list(z(1, 8208), 2)                                # the kernel serves it; a payload is not defined there


# ------------------------------------------------------------------------------------------------ end to end at the list walk's sigma
@pytest.fixture(scope="module")
def E2E(G):
    """the 20 walk latents issued with ecc="conv" under their own records (12 keys), noise of the list walk's sigma added; the restatement's votes"""
    s = R.walk_setup()
    B, M, shape = R.WALK["images"], R.WALK["M"], R.WALK["shape"]
    reg = G.trace.KeyedRegistry(M // 8)
    reqs = [G.issue.Request(f"user{b}", s["payloads"][b], s["keys"][b], s["nonces"][b]) for b in range(B)]
    np.random.seed(R.WALK["seed"])                                  # issue_latents(seed=None) draws NumPy's global MT19937 stream: the walk's uniforms
    z, rows = G.issue.issue_latents(reqs, shape, registry=reg, ecc="conv")
    held = R.held(z.cpu().numpy().reshape(B, -1), s["noise"], SIGMA)
    score, thr = R.walk_scores(s, held, M)
    ring = G.detect.Keyring()
    for i, (key, nonce) in enumerate(s["ring"]):
        ring.add(f"key{i}", key, nonce)
    return SimpleNamespace(s=s, B=B, M=M, rows=rows, held_dev=torch.from_numpy(held).cuda().view(B, *shape), score=score, thr=thr, ring=ring,
                           want={L: LR.decode_list(score, L) for L in LR.LIST_SIZES})


def _assert_read(read, want, where, M=256):
    assert type(read).__name__ == "EccListRead", where
    assert read.payload == R.payloads(want["info"], M), where
    assert read.ok == [bool(v) for v in want["ok"]] and read.flips == want["flips"].tolist() and read.metric == want["metric"].tolist(), where
    assert read.rank == want["rank"].tolist() and read.n_ok == want["n_ok"].tolist(), where
    assert np.array_equal(read.message.cpu().numpy(), want["message"]), where


def _row(want, b):
    return {k: v[b:b + 1] for k, v in want.items()}


def test_payloads_read_back_through_extract_soft_and_read_list(G, E2E):
    e = E2E
    vote = G.codec.extract_soft(e.held_dev, e.rows, 32, torch.from_numpy(e.thr).cuda())
    assert np.array_equal(vote.score.cpu().numpy(), e.score)
    for L in (2, 4, 8):
        read = G.ecc.read_list(vote.score, L)
        _assert_read(read, e.want[L], f"read_list L = {L}")
        right = sum(1 for b in range(e.B) if read.ok[b] and read.payload[b] == e.s["payloads"][b])
        assert right == LR.LIST_WALK["reads"][L] and sum(read.ok) == right                       # no wrong payload passes
    read8 = G.ecc.read_list(vote.score, 8)
    assert read8.payload == e.s["payloads"] and all(read8.ok) and max(read8.rank) > 0           # every payload, some of them from below rank 0
    # list size 1: today's launch, today's EccRead, today's count
    today = G.ecc.read(vote.score)
    one = G.ecc.read_any(vote.score, 1)
    assert type(one).__name__ == "EccRead" and one[:4] == today[:4] and torch.equal(one.message, today.message)
    assert sum(1 for b in range(e.B) if today.ok[b] and today.payload[b] == e.s["payloads"][b]) == LR.LIST_WALK["reads"][1] < e.B
    _assert_read(G.ecc.read_list(vote.score, 1), e.want[1], "read_list L = 1")
    assert G.ecc.read_list(vote.score, 1)[:4] == today[:4]


def test_detect_payloads_with_a_list(G, E2E):
    e = E2E
    plain = G.detect.detect_latents(e.held_dev, e.ring, 256, reliability=15)
    results, reads = G.detect.detect_payloads(e.held_dev, e.ring, 256, reliability=15, list_size=8)
    assert results == plain and [r.key_id for r in results] == [f"key{b % 12}" for b in range(e.B)]
    vote = G.codec.extract_soft(e.held_dev, e.rows, 32, G.soft.uniform_thresholds(e.held_dev, 15, 2.5))      # the read's own table, the image's own key
    want = LR.decode_list(vote.score.cpu().numpy(), 8)
    for b in range(e.B):
        _assert_read(reads[b], _row(want, b), f"detect_payloads image {b}")
    right = sum(1 for b in range(e.B) if reads[b].ok == [True] and reads[b].payload == [e.s["payloads"][b]])
    assert right == sum(1 for b, p in enumerate(e.s["payloads"]) if want["ok"][b] and R.payloads(want["info"], 256)[b] == p) >= LR.LIST_WALK["reads"][1]
    # list_size 1 is today's call
    r1, reads1 = G.detect.detect_payloads(e.held_dev, e.ring, 256, reliability=15, list_size=1)
    r0, reads0 = G.detect.detect_payloads(e.held_dev, e.ring, 256, reliability=15)
    assert r1 == r0 and all(type(a).__name__ == "EccRead" and a[:4] == b[:4] for a, b in zip(reads1, reads0))
    # the sign statistic: 2 counts - copies under the named key
    results, reads = G.detect.detect_payloads(e.held_dev, e.ring, 256, list_size=4)
    _, _, _, counts = G.codec.extract_records(e.held_dev, e.rows, 32, return_counts=True)
    want = LR.decode_list((2 * counts - 16).cpu().numpy(), 4)
    named = [b for b in range(e.B) if results[b].key_id is not None]      # (at this noise the sign statistic need not name every key: no key, no read)
    assert named and all(results[b].key_id == f"key{b % 12}" for b in named)
    for b in range(e.B):
        if b in named:
            _assert_read(reads[b], _row(want, b), f"detect_payloads (signs) image {b}")
        else:
            assert reads[b] is None
    with pytest.raises(ValueError, match="list size"):
        G.detect.detect_payloads(e.held_dev, e.ring, 256, list_size=3)


def test_unwatermarked_latents_give_no_ok_at_any_list_size(G, E2E):
    """a false ok has probability at most L 2^-18 per image at M = 256; none occurs under the committed seed (tests/test_ecc_list_host.py checks it on the CPU)"""
    e = E2E
    blank_score = LR.blank_scores(e.s)
    blank = e.s["blank"]
    thr = np.stack([R.uniform_thresholds32(row) for row in blank])
    vote = G.soft.extract_soft(torch.from_numpy(blank).cuda().view(64, 4, 32, 32), e.s["keys"][0], e.s["nonces"][0], 256, thresholds=torch.from_numpy(thr).cuda())
    assert np.array_equal(vote.score.cpu().numpy(), blank_score)
    for L in LR.LIST_SIZES:
        read = G.ecc.read_list(vote.score, L)
        _assert_read(read, LR.decode_list(blank_score, L), f"blank latents L = {L}")
        assert not any(read.ok) and not any(read.n_ok) and not any(read.rank)
    results, reads = G.detect.detect_payloads(torch.from_numpy(blank[:8]).cuda().view(8, 4, 32, 32), e.ring, 256, reliability=15, list_size=8)
    assert all(r.key_id is None for r in results) and reads == [None] * 8


def _zero_eps(x, t, ctx):
    return torch.zeros_like(x)


def test_verify_records_with_a_list(G, E2E):
    e = E2E
    ctx = torch.zeros(1, 1, 1, device="cuda", dtype=torch.float32)
    pipe = G.pipeline.GaussianShadingPipeline(_zero_eps, e.s["keys"][0], e.s["nonces"][0], R.encode(e.s["payloads"][0], 256), height=256, width=256,
                                              num_inference_steps=10, dtype=torch.float32, ctx_uncond=ctx)
    today = pipe.verify_records(e.held_dev, e.rows, 32, soft=True, ecc="conv")
    res, read = pipe.verify_records(e.held_dev, e.rows, 32, soft=True, ecc="conv", ecc_list=8)
    assert all(torch.equal(a, b) for a, b in zip(res, today[0]))
    _assert_read(read, LR.decode_list(res.score.cpu().numpy(), 8), "verify_records(soft=True, ecc_list=8)")
    res1, read1 = pipe.verify_records(e.held_dev, e.rows, 32, soft=True, ecc="conv", ecc_list=1)
    assert type(read1).__name__ == "EccRead" and read1[:4] == today[1][:4]
    (bits, flags, matches), read = pipe.verify_records(e.held_dev, e.rows, 32, ecc="conv", ecc_list=2)
    _, _, _, counts = G.codec.extract_records(pipe.invert(e.held_dev), e.rows, 32, return_counts=True)
    _assert_read(read, LR.decode_list((2 * counts - 16).cpu().numpy(), 2), "verify_records(ecc_list=2)")
    with pytest.raises(ValueError, match="ecc_list"):
        pipe.verify_records(e.held_dev, e.rows, 32, soft=True, ecc_list=8)
    with pytest.raises(ValueError, match="list size"):
        pipe.verify_records(e.held_dev, e.rows, 32, soft=True, ecc="conv", ecc_list=5)


def test_the_extract_line_carries_the_rank(G, E2E):
    """every decoder of `extract` with --ecc conv --ecc_list 8: the bit string is the vote's, the note the list decode of that vote's own score"""
    e, X = E2E, G.extract
    own = [0, 12]                                                                                            # the images under key 0
    z = e.held_dev[own].contiguous()
    base = dict(key=e.s["keys"][0], nonce=e.s["nonces"][0], message_length=256, l=1, ecc="conv", ecc_list=8, soft_levels=15, soft_clip=2.5, tile=8, iters=2,
                sign_rounds=1)
    for extra in (dict(soft=1), dict(), dict(robust=1), dict(robust_soft=7), dict(window_soft=7, l=2)):
        args = SimpleNamespace(**{**base, **extra})
        out = X.recover_exactracted_message_batch(z, args)
        bits, flags, score = X._vote_scored(z, SimpleNamespace(**{**base, **extra, "ecc": None, "ecc_list": 1}), 256, args.l)
        want = LR.decode_list(score.cpu().numpy(), 8)
        today = X.recover_exactracted_message_batch(z, SimpleNamespace(**{**base, **extra, "ecc_list": 1}))
        plain = R.decode(score.cpu().numpy())
        for i in range(2):
            assert isinstance(out[i], str) and out[i] == today[i], extra
            assert out[i].note == LR.format_read_list(want, i, 256, 8), extra
            assert today[i].note == f"payload {R.payloads(plain['info'], 256)[i].hex()} crc {'ok' if plain['ok'][i] else 'FAILED'}, corrected {plain['flips'][i]} of 256", extra
        if extra == dict(soft=1):
            assert [o.note.split(",")[0] for o in out] == [f"payload {e.s['payloads'][b].hex()} crc ok" for b in own]
            assert all(f", list rank {want['rank'][i]} of 8" in out[i].note for i in range(2))
            one = X.recover_exactracted_message(z[1].cpu().numpy(), args)
            assert one == out[1] and one.note == out[1].note
    with pytest.raises(ValueError, match="--ecc_list"):
        X.recover_exactracted_message_batch(z, SimpleNamespace(**{**base, "ecc": None}))
    with pytest.raises(ValueError, match="--align"):
        X.recover_exactracted_message_batch(z, SimpleNamespace(**{**base, "align": "d4"}))
