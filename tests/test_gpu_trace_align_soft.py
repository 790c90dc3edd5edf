"""GPU: the aligned registry search ranked by reliability levels -- codec.level_counts_align bit for bit against the NumPy restatement of
tests/trace_align_soft_reference.py on poisoned, guard-banded buffers (tests/poison.py), against the device's own soft vote of the aligned latent and against
codec.counts_align, its refusals, the two searches against their restatement (ties and cuts included), then trace_latents_aligned_soft and
trace_latents_keyed_aligned_soft end to end on the two cases of DESIGN.md section 4.26, the tamper map under an alignment, and the front end.  Integers are
compared EXACTLY; the bounds, which are floats computed from equal integers, within 1e-9."""
import math
import os

import numpy as np
import pytest
import torch

import align_reference as AR
import key_search_reference as R
import key_search_soft_reference as KS
import trace_align_reference as TR
import trace_align_soft_reference as TS
from poison import FINITE, NAN, Ledger, poisoned

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gswm_amd  # noqa: F401
    from gswm_amd import align, codec, soft, trace
    assert hasattr(codec, "level_counts_align")
    return codec, align, soft, trace


def _align_list(H, W, A):
    """identity first, then every legal d, with shifts that are zero, negative, >= the lattice's side and far outside it (all taken modulo)"""
    ds = [d for d in range(8) if H == W or not d & 1]
    shifts = [(0, 0), (-1, 2), (H, -W - 1), (H + 3, W + 5), (-2 * H - 1, 0), (0, 3 * W - 1), (1, 1), (-H // 2, W // 2)]
    out = [(0, 0, 0)]
    i = 1
    while len(out) < A:
        out.append((ds[i % len(ds)], *shifts[(i // len(ds) + i) % len(shifts)]))
        i += 1
    return out


def _key(rng):
    return bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8))


def _rows(codec, signs: np.ndarray, lv: np.ndarray, P: int):
    """host sign rows and levels -> a `codec.LevelRows` on the device"""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return codec.LevelRows(dev(signs), dev(KS.planes_of_levels(lv, P)), dev(lv.sum(axis=1).astype(np.int32)), dev((lv * lv).sum(axis=1).astype(np.int32)),
                           torch.zeros(signs.shape[0], dtype=torch.int32).cuda())


# C, H, W, M, P, B, A, levels ("random" or "top"): the smallest case; the byte path on a non-square lattice with an odd H; 425-byte rows (unaligned row starts), odd W,
# the byte path, 250 of 256 lanes; the word path with 224 lanes without a word and 200 alignments; three message words (255 lanes); V = 1 at the longest
# message; V = 32 on one message word (256 lanes on it); 16 alignments per workgroup with a half-full last chunk; three per workgroup with one in the last;
# every level 15 at the largest per-lane count the plan accepts at P = 4, on the word path (16 words per lane) and on the byte path (64 bytes per lane)
CASES = [(1, 8, 8, 8, 1, 1, 1, "random"), (3, 5, 8, 24, 2, 3, 4, "random"), (8, 17, 25, 200, 3, 3, 12, "random"), (4, 16, 16, 64, 4, 17, 200, "random"),
         (4, 12, 12, 96, 2, 3, 8, "random"), (2, 32, 32, 2048, 1, 2, 8, "random"), (4, 16, 16, 32, 4, 2, 8, "random"), (1, 8, 8, 64, 1, 300, 120, "random"),
         (4, 16, 16, 64, 4, 17, 400, "random"), (4, 128, 256, 32, 4, 1, 2, "top"), (4, 128, 256, 8, 4, 1, 2, "top")]


@pytest.mark.parametrize("C,H,W,M,P,B,A,levels", CASES)
def test_level_counts_align_matches_the_restatement(G, C, H, W, M, P, B, A, levels):
    codec = G[0]
    rng = np.random.default_rng(C + 3 * H + 7 * W + 11 * P + 13 * B + A + 17 * M)
    n = C * H * W
    signs = rng.integers(0, 256, (B, n // 8), dtype=np.uint8)
    top = (1 << P) - 1
    lv = np.full((B, n), top, dtype=np.int64) if levels == "top" else rng.integers(0, top + 1, (B, n), dtype=np.int64)
    key, nonce = _key(rng)
    aligns = _align_list(H, W, A)
    assert aligns[0] == (0, 0, 0) and len(aligns) == A
    bias = top * (n // M) + 3
    want_s, want_w = TS.level_counts_align(signs, lv, (C, H, W), aligns, R.keystreams([(key, nonce)], n)[0], M)
    assert want_s.shape == want_w.shape == (B, A, M) and (np.abs(want_s) <= want_w).all() and int(want_w.max()) <= top * (n // M)
    rows = _rows(codec, signs, lv, P)
    table = torch.tensor(aligns, dtype=torch.int32).cuda()
    for name, pattern in (("NAN", NAN), ("FINITE", FINITE)):
        L = Ledger(pattern)
        try:
            with poisoned(L):
                wrapped = codec.LevelRows(*(L.wrap(t) for t in rows))
                score, wsum = codec.level_counts_align(wrapped, (C, H, W), L.wrap(table) if pattern == NAN else aligns, key, nonce, M, bias=bias,
                                                       return_wsum=True)                                     # a device table, a list
                alone = codec.level_counts_align(wrapped, (C, H, W), aligns, key, nonce, M)                    # no wsum, no bias
            torch.cuda.synchronize()
            L.check()
            for out in (score, wsum, alone):
                assert L.untouched(out) == 0, f"never written ({name} run) -- {L.where(out)}"                # (no value is 0x7FFF7FFF or 0x4D4D4D4D)
            got_s, got_w, got_a = score.cpu().numpy(), wsum.cpu().numpy(), alone.cpu().numpy()
        finally:
            L.release()
        assert got_s.dtype == got_w.dtype == np.int32 and got_s.shape == got_w.shape == (B, A, M)
        assert np.array_equal(got_w, want_w), (name, np.argwhere(got_w != want_w)[:5])
        assert np.array_equal(got_s, want_s + bias), (name, np.argwhere(got_s != want_s + bias)[:5])
        assert np.array_equal(got_a, want_s), name


def test_an_entry_without_a_map_writes_the_bias_and_zeros(G):
    """a quarter turn on a non-square lattice and a d outside 0..7 never pass `align_table`; handed to the launch behind its back they write `bias` and zeros, the
    entries between them what they should, and nothing outside the outputs"""
    codec = G[0]
    rng = np.random.default_rng(11)
    C, H, W, M, P = 3, 5, 8, 24, 2
    n = C * H * W
    signs = rng.integers(0, 256, (2, n // 8), dtype=np.uint8)
    lv = rng.integers(0, 4, (2, n), dtype=np.int64)
    key, nonce = _key(rng)
    aligns = [(0, 0, 0), (1, 0, 0), (2, 1, 1), (9, 0, 0), (-1, 2, 2)]
    ok = [0, 2]
    want_s, want_w = TS.level_counts_align(signs, lv, (C, H, W), [aligns[i] for i in ok], R.keystreams([(key, nonce)], n)[0], M)
    rows = _rows(codec, signs, lv, P)
    L = Ledger(NAN)
    try:
        with poisoned(L):
            table = L.wrap(torch.tensor(aligns, dtype=torch.int32).cuda())
            score, wsum = codec._level_counts_align_launch(codec.LevelRows(*(L.wrap(t) for t in rows)), (C, H, W), table, key, nonce, M, 77, True)
        torch.cuda.synchronize()
        L.check()
        assert L.untouched(score) == 0 and L.untouched(wsum) == 0
        score, wsum = score.cpu().numpy(), wsum.cpu().numpy()
    finally:
        L.release()
    assert np.array_equal(score[:, ok], want_s + 77) and np.array_equal(wsum[:, ok], want_w)
    assert (score[:, [1, 3, 4]] == 77).all() and not wsum[:, [1, 3, 4]].any()


def test_level_counts_align_is_the_soft_vote_of_the_aligned_latent(G):
    codec, AL, S, T = G
    key, nonce = _key(np.random.default_rng(1))
    aligns = [(d, 0, 0) for d in range(4)] + [(d, -3, 5) for d in range(4, 8)]
    for dtype in (torch.float16, torch.bfloat16, torch.float32, torch.float64):
        z = torch.randn(3, 4, 16, 16, generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dtype).cuda()
        for thr in (S.uniform_thresholds(z, 15), S.uniform_thresholds(z, 5)[0].contiguous()):               # a table per image at P = 4, one for all at P = 3
            rows = codec.level_pack(z, thr)
            assert int(rows.flags.abs().sum()) == 0
            score, wsum = codec.level_counts_align(rows, (4, 16, 16), aligns, key, nonce, 64, return_wsum=True)
            for i, a in enumerate(aligns):
                vote = S.extract_soft(AL.apply(z, a).contiguous(), key, nonce, 64, thresholds=thr)
                assert torch.equal(score[:, i], vote.score) and torch.equal(wsum[:, i], vote.wsum), (dtype, a)


def test_one_plane_of_ones_is_counts_align(G):
    codec = G[0]
    rng = np.random.default_rng(2)
    key, nonce = _key(rng)
    for (C, H, W), M in (((4, 16, 16), 64), ((3, 5, 8), 24)):
        n = C * H * W
        signs = rng.integers(0, 256, (5, n // 8), dtype=np.uint8)
        rows = _rows(codec, signs, np.ones((5, n), dtype=np.int64), 1)
        aligns = _align_list(H, W, 9)
        score, wsum = codec.level_counts_align(rows, (C, H, W), aligns, key, nonce, M, return_wsum=True)
        counts = codec.counts_align(rows.signs, (C, H, W), 1, aligns, key, nonce, M)
        assert torch.equal(score, 2 * counts - n // M) and bool((wsum == n // M).all())
        assert torch.equal(codec.level_counts_align(rows, (C, H, W), aligns, key, nonce, M, bias=n // M), 2 * counts)


def test_level_counts_align_refuses_before_any_launch(G):
    codec = G[0]
    key, nonce = bytes(32), bytes(16)
    z = lambda *s, dt=torch.uint8: torch.zeros(*s, dtype=dt).cuda()
    rows = lambda B, nb, P=1: codec.LevelRows(z(B, nb), z(B, P, nb), z(B, dt=torch.int32), z(B, dt=torch.int32), z(B, dt=torch.int32))
    ok = rows(2, 8)
    ident = [(0, 0, 0)]
    with pytest.raises(ValueError, match="multiple of 8"):
        codec.level_counts_align(ok, (1, 8, 8), ident, key, nonce, 12)
    with pytest.raises(ValueError, match="multiple of 8"):
        codec.level_counts_align(ok, (1, 8, 8), ident, key, nonce, 2056)
    with pytest.raises(IndexError, match="string index out of range"):
        codec.level_counts_align(ok, (1, 8, 8), ident, key, nonce, 24)
    with pytest.raises(ValueError, match="0..7"):
        codec.level_counts_align(ok, (1, 8, 8), [(8, 0, 0)], key, nonce, 8)
    with pytest.raises(ValueError, match="0..7"):
        codec.level_counts_align(ok, (1, 8, 8), torch.tensor([[0, 0, 0], [-1, 0, 0]], dtype=torch.int32).cuda(), key, nonce, 8)
    with pytest.raises(ValueError, match="square"):
        codec.level_counts_align(rows(2, 8), (1, 4, 16), [(0, 0, 0), (3, 0, 0)], key, nonce, 8)
    with pytest.raises(ValueError, match="whole bytes"):
        codec.level_counts_align(rows(2, 2), (1, 3, 3), ident, key, nonce, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        codec.level_counts_align(codec.LevelRows(*(t.cpu() for t in ok)), (1, 8, 8), ident, key, nonce, 8)
    with pytest.raises(ValueError):
        codec.level_counts_align(ok, (1, 8, 16), ident, key, nonce, 8)                                  # rows of 8 bytes, a lattice of 16
    with pytest.raises(ValueError):
        codec.level_counts_align(ok, (1, 8, 8), ident, key[:31], nonce, 8)
    with pytest.raises(ValueError, match="rows.planes"):
        codec.level_counts_align(ok._replace(planes=z(2, 5, 8)), (1, 8, 8), ident, key, nonce, 8)
    with pytest.raises(ValueError, match="1 \\+ P"):
        codec.level_counts_align(rows(1, 4 * 256 * 256 // 8, 4), (4, 256, 256), ident, key, nonce, 256)
    with pytest.raises(ValueError, match="bytes of LDS"):
        codec.level_counts_align(rows(1, 4 * 256 * 264 // 8, 1), (4, 256, 264), ident, key, nonce, 256)
    with pytest.raises(ValueError, match="int32"):
        codec.level_counts_align(ok, (1, 8, 8), ident, key, nonce, 8, bias=2 ** 31 - 15 * 8)
    with pytest.raises(ValueError, match="bias"):
        codec.level_counts_align(ok, (1, 8, 8), ident, key, nonce, 8, bias=1.5)


# ------------------------------------------------------------------------------------------------------------ the searches
@pytest.fixture(scope="module")
def SEARCH(G):
    """`test_gpu_trace_align.py`'s search case with levels: 4 x 16 x 16, five noise images, 202 alignments of which the last two repeat entries 0 and 100, nine
    records of which rows 2 and 6 are the same; the restatement's scores under the table that the device is given, computed once"""
    codec, AL, S, T = G
    rng = np.random.default_rng(426)
    z = torch.randn(5, 4, 16, 16, generator=torch.Generator().manual_seed(426)).half()
    thr = S.uniform_thresholds(z, 15)
    aligns = AL.alignments("d4", 2, 16, 16)
    assert aligns[100] == (4, 0, 0)
    aligns = aligns + [(0, 16, -16), (4, 0, 16)]
    key, nonce = _key(rng)
    msgs = [bytes(rng.integers(0, 256, 8, dtype=np.uint8)) for _ in range(9)]
    reg = T.Registry(8)
    for u, m in enumerate(msgs):
        reg.add(f"user-{u}", m)
    reg._messages[6] = reg._messages[2]
    reg._device_cache.clear()
    registry = np.stack([np.frombuffer(m, dtype=np.uint8) for m in reg._messages])
    _, Sh, wsq = TS.shared_search(z, thr.numpy(), aligns, R.keystreams([(key, nonce)], 1024)[0], registry)
    records = [(*_key(rng), m) for m in msgs]
    kreg = T.KeyedRegistry(8)
    for u, r in enumerate(records):
        kreg.add(f"user-{u}", *r)
    records[6] = kreg._records[6] = records[2]
    kreg._device_cache.clear()
    return dict(z=z.cuda(), thr=thr.cuda(), aligns=aligns, key=key, nonce=nonce, reg=reg, S=Sh, wsq=wsq, kreg=kreg, KS=TS.keyed_search(z, thr.numpy(), aligns, records)[0])


def _found(results):
    return [[(c.index, c.alignment, c.score) for c in r.candidates] for r in results]


@pytest.mark.parametrize("keyed", [False, True])
@pytest.mark.parametrize("k", [1, 3])
def test_the_searches_match_the_restatement(G, SEARCH, keyed, k):
    codec, AL, S, T = G
    Sc = SEARCH["KS" if keyed else "S"]
    aligns = SEARCH["aligns"]
    A = len(aligns)
    rec, al, sc = TS.merge(Sc, k)
    assert np.array_equal(Sc[:, :, 2], Sc[:, :, 6]) and np.array_equal(Sc[:, 0], Sc[:, 200]) and np.array_equal(Sc[:, 100], Sc[:, 201])       # the forced ties
    for order in rec.tolist():                                                       # row 6 never comes before row 2, a repeated alignment never wins
        assert 6 not in order or (2 in order and order.index(2) < order.index(6))
    assert (al < 200).all()
    want = [[(int(rec[b, j]), aligns[int(al[b, j])], int(sc[b, j])) for j in range(k)] for b in range(5)]
    per_image = 5 * 128 if keyed else 4 * 64                                         # bytes of one aligned image: its sign row and four planes, or its 64 scores
    name = "trace_keyed_soft_topk" if keyed else "trace_topk"
    rows_of = (lambda a: a[0].signs.shape[0]) if keyed else (lambda a: a[0].shape[0])
    for budget, launches in ((None, 1), (2 * A * per_image, 3), (70 * per_image, 15)):     # one chunk; three chunks of images; the alignments of ONE image cut in three
        calls = []
        real = getattr(codec, name)
        setattr(codec, name, lambda *a, **kw: (calls.append(rows_of(a)), real(*a, **kw))[1])
        try:
            if keyed:
                got = T.trace_latents_keyed_aligned_soft(SEARCH["z"], SEARCH["kreg"], aligns, thresholds=SEARCH["thr"], k=k, budget_bytes=budget)
            else:
                got = T.trace_latents_aligned_soft(SEARCH["z"], SEARCH["key"], SEARCH["nonce"], SEARCH["reg"], aligns, thresholds=SEARCH["thr"], k=k,
                                                   budget_bytes=budget)
        finally:
            setattr(codec, name, real)
        assert len(calls) == launches and sum(calls) == 5 * A, (budget, calls)
        assert _found(got) == want, (budget, _found(got), want)
        for b, r in enumerate(got):
            assert r.attributed is None and r.alignment is None                     # noise names nobody
            assert all(c.log10_p_any == T.log10_p_any(S.log10_p(c.score, int(SEARCH["wsq"][b])), 9 * A) for c in r.candidates)


# ------------------------------------------------------------------------------------------------------------ end to end, one key
@pytest.fixture(scope="module")
def E2E(G):
    codec, AL, S, T = G
    E = TS.SHARED
    s = TS.shared_setup()
    cands = AL.alignments("d4", E["shift"], E["shape"][1], E["shape"][2])
    assert len(cands) == 200
    reg = T.Registry(E["msg_bytes"])
    for u, m in enumerate(s["registry"]):
        reg.add(f"user-{u}", bytes(m))
    thr = S.uniform_thresholds(s["held"], E["levels"])                           # AFTER the latents are held; the device is given this very table
    score, Sl, wsq = TS.shared_search(s["held"], thr.numpy(), cands, s["ks"], s["registry"])
    host = TS.trace_host(Sl, wsq, S.log10_p, T.log10_p_any)
    return dict(s, cands=cands, reg=reg, thr=thr, score=score, S=Sl, wsq=wsq, host=host, n=int(np.prod(E["shape"])))


def _close(a, b):
    return abs(a - b) <= 1e-9


def test_trace_latents_aligned_soft_names_six_where_the_signs_name_fewer(G, E2E):
    codec, AL, S, T = G
    E = TS.SHARED
    limit = math.log10(E["fpr"])
    M, host, cands = 8 * E["msg_bytes"], E2E["host"], E2E["cands"]
    print("levels, log10 p over U A pairs:", [round(h[3], 1) for h in host])
    assert [h[0] for h in host] == list(E["rows"]) and all(h[3] <= limit for h in host)               # the restatement alone meets the case
    z = E2E["held"].cuda()
    dev = T.trace_latents_aligned_soft(z, E2E["key"], E2E["nonce"], E2E["reg"], cands, thresholds=E2E["thr"].cuda(), fpr=E["fpr"])
    for b, (d, h) in enumerate(zip(dev, host)):
        top = d.candidates[0]
        assert d.attributed == f"user-{E['rows'][b]}" == top.user_id and len(d.candidates) == 1
        assert (top.index, top.score) == (h[0], h[2]) and _close(top.log10_p_any, h[3]) and top.log10_p_any <= limit
        assert d.alignment == top.alignment == cands[h[1]] == AL.inverse(E["attacks"][b], 32, 32)
        assert torch.equal(AL.apply(torch.from_numpy(E2E["attacked"][b]), d.alignment), torch.from_numpy(E2E["clean"][b]))
        voted = (E2E["score"][b, h[1]] > 0).astype(np.uint8)                                            # the soft vote of the aligned latent
        assert top.agree == int((voted == np.unpackbits(E2E["registry"][h[0]])).sum()) and top.agree > 32
        assert T.format_line("x.png", d, M).endswith(f", alignment: {AL.describe(d.alignment)}")
    # the table the tracer takes by itself (the same rule, evaluated on the device) names the same six with the same alignments
    own = T.trace_latents_aligned_soft(z, E2E["key"], E2E["nonce"], E2E["reg"], cands, fpr=E["fpr"])
    assert [(d.attributed, d.alignment) for d in own] == [(d.attributed, d.alignment) for d in dev]
    # k = 3: the runners-up are other records, each with its own best alignment, none significant
    more = T.trace_latents_aligned_soft(z, E2E["key"], E2E["nonce"], E2E["reg"], cands, thresholds=E2E["thr"].cuda(), k=3, fpr=E["fpr"])
    rec, al, sc = TS.merge(E2E["S"], 3)
    for b, (d, one) in enumerate(zip(more, dev)):
        assert d.candidates[0] == one.candidates[0] and [(c.index, c.alignment, c.score) for c in d.candidates] == \
            [(int(rec[b, j]), cands[int(al[b, j])], int(sc[b, j])) for j in range(3)]
        assert all(c.log10_p_any > limit for c in d.candidates[1:])
    # the sign tracer on the same latents names fewer
    sign = T.trace_latents_aligned(z, E2E["key"], E2E["nonce"], E2E["reg"], cands, fpr=E["fpr"])
    print("signs, log10 p over U A pairs:", [round(r.candidates[0].log10_p_any, 1) for r in sign])
    assert sum(r.attributed == f"user-{E['rows'][b]}" for b, r in enumerate(sign)) < 6


def test_unwatermarked_latents_name_nobody_and_flagged_ones_raise(G, E2E):
    codec, AL, S, T = G
    E = TS.SHARED
    cands = E2E["cands"]
    thb = S.uniform_thresholds(E2E["held_blank"], E["levels"])
    _, Sb, wb = TS.shared_search(E2E["held_blank"], thb.numpy(), cands, E2E["ks"], E2E["registry"])
    host = TS.trace_host(Sb, wb, S.log10_p, T.log10_p_any)
    assert all(h[3] == 0.0 for h in host)                                                              # the restatement alone meets the case
    z = E2E["held_blank"].clone()
    z[3, 0, 0, 0] = float("nan")
    dev = T.trace_latents_aligned_soft(z.cuda(), E2E["key"], E2E["nonce"], E2E["reg"], cands, thresholds=thb.cuda(), fpr=E["fpr"], tamper_tile=8)
    for d, h in zip(dev[:3], host):
        top = d.candidates[0]
        assert d.attributed is None and d.alignment is None and d.tamper is None
        assert (top.index, top.alignment, top.score, top.log10_p_any) == (h[0], cands[h[1]], h[2], 0.0)
    assert isinstance(dev[3], ValueError) and "NaN" in str(dev[3])
    # the six noisy latents as they are, saturated elements and all: the reference's error for every one of them
    out = T.trace_latents_aligned_soft(E2E["z16"].cuda(), E2E["key"], E2E["nonce"], E2E["reg"], cands)
    assert len(out) == 6 and all(isinstance(r, ValueError) and "invalid literal for int() with base 2" in str(r) for r in out)
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        T.trace_latents_aligned_soft(E2E["held_blank"].view(4, -1).cuda(), E2E["key"], E2E["nonce"], E2E["reg"], cands)
    with pytest.raises(ValueError, match="square"):
        T.trace_latents_aligned_soft(torch.zeros(1, 4, 16, 32).half().cuda(), E2E["key"], E2E["nonce"], E2E["reg"], cands)
    with pytest.raises(ValueError, match="levels"):
        T.trace_latents_aligned_soft(E2E["held_blank"].cuda(), E2E["key"], E2E["nonce"], E2E["reg"], cands, levels=16)
    with pytest.raises(ValueError, match="1 \\+ P"):                                                   # 262 144 elements with four planes
        T.trace_latents_aligned_soft(torch.zeros(1, 4, 256, 256).half().cuda(), E2E["key"], E2E["nonce"], E2E["reg"], [(0, 0, 0)])
    with pytest.raises(ValueError, match="bytes of LDS"):                                              # one plane: inside the search's domain, past the kernel's LDS
        T.trace_latents_aligned_soft(torch.zeros(1, 4, 256, 264).half().cuda(), E2E["key"], E2E["nonce"], E2E["reg"], [(0, 0, 0)], levels=1)


# ------------------------------------------------------------------------------------------------------------ end to end, a key per record
def test_trace_latents_keyed_aligned_soft_names_six_where_the_signs_name_fewer(G):
    codec, AL, S, T = G
    E = TS.KEYED
    limit = math.log10(E["fpr"])
    s = TS.keyed_setup()
    cands = AL.alignments("d4", E["shift"], E["shape"][1], E["shape"][2])
    thr = S.uniform_thresholds(s["held"], E["levels"])
    Sl, wsq = TS.keyed_search(s["held"], thr.numpy(), cands, s["records"])
    host = TS.trace_host(Sl, wsq, S.log10_p, T.log10_p_any)
    print("keyed levels, log10 p over U A pairs:", [round(h[3], 1) for h in host])
    assert [h[0] for h in host] == list(s["rows"]) and all(h[3] <= limit for h in host)               # the restatement alone meets the case
    assert [cands[h[1]] for h in host] == [AL.inverse(a, 32, 32) for a in E["attacks"]]
    reg = T.KeyedRegistry(E["msg_bytes"])
    for u, r in enumerate(s["records"]):
        reg.add(f"user-{u}", *r)
    z = s["held"].cuda()
    dev = T.trace_latents_keyed_aligned_soft(z, reg, cands, thresholds=thr.cuda(), fpr=E["fpr"])
    signs, lv = TS.ASR.rows_of(s["held"], thr.numpy())
    for b, (d, h) in enumerate(zip(dev, host)):
        top = d.candidates[0]
        assert d.attributed == f"user-{s['rows'][b]}" and (top.index, top.score) == (h[0], h[2]) and _close(top.log10_p_any, h[3])
        assert d.alignment == top.alignment == cands[h[1]]
        assert torch.equal(AL.apply(torch.from_numpy(s["attacked"][b]), d.alignment), torch.from_numpy(s["clean"][b]))
        key, nonce, msg = s["records"][h[0]]
        s_al, w_al = TS.aligned_rows(signs[b:b + 1], lv[b:b + 1], E["shape"], [cands[h[1]]])
        voted = KS.voted_message(s_al[0, 0], w_al[0, 0], R.keystreams([(key, nonce)], 4096)[0], E["msg_bytes"])
        assert top.agree == 64 - int(np.unpackbits(np.frombuffer(voted, dtype=np.uint8) ^ np.frombuffer(msg, dtype=np.uint8)).sum()) and top.agree > 32
    sign = T.trace_latents_keyed_aligned(z, reg, cands, fpr=E["fpr"])
    print("keyed signs, log10 p over U A pairs:", [round(r.candidates[0].log10_p_any, 1) for r in sign])
    assert sum(r.attributed == f"user-{s['rows'][b]}" for b, r in enumerate(sign)) < 6
    blank = T.trace_latents_keyed_aligned_soft(s["held_blank"].cuda(), reg, cands, fpr=E["fpr"])
    assert all(r.attributed is None and r.alignment is None and r.candidates[0].log10_p_any == 0.0 for r in blank)
    raw = T.trace_latents_keyed_aligned_soft(s["z16"].cuda(), reg, cands)
    assert len(raw) == 6 and all(isinstance(r, ValueError) and "invalid literal for int() with base 2" in str(r) for r in raw)
    with pytest.raises(ValueError, match="1 \\+ P"):
        T.trace_latents_keyed_aligned_soft(torch.zeros(1, 4, 256, 256).half().cuda(), reg, [(0, 0, 0)])


# ------------------------------------------------------------------------------------------------------------ where, under an alignment
@pytest.mark.parametrize("keyed", [False, True])
def test_tamper_map_under_an_alignment(G, E2E, keyed):
    """The top 16 of the 32 lattice rows of image 1 are replaced by noise, THEN the image is mirrored: the level-weighted tracers still attribute it, and its map
    -- in the coordinates of the lattice as embedded -- marks intact tiles in the surviving lower half only and equals the map of the restatement's counts"""
    codec, AL, S, T = G
    from gswm_amd import tamper as TM
    E = TS.SHARED
    cands = E2E["cands"]
    z = torch.from_numpy(E2E["clean"][1]).clone()
    z[:, :16, :] = torch.randn(4, 16, 32, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    z16 = AL.apply(z, (4, 0, 0)).half()[None].contiguous()
    row = E["rows"][1]
    if keyed:
        reg = T.KeyedRegistry(E["msg_bytes"])
        reg.add("someone", bytes(range(32)), bytes(range(16)), bytes(8))
        reg.add("issuer", E2E["key"], E2E["nonce"], bytes(E2E["registry"][row]))
        (r,) = T.trace_latents_keyed_aligned_soft(z16.cuda(), reg, cands, fpr=E["fpr"], tamper_tile=8)
        assert r.attributed == "issuer"
    else:
        (r,) = T.trace_latents_aligned_soft(z16.cuda(), E2E["key"], E2E["nonce"], E2E["reg"], cands, fpr=E["fpr"], tamper_tile=8)
        assert r.attributed == f"user-{row}"
    assert r.alignment == (4, 0, 0) and r.tamper is not None and r.tamper.source == "registry"
    rows = R.sign_rows(z16.reshape(1, -1).double().numpy())
    back = AR.rows_align(rows, E["shape"], 1, [r.alignment])[0, 0]
    cw = E2E["ks"] ^ np.resize(E2E["registry"][row], E2E["n"] // 8)
    agree = TR.tile_agree(back, cw, E["shape"], 8)
    want = TM.make_map(agree, 4 * 64, 8, E["fpr"], "registry")
    assert np.array_equal(r.tamper.agree, agree) and np.array_equal(r.tamper.intact, want.intact)
    assert not r.tamper.intact[:2].any() and r.tamper.intact[2:].all()                                 # only the surviving half, and all of it (no noise was added)
    assert f", intact tiles 8/16, alignment: {AL.describe((4, 0, 0))}" in T.format_line("x.png", r, 64)


# ------------------------------------------------------------------------------------------------------------ front end
@pytest.mark.parametrize("keyed", [False, True])
def test_cli_with_align_reliability(G, E2E, keyed, tmp_path, monkeypatch, capsys):
    """The front end with --align d4 --align_shift 2 --align_reliability 15 on two generated files.  As in test_gpu_trace_align.py the inversion is replaced by
    latents (the mirrored image and an unwatermarked one) and no model is built; registry, candidates, search, trace.txt and the maps are the real run."""
    from PIL import Image
    from gswm_amd import extract as X
    codec, AL, S, T = G
    E = TS.SHARED
    d = tmp_path / "imgs"
    d.mkdir()
    rng = np.random.RandomState(5)
    for i in range(2):
        Image.fromarray(rng.randint(0, 256, (64, 64, 3), dtype=np.uint8)).save(str(d / f"img{i}.png"))
    mirrored = AL.apply(torch.from_numpy(E2E["clean"][1]), (4, 0, 0)).half()[None]
    latents = torch.cat([mirrored, E2E["blank"][:1]]).cuda()
    monkeypatch.setattr(X, "invert_decoded_images", lambda arrs, args, **kw: latents[:len(arrs)].clone())
    monkeypatch.setattr(X, "load_models", lambda *a, **kw: None)               # (nothing is inverted: building the synthetic UNet would be most of the test's time)
    reg_file = tmp_path / "registry.tsv"
    if keyed:
        reg = T.KeyedRegistry(E["msg_bytes"])
        for u in range(20):
            reg.add(f"user-{u}", E2E["key"] if u % 2 else bytes([u]) * 32, E2E["nonce"], bytes(E2E["registry"][E["rows"][1] - 7 + u]))
        extra = ["--per_record_keys"]
    else:
        reg = E2E["reg"]
        extra = ["--key_hex", E2E["key"].hex(), "--nonce_hex", E2E["nonce"].hex()]
    reg.save(reg_file)
    maps = tmp_path / "maps"
    T.main(["--images_directory_path", str(d), "--registry", str(reg_file), "--allow_synthetic_weights", "--num_inference_steps", "2", "--width", "256",
            "--height", "256", "--strict_kernels", "0", "--align", "d4", "--align_shift", "2", "--align_reliability", "15", "--top", "2",
            "--tamper_map", str(maps)] + extra)
    out = capsys.readouterr().out
    lines = (d / "trace.txt").read_text().splitlines()
    start = lines.index("=" * 40 + "Batch Start" + "=" * 40)
    info = dict(l.split(",", 1) for l in lines[1:start])
    assert info["statistic"] == "soft, 15 reliability levels over 200 alignments" and info["alignments"] == "200" and info["users"] == str(len(reg))
    body = lines[start + 2:-1]
    files = X._DirJob(str(d)).files
    assert len(body) == len(files) == 2
    cands = AL.alignments("d4", 2, 32, 32)
    if keyed:
        want = T.trace_latents_keyed_aligned_soft(latents, reg, cands, levels=15, k=2, tamper_tile=8)
    else:
        want = T.trace_latents_aligned_soft(latents, E2E["key"], E2E["nonce"], reg, cands, levels=15, k=2, tamper_tile=8)
    for f, line, w in zip(files, body, want):
        assert line == T.format_line(os.path.basename(f), w, 64) and line in out
    user = "user-7" if keyed else f"user-{E['rows'][1]}"
    assert body[0].startswith(f"{os.path.basename(files[0])}, user: {user}, agreement, 1.0, log10 p, -") and body[0].endswith(", intact tiles 16/16, alignment: hflip")
    assert body[1].startswith(f"{os.path.basename(files[1])}, user: none, ") and "alignment" not in body[1]
    stem = os.path.splitext(os.path.basename(files[0]))[0]
    assert sorted(os.listdir(maps)) == [f"{stem}.tamper.npy", f"{stem}.tamper.png"]                    # the attributed image alone has a map
    for bad in (["--align_reliability", "15"], ["--align", "d4", "--align_reliability", "15", "--hard"], ["--align", "d4", "--align_reliability", "15", "--l", "2"]):
        if keyed and "--hard" in bad:
            continue
        with pytest.raises(SystemExit):
            T.main(["--images_directory_path", str(d), "--registry", str(reg_file)] + bad + extra)
