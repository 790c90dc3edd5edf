"""GPU: pooled evidence across the images of a set -- codec.pool_rows and codec.trace_keyed_pooled_topk against the NumPy restatement
of tests/pool_reference.py on poisoned, guard-banded buffers, the two exact identities with the per-image searches, then trace.trace_sets_keyed / trace_sets
end to end and the front end.  EXACT equality of bytes, sums, indices and scores everywhere; the bounds match to 1e-9 decades."""
import math
import os

import numpy as np
import pytest
import torch

import pool_reference as PR
from poison import FINITE, NAN, Ledger, poisoned
from test_gpu_trace_keyed import _records_and_codewords, _rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gswm_amd  # noqa: F401
    from gswm_amd import codec, soft, trace
    return codec, soft, trace


def _planes_of(lv, P):
    return np.stack([np.packbits(((lv >> k) & 1).astype(np.uint8), axis=1) for k in range(P)], axis=1)


def _random_images(rng, B, nbytes, P):
    """sign rows and (P > 0) levels 0 .. 2^P - 1 as planes, made on the host"""
    signs = rng.integers(0, 256, (B, nbytes), dtype=np.uint8)
    if not P:
        return signs, None
    return signs, _planes_of(rng.integers(0, 2 ** P, (B, nbytes * 8), dtype=np.int64), P)


def _sets_of(sizes):
    edges = np.concatenate([[0], np.cumsum(sizes)])
    return [list(range(edges[i], edges[i + 1])) for i in range(len(sizes))]


def _assert_pooled(got, want, where):
    assert got.signs.dtype == torch.uint8 and got.planes.dtype == torch.uint8 and got.wsum.dtype == torch.int32 and got.wsq.dtype == torch.int64, where
    assert got.planes.shape[1] == want["Q"], where
    assert np.array_equal(got.signs.cpu().numpy(), want["signs"]), where
    assert np.array_equal(got.planes.cpu().numpy(), want["planes"]), where
    assert got.wsum.cpu().tolist() == want["wsum"].tolist() and got.wsq.cpu().tolist() == want["wsq"].tolist(), where


# ------------------------------------------------------------------------------------------------------------ pool_rows
# row bytes x P x set sizes: 1-byte rows without planes; 15-byte rows (no whole dword) at P = 2; 32-byte rows at P = 4 with 68 images (Q = 10, the top);
# 8-byte rows with 1023 images (Q = 10 at unit levels); a row of three workgroup steps (2052 bytes: 513 words) with every P in between
POOL_CASES = [(1, 0, (1, 3)), (15, 2, (1, 2, 5)), (32, 4, (68,)), (8, 0, (1023,)), (2052, 3, (2, 1)), (2052, 1, (7,)), (64, 4, (3, 68, 1))]


@pytest.mark.parametrize("nbytes,P,sizes", POOL_CASES)
@pytest.mark.parametrize("pattern", [NAN, FINITE])
def test_pool_rows_matches_the_restatement_on_poisoned_buffers(G, nbytes, P, sizes, pattern):
    codec, S, T = G
    rng = np.random.default_rng(nbytes * 31 + P * 7 + sum(sizes))
    signs, planes = _random_images(rng, sum(sizes), nbytes, P)
    want = PR.pool_rows(signs, planes, _sets_of(sizes))
    led = Ledger(pattern)
    with poisoned(led):
        got = codec.pool_rows(led.wrap(torch.from_numpy(signs).cuda()), led.wrap(torch.from_numpy(planes).cuda()) if P else None, sizes)
    led.check()
    _assert_pooled(got, want, (nbytes, P, sizes))


def test_pool_rows_writes_every_output_byte(G):
    """constant rows under the pattern whose bytes no result takes: zeros pool to sign 0x00 and planes of 0x00 / 0xFF, never 0x4D"""
    codec, S, T = G
    for nbytes, P, sizes in ((15, 2, (2, 5)), (2052, 0, (3,)), (1, 0, (1, 1)), (64, 4, (68,))):
        B = sum(sizes)
        signs = np.zeros((B, nbytes), dtype=np.uint8)
        planes = np.full((B, P, nbytes), 0xFF, dtype=np.uint8) if P else None
        led = Ledger(FINITE)
        with poisoned(led):
            got = codec.pool_rows(torch.from_numpy(signs).cuda(), torch.from_numpy(planes).cuda() if P else None, sizes)
        led.check()
        assert all(led.untouched(t) == 0 for t in got), [led.where(t) for t in got if led.untouched(t)]
        _assert_pooled(got, PR.pool_rows(signs, planes, _sets_of(sizes)), (nbytes, P, sizes))


@pytest.mark.parametrize("shift", [1, 3])
def test_pool_rows_through_the_c_abi_at_odd_base_pointers(G, shift):
    """15-byte rows, P = 2, sets of 1, 2 and 5: every row pointer sits `shift` bytes past a 4-byte boundary, so the kernel reads and writes byte by byte"""
    from gswm_amd import _native as N
    codec, S, T = G
    nbytes, P, sizes = 15, 2, (1, 2, 5)
    B, Gs = sum(sizes), len(sizes)
    rng = np.random.default_rng(shift)
    signs, planes = _random_images(rng, B, nbytes, P)
    want = PR.pool_rows(signs, planes, _sets_of(sizes))
    Q = want["Q"]
    led = Ledger(NAN)

    def shifted(nbytes_total, src=None):
        buf = led.empty((nbytes_total + 8,), torch.uint8, "cuda")
        view = buf[shift:shift + nbytes_total]
        if src is not None:
            view.copy_(torch.from_numpy(src.reshape(-1)).cuda())
        assert view.data_ptr() % 4 == shift
        return buf, view

    _, s_dev = shifted(B * nbytes, signs)
    _, p_dev = shifted(B * P * nbytes, planes)
    os_buf, os_dev = shifted(Gs * nbytes)
    op_buf, op_dev = shifted(Gs * Q * nbytes)
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).cuda()
    wsum, wsq = led.empty((Gs,), torch.int32, "cuda"), led.empty((Gs,), torch.int64, "cuda")
    stream = torch.cuda.current_stream().cuda_stream
    rc = N.lib().gsw_pool_rows(s_dev.data_ptr(), p_dev.data_ptr(), P, B, nbytes * 8, ptr.data_ptr(), Gs, max(sizes), Q, os_dev.data_ptr(), op_dev.data_ptr(),
                               wsum.data_ptr(), wsq.data_ptr(), stream)
    assert rc == N.GSW_OK
    torch.cuda.synchronize()
    led.check()
    assert np.array_equal(os_dev.cpu().numpy().reshape(Gs, nbytes), want["signs"]) and np.array_equal(op_dev.cpu().numpy().reshape(Gs, Q, nbytes), want["planes"])
    assert wsum.cpu().tolist() == want["wsum"].tolist() and wsq.cpu().tolist() == want["wsq"].tolist()
    # the bytes around the shifted outputs still hold the pattern
    for buf, size in ((os_buf, Gs * nbytes), (op_buf, Gs * Q * nbytes)):
        assert led.untouched(buf[:shift]) == shift and led.untouched(buf[shift + size:]) == 8 - shift


def test_opposite_images_cancel_and_sets_beyond_the_planes_are_refused(G):
    codec, S, T = G
    rng = np.random.default_rng(11)
    signs, planes = _random_images(rng, 1, 32, 3)
    lv = PR.levels_of_planes(planes, 1, 256)
    flip = np.zeros(256, dtype=np.uint8)
    flip[[0, 7, 8, 100, 255]] = 1                                              # chosen positions: the second image has the opposite sign there, equal levels
    lv[0, [0, 7, 8, 100, 255]] = [7, 1, 3, 5, 7]
    planes = _planes_of(lv, 3)
    two_s = np.concatenate([signs, signs ^ np.packbits(flip)[None]])
    got = codec.pool_rows(torch.from_numpy(two_s).cuda(), torch.from_numpy(np.concatenate([planes, planes])).cuda(), [2])
    want = PR.pool_rows(two_s, np.concatenate([planes, planes]), [[0, 1]])
    _assert_pooled(got, want, "cancel")
    assert not want["S"][0, [0, 7, 8, 100, 255]].any()
    out_bits = np.unpackbits(got.signs.cpu().numpy(), axis=1)[0]
    out_lv = PR.levels_of_planes(got.planes.cpu().numpy(), 1, 256)[0]
    assert not out_bits[[0, 7, 8, 100, 255]].any() and not out_lv[[0, 7, 8, 100, 255]].any()
    # 69 images at 15 levels and 1024 at unit levels: refused by name before a launch, by the wrapper and by the C entry point
    with pytest.raises(ValueError, match="68 images"):
        codec.pool_rows(torch.zeros(69, 32, dtype=torch.uint8).cuda(), torch.zeros(69, 4, 32, dtype=torch.uint8).cuda(), [69])
    with pytest.raises(ValueError, match="1023 images"):
        codec.pool_rows(torch.zeros(1024, 8, dtype=torch.uint8).cuda(), None, [1024])
    with pytest.raises(ValueError, match="set_sizes"):
        codec.pool_rows(torch.zeros(4, 8, dtype=torch.uint8).cuda(), None, [2, 1])
    with pytest.raises(ValueError, match="set_sizes"):
        codec.pool_rows(torch.zeros(4, 8, dtype=torch.uint8).cuda(), None, [4, 0])


def test_one_image_at_the_top_of_the_domain(G):
    """524 288 bits, Q = 1: the pooled row is the image (signs where the level is 1), and the search takes it"""
    codec, S, T = G
    rng = np.random.default_rng(5)
    n = 524288
    signs = rng.integers(0, 256, (1, n // 8), dtype=np.uint8)
    got = codec.pool_rows(torch.from_numpy(signs).cuda(), None, [1])
    assert got.planes.shape == (1, 1, n // 8) and np.array_equal(got.signs.cpu().numpy(), signs) and bool((got.planes == 0xFF).all())
    assert got.wsum.tolist() == [n] and got.wsq.tolist() == [n]
    recs, cw = _records_and_codewords(rng, 5, n, 32)
    idx, score = codec.trace_keyed_pooled_topk(got, n, _rows(T, recs, 32).to_device(), 32, k=4)
    sign_idx, sign_score = codec.trace_keyed_topk(got.signs, n, _rows(T, recs, 32).to_device(), 32, k=4)
    assert torch.equal(idx, sign_idx) and torch.equal(score, sign_score)
    with pytest.raises(ValueError, match="domain"):
        codec.pool_rows(torch.zeros(2, n // 8, dtype=torch.uint8).cuda(), None, [2])


# ------------------------------------------------------------------------------------------------------------ the pooled search
def _pooled_rows(rng, Gs, n, Q, cw, U):
    """pooled rows made on the host (the search alone): set 0 carries no weight, the last set the top level everywhere, set 1 (G > 2) the codeword of
    record U // 2 with one element flipped at the top level"""
    top = 2 ** Q - 1
    signs = rng.integers(0, 256, (Gs, n // 8), dtype=np.uint8)
    lv = rng.integers(0, top + 1, (Gs, n), dtype=np.int64)
    lv[0] = 0
    if Gs > 1:
        lv[-1] = top
    if Gs > 2:
        j = int(rng.integers(0, n))
        signs[1] = cw[U // 2]
        signs[1, j >> 3] ^= 0x80 >> (j & 7)
        lv[1, j] = top
    return signs, _planes_of(lv, Q), lv.sum(axis=1).astype(np.int32)


# U x n x msg_bytes x G x k x Q: n = 1920 has a ragged last ChaCha block; U = 37 and 1000 carry two identical records; every tile (G = 1, 3, 5, 17) and both
# message forms; Q on both sides of the soft search's four planes and at the top
SEARCH_CASES = [(5, 256, 4, 1, 8, 1), (5, 256, 32, 3, 3, 10), (37, 256, 8, 5, 8, 5), (37, 1920, 5, 17, 3, 4), (1000, 1920, 8, 3, 1, 10), (1000, 256, 32, 17, 8, 7),
                (37, 1920, 5, 1, 1, 9), (5, 1920, 4, 5, 3, 2), (1000, 1920, 5, 5, 8, 6), (37, 256, 4, 17, 1, 3)]


@pytest.mark.parametrize("U,n,msg_bytes,Gs,k,Q", SEARCH_CASES)
def test_pooled_search_matches_the_restatement(G, U, n, msg_bytes, Gs, k, Q):
    codec, S, T = G
    rng = np.random.default_rng(U * 7 + n + msg_bytes + Gs + Q)
    recs, cw = _records_and_codewords(rng, U, n, msg_bytes)
    if U >= 37:                                                                # two identical records: the lower index comes first
        recs[U - 2] = recs[3]
        cw[U - 2] = cw[3]
    signs, planes, wsum = _pooled_rows(rng, Gs, n, Q, cw, U)
    if U >= 37 and Gs > 2:
        signs[2] = cw[3]                                                       # set 2 matches the twins best
    reg = torch.from_numpy(np.stack([np.frombuffer((key + nonce + msg).ljust(codec.keyed_record_stride(msg_bytes), b"\0"), dtype=np.uint8)
                                     for key, nonce, msg in recs])).cuda()
    want_idx, want_score = PR.topk(PR.scores(PR.sums_of_rows(signs, planes, wsum), cw), k)
    led = Ledger(NAN)
    with poisoned(led):
        rows = codec.PooledRows(led.wrap(torch.from_numpy(signs).cuda()), led.wrap(torch.from_numpy(planes).cuda()), torch.from_numpy(wsum).cuda(),
                                torch.zeros(Gs, dtype=torch.int64).cuda())
        idx, score = codec.trace_keyed_pooled_topk(rows, n, reg, msg_bytes, k=k)
    led.check()
    got_idx, got_score = idx.cpu().numpy(), score.cpu().numpy()
    assert got_idx.dtype == np.int32 and got_score.dtype == np.int32 and got_idx.shape == (Gs, k)
    assert np.array_equal(got_score, want_score), (np.argwhere(got_score != want_score)[:5], got_score[:2], want_score[:2])
    assert np.array_equal(got_idx, want_idx), (np.argwhere(got_idx != want_idx)[:5], got_idx[:2], want_idx[:2])
    assert (got_score[0][got_idx[0] >= 0] == 0).all()                          # set 0 carries no weight
    if U >= 37 and Gs > 2 and k >= 3:
        assert got_idx[2, 0] == 3 and got_idx[2, 1] == U - 2 and got_score[2, 0] == got_score[2, 1]
    if U < k:
        assert (got_idx[:, U:] == -1).all() and (got_score[:, U:] == -2 ** 31).all()


def test_with_at_most_four_planes_it_is_the_soft_search(G):
    codec, S, T = G
    rng = np.random.default_rng(21)
    n, mb, U = 1920, 5, 300
    recs, cw = _records_and_codewords(rng, U, n, mb)
    reg = _rows(T, recs, mb).to_device()
    for Q, Gs in ((1, 1), (2, 3), (3, 5), (4, 17)):
        signs, planes, wsum = _pooled_rows(rng, Gs, n, Q, cw, U)
        dev = [torch.from_numpy(a).cuda() for a in (signs, planes, wsum)]
        zero = torch.zeros(Gs, dtype=torch.int32).cuda()
        soft_idx, soft_score = codec.trace_keyed_soft_topk(codec.LevelRows(*dev, zero, zero), n, reg, mb, k=8)
        idx, score = codec.trace_keyed_pooled_topk(codec.PooledRows(*dev, zero.long()), n, reg, mb, k=8)
        assert torch.equal(idx, soft_idx) and torch.equal(score, soft_score), Q


def test_pooled_scores_are_the_sums_of_the_per_image_scores(G):
    """U = 8, k = 8: every record is reported, so the per-image scores of the sign search can be summed set by set"""
    codec, S, T = G
    rng = np.random.default_rng(22)
    n, mb, U = 1920, 8, 8
    recs, cw = _records_and_codewords(rng, U, n, mb)
    reg = _rows(T, recs, mb).to_device()
    sizes = (1, 4, 9)
    signs = torch.from_numpy(rng.integers(0, 256, (sum(sizes), n // 8), dtype=np.uint8)).cuda()
    idx1, score1 = codec.trace_keyed_topk(signs, n, reg, mb, k=8)
    per_image = torch.zeros(sum(sizes), U, dtype=torch.int64, device="cuda").scatter_(1, idx1.long(), score1.long())
    idx, score = codec.trace_keyed_pooled_topk(codec.pool_rows(signs, None, sizes), n, reg, mb, k=8)
    pooled = torch.zeros(len(sizes), U, dtype=torch.int64, device="cuda").scatter_(1, idx.long(), score.long())
    for g, members in enumerate(_sets_of(sizes)):
        assert torch.equal(pooled[g], per_image[members].sum(dim=0)), g


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def E2E(G):
    """16 images of 4 x 32 x 32 from codec.embed_records under one record among 1000, 16 more under two records (8 + 8), 16 unwatermarked; the noise of
    tests/pool_reference.py added on the host, so that the device and the restatement see the same float32 latents.  The restatement is computed once."""
    codec, S, T = G
    E = PR.E2E
    B = E["B"]
    recs, cw, u, noise = PR.e2e_setup()
    reg = _rows(T, recs, E["msg_bytes"])
    rec_dev = reg.to_device()

    def embed(owners):
        rows = rec_dev[torch.tensor(owners, device="cuda")].contiguous()
        z = codec.embed_records(rows, E["msg_bytes"], E["shape"], u=torch.from_numpy(u[:len(owners)]).cuda())
        return PR.held(z.cpu().numpy().reshape(len(owners), -1), noise)

    one = embed([E["owner"]] * B)
    two = embed([E["owner"]] * 8 + [E["other"]] * 8)
    blank = PR.held(torch.special.ndtri(torch.from_numpy(u[:B]).clamp(1e-12, 1 - 1e-12)).float().numpy(), noise)
    return dict(recs=recs, cw=cw, reg=reg, one=one, two=two, blank=blank, flags=np.zeros(B, dtype=np.int64))


def _same(result, want, T, recs=None):
    """a SetTraceResult against the restatement's dict: exact but for the bound"""
    assert isinstance(result, T.SetTraceResult) and (result.size, result.skipped, result.wsq) == (want["size"], want["skipped"], want["wsq"])
    assert [(c.index, c.score, c.agree) for c in result.candidates] == [c[:3] for c in want["candidates"]]
    assert all(c.log10_p_any == pytest.approx(w[3], abs=1e-9) for c, w in zip(result.candidates, want["candidates"]))
    assert result.attributed == (None if want["attributed"] is None else f"u{want['attributed']}")
    assert all(c.user_id == f"u{c.index}" for c in result.candidates)


def test_pooling_attributes_the_set_no_image_is_attributed_alone(G, E2E):
    codec, S, T = G
    E = PR.E2E
    limit, B, U, n = math.log10(E["fpr"]), E["B"], E["U"], int(np.prod(E["shape"]))
    held = E2E["one"]
    signs = PR.sign_rows(held.numpy())
    everyone = [list(range(B))]
    sets = everyone + [[b] for b in range(B)] + [[0] * 8]
    want = PR.trace_sets(signs, None, E2E["flags"], sets, E2E["recs"], E2E["cw"], 2, E["fpr"])
    # the conditions, on the restatement alone
    singles = want[1:1 + B]
    exact = [T.log10_p_any(T.log10_p_soft(r["candidates"][0][1], n), U) for r in singles]
    print("single images, Hoeffding:", [round(r["candidates"][0][3], 2) for r in singles], "exact tail:", [round(x, 2) for x in exact])
    print("pooled:", want[0]["candidates"], "wsq", want[0]["wsq"])
    assert min(r["candidates"][0][3] for r in singles) >= limit + 1 and min(exact) >= limit + 1
    assert want[0]["attributed"] == E["owner"] and want[0]["candidates"][0][3] <= limit - 1
    # the device: the same user, score and wsq, set by set
    z = held.view(B, *E["shape"]).cuda()
    got = T.trace_sets_keyed(z, sets, E2E["reg"], k=2, fpr=E["fpr"])
    assert len(got) == len(sets)
    for r, w in zip(got, want):
        _same(r, w, T)
    assert got[0].attributed == f"u{E['owner']}" and all(r.attributed is None for r in got[1:])
    # what a caller runs today names nobody either
    assert all(r.attributed is None for r in T.trace_latents_keyed(z, E2E["reg"], fpr=E["fpr"]))
    # eight copies of one image carry that image's own bound
    assert got[-1].candidates[0].log10_p_any == pytest.approx(got[1].candidates[0].log10_p_any, abs=1e-9) and got[-1].wsq == 64 * got[1].wsq
    assert got[-1].candidates[0].score == 8 * got[1].candidates[0].score and got[-1].size == 8


def test_controls_blank_sets_two_users_flagged_images(G, E2E):
    codec, S, T = G
    E = PR.E2E
    limit, B = math.log10(E["fpr"]), E["B"]
    everyone = [list(range(B))]
    # 16 unwatermarked latents name nobody
    blank = E2E["blank"]
    want = PR.trace_sets(PR.sign_rows(blank.numpy()), None, E2E["flags"], everyone, E2E["recs"], E2E["cw"], 1, E["fpr"])
    got = T.trace_sets_keyed(blank.view(B, *E["shape"]).cuda(), everyone, E2E["reg"], fpr=E["fpr"])
    _same(got[0], want[0], T)
    assert got[0].attributed is None and want[0]["candidates"][0][3] > limit + 1
    # 8 + 8 images of two users, k = 2: exactly those two
    two = E2E["two"]
    want = PR.trace_sets(PR.sign_rows(two.numpy()), None, E2E["flags"], everyone, E2E["recs"], E2E["cw"], 2, E["fpr"])
    got = T.trace_sets_keyed(two.view(B, *E["shape"]).cuda(), everyone, E2E["reg"], k=2, fpr=E["fpr"])
    _same(got[0], want[0], T)
    assert {c.index for c in got[0].candidates} == {E["owner"], E["other"]}
    # a NaN and a saturated image are left out and counted; a set of them alone gets the reference's ValueError; an image may sit in several sets
    bad = E2E["one"].clone()
    bad[3, 5] = float("nan")
    bad[5, 9] = 9.0
    flags = E2E["flags"].copy()
    flags[[3, 5]] = 1
    sets = [list(range(B)), [3, 5], [5], [0, 3], [0]]
    want = PR.trace_sets(PR.sign_rows(bad.numpy()), None, flags, sets, E2E["recs"], E2E["cw"], 1, E["fpr"])
    got = T.trace_sets_keyed(bad.view(B, *E["shape"]).cuda(), sets, E2E["reg"], fpr=E["fpr"])
    assert want[1] is None and want[2] is None
    assert isinstance(got[1], ValueError) and "NaN" in str(got[1]) and isinstance(got[2], ValueError) and "base 2" in str(got[2])
    for i in (0, 3, 4):
        _same(got[i], want[i], T)
    assert (got[0].size, got[0].skipped) == (B - 2, 2) and (got[3].size, got[3].skipped) == (1, 1) and got[0].attributed == f"u{E['owner']}"
    with pytest.raises(ValueError, match="empty"):
        T.trace_sets_keyed(bad.view(B, *E["shape"]).cuda(), [[0], []], E2E["reg"])
    with pytest.raises(IndexError):
        T.trace_sets_keyed(bad.view(B, *E["shape"]).cuda(), [[0, B]], E2E["reg"])


def test_fifteen_levels_match_the_restatement(G, E2E):
    import keyed_soft_reference as KR
    codec, S, T = G
    E = PR.E2E
    B = E["B"]
    held = E2E["one"]
    z = held.view(B, *E["shape"]).cuda()
    thr = S.uniform_thresholds(z, 15, 2.5).cpu().numpy()                        # the table is the device's; the levels are restated from it
    rows = KR.level_rows(held.numpy(), thr)
    sets = [list(range(B)), [0, 1, 2], [4] * 5]
    want = PR.trace_sets(rows["signs"], rows["planes"], E2E["flags"], sets, E2E["recs"], E2E["cw"], 2, E["fpr"])
    got = T.trace_sets_keyed(z, sets, E2E["reg"], levels=15, k=2, fpr=E["fpr"])
    for r, w in zip(got, want):
        _same(r, w, T)
    unit = T.trace_sets_keyed(z, sets[:1], E2E["reg"], fpr=E["fpr"])[0]
    print("pooled bound of the 16 images: 15 levels", round(got[0].candidates[0].log10_p_any, 2), "unit levels", round(unit.candidates[0].log10_p_any, 2))
    with pytest.raises(ValueError, match="l = 2"):
        T.trace_sets_keyed(z, sets, E2E["reg"], levels=15, l=2)
    with pytest.raises(ValueError, match="68 images"):
        T.trace_sets_keyed(z, [[0] * 69], E2E["reg"], levels=15)


def test_multi_bit_windows_pool_at_unit_levels(G):
    """l = 2: the rows are quant_pack's, the codewords span n l bits"""
    codec, S, T = G
    rng = np.random.default_rng(8)
    shape, mb, U, B = (4, 8, 8), 8, 20, 6
    n = int(np.prod(shape))
    recs, cw = _records_and_codewords(rng, U, 2 * n, mb)
    reg = _rows(T, recs, mb)
    z = codec.embed_records(reg.to_device()[torch.tensor([7] * B, device="cuda")].contiguous(), mb, shape, seed=3, l=2)
    z = z + 0.6 * torch.randn(z.shape, generator=torch.Generator().manual_seed(1)).cuda()
    packed, flags = codec.quant_pack(z, 2)
    sets = [list(range(B)), [1, 2]]
    want = PR.trace_sets(packed.cpu().numpy(), None, flags.cpu().numpy(), sets, recs, cw, 3, 1e-6)
    got = T.trace_sets_keyed(z, sets, reg, k=3, l=2)
    for r, w in zip(got, want):
        _same(r, w, T)
    assert got[0].attributed == "u7"


def test_the_shared_key_form_gives_the_keyed_scores(G, E2E):
    codec, S, T = G
    E = PR.E2E
    B = E["B"]
    rng = np.random.default_rng(4)
    key, nonce = bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8))
    shared = T.Registry(E["msg_bytes"])
    for i in range(50):
        shared.add(f"s{i}", bytes(rng.integers(0, 256, E["msg_bytes"], dtype=np.uint8)))
    z = codec.embed_batch(key, nonce, shared.message_at(17), B, E["shape"], seed=9)
    z = (z + 6.0 * torch.randn(z.shape, generator=torch.Generator().manual_seed(2)).cuda()) / 37.0 ** 0.5      # (unit variance: nothing saturates)
    sets = [list(range(B)), [0, 1]]
    a = T.trace_sets(z, sets, key, nonce, shared, k=3)
    b = T.trace_sets_keyed(z, sets, T.keyed_from_shared(shared, key, nonce), k=3)
    assert a == b and a[0].attributed == "s17" and a[0].candidates[0].index == 17
    # the pooled score is the sum over the images of the shared-key soft score of that message
    single = T.trace_latents(z, key, nonce, shared, k=1)
    assert all(r.candidates[0].index == 17 for r in single) and a[0].candidates[0].score == sum(r.candidates[0].score for r in single)


# ------------------------------------------------------------------------------------------------------------ the front end
def test_cli_with_pool_subdirs(G, E2E, tmp_path, monkeypatch, capsys):
    """The front end with --pool subdirs on two small directories; as in test_gpu_align_soft.py the inversion is replaced by latents (chosen by the first
    pixel of the file) and no model is built.  The rest -- registry, packing across device batches, pooling, search, bounds, trace.txt -- is the real run."""
    from PIL import Image
    from gswm_amd import extract as X
    codec, S, T = G
    E = PR.E2E
    reg_file = tmp_path / "reg.tsv"
    E2E["reg"].save(reg_file)
    root = tmp_path / "imgs"
    latents = torch.cat([E2E["one"][:5], E2E["blank"][:3]]).view(8, *E["shape"]).cuda()
    where = {"leak": [0, 1, 2, 3, 4], "other": [5, 6, 7]}
    for name, members in where.items():
        (root / name).mkdir(parents=True)
        for i in members:
            Image.fromarray(np.full((16, 16, 3), i, dtype=np.uint8)).save(str(root / name / f"img{i}.png"))
    monkeypatch.setattr(X, "invert_decoded_images", lambda arrs, args, **kw: latents[[int(a[0, 0, 0]) for a in arrs]].clone())
    monkeypatch.setattr(X, "load_models", lambda *a, **kw: None)               # (nothing is inverted: building the synthetic UNet would be most of the test's time)
    T.main(["--images_directory_path", str(root), "--registry", str(reg_file), "--per_record_keys", "--allow_synthetic_weights", "--num_inference_steps", "2",
            "--width", "256", "--height", "256", "--strict_kernels", "0", "--is_traverse_subdirectories", "1", "--pool", "subdirs", "--batch_size", "2",
            "--top", "2"])
    out = capsys.readouterr().out
    want = T.trace_sets_keyed(latents, [where["leak"], where["other"]], E2E["reg"], k=2)
    each = T.trace_latents_keyed(latents, E2E["reg"], k=2)
    for (name, members), w in zip(where.items(), want):
        lines = (root / name / "trace.txt").read_text().splitlines()
        start = lines.index("=" * 40 + "Batch Start" + "=" * 40)
        info = dict(l.split(",", 1) for l in lines[1:start])
        assert info["pool"] == "subdirs" and "pool_reliability" not in info
        body = lines[start + 2:-1]
        order = [int(os.path.basename(f)[3:-4]) for f in X._DirJob(str(root / name)).files]                          # the job's own order of its files
        assert sorted(order) == members
        assert body[:-1] == [T.format_line(f"img{i}.png", each[i], E2E["reg"].message_bits) for i in order]         # the per-image lines, as they are
        assert body[-1] == T.format_set_line(name, w) and body[-1] in out
    assert T.format_set_line("leak", want[0]).startswith(f"set leak, images, 5, skipped, 0, user: u{E['owner']}, log10 p, -")
    assert T.format_set_line("other", want[1]).startswith("set other, images, 3, skipped, 0, user: none, ")


def test_cli_with_pool_all_and_reliability(G, E2E, tmp_path, monkeypatch, capsys):
    """--pool all --pool_reliability 15 on one directory: every traced image is one set, pooled from level_pack's rows; a file that cannot be decoded is
    reported on its own line and is not in the set"""
    from PIL import Image
    from gswm_amd import extract as X
    codec, S, T = G
    E = PR.E2E
    reg_file = tmp_path / "reg.tsv"
    E2E["reg"].save(reg_file)
    root = tmp_path / "leak"
    root.mkdir()
    latents = E2E["one"][:6].view(6, *E["shape"]).cuda()
    for i in range(6):
        Image.fromarray(np.full((16, 16, 3), i, dtype=np.uint8)).save(str(root / f"img{i}.png"))
    (root / "broken.png").write_bytes(b"not an image")
    monkeypatch.setattr(X, "invert_decoded_images", lambda arrs, args, **kw: latents[[int(a[0, 0, 0]) for a in arrs]].clone())
    monkeypatch.setattr(X, "load_models", lambda *a, **kw: None)
    T.main(["--images_directory_path", str(root), "--registry", str(reg_file), "--per_record_keys", "--allow_synthetic_weights", "--num_inference_steps", "2",
            "--width", "256", "--height", "256", "--strict_kernels", "0", "--pool", "all", "--pool_reliability", "15", "--batch_size", "4"])
    out = capsys.readouterr().out
    want = T.trace_sets_keyed(latents, [list(range(6))], E2E["reg"], levels=15)[0]
    lines = (root / "trace.txt").read_text().splitlines()
    start = lines.index("=" * 40 + "Batch Start" + "=" * 40)
    info = dict(l.split(",", 1) for l in lines[1:start])
    assert info["pool"] == "all" and info["pool_reliability"] == "15"
    body = lines[start + 2:-1]
    assert len(body) == 8 and sum(l.startswith("Error processing") for l in body[:-1]) == 1
    assert body[-1] == T.format_set_line("all", want) and body[-1] in out
    assert body[-1].startswith(f"set all, images, 6, skipped, 0, user: u{E['owner']}, log10 p, -")
    # a single image is a set of one: its line, then the set's
    T.main(["--single_image_path", str(root / "img2.png"), "--registry", str(reg_file), "--per_record_keys", "--allow_synthetic_weights", "--num_inference_steps", "2",
            "--width", "256", "--height", "256", "--strict_kernels", "0", "--pool", "all"])
    printed = capsys.readouterr().out.splitlines()
    assert printed[-1] == T.format_set_line("all", T.trace_sets_keyed(latents[2:3], [[0]], E2E["reg"])[0]) and printed[-2].startswith("img2.png, user: ")
