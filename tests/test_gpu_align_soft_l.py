"""GPU: reliability levels of multi-bit windows (l = 2, 4) through the alignment searches -- codec.level_rows_align_l and
codec.level_counts_align_l bit for bit against the NumPy restatement of tests/align_soft_l_reference.py on poisoned, guard-banded buffers (tests/poison.py),
against the device's own packer and soft vote of the aligned latent and against codec.rows_align / codec.counts_align; l = 1 through the new C entry points against
the l = 1 entry points; the three searches against their restatement (cuts included); the end-to-end case at the noise tests/test_align_soft_l_host.py settles on
the restatement; the tamper map under an alignment and both front ends.  Integers are compared EXACTLY; the bounds, floats computed from equal integers, within 1e-9."""
import math
import os

import numpy as np
import pytest
import torch

import align_reference as AR
import align_soft_l_reference as ALR
import key_search_reference as R
import key_search_soft_reference as KS
import trace_align_reference as TR
import trace_align_soft_reference as TS
from poison import FINITE, NAN, Ledger, poisoned

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gswm_amd  # noqa: F401
    from gswm_amd import align, codec, detect, soft, trace
    assert hasattr(codec, "level_rows_align_l") and hasattr(codec, "level_counts_align_l")
    return codec, align, soft, trace, detect


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


def _by_chance(want, pattern):
    """how many bytes of the expected output equal the pattern's byte at their place (its low byte sits at even offsets): exactly those look untouched"""
    flat = want.reshape(-1)
    return int((flat[0::2] == (pattern & 0xFF)).sum() + (flat[1::2] == (pattern >> 8)).sum())


def _key(rng):
    return bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8))


def _random_rows(rng, B, P, rowbytes):
    signs = rng.integers(0, 256, (B, rowbytes), dtype=np.uint8)
    planes = rng.integers(0, 256, (B, P, rowbytes), dtype=np.uint8)
    return signs, planes, KS.levels_of_planes(planes)


def _rows(codec, signs, planes, lv, wrap=lambda t: t):
    """host rows -> a `codec.LevelRows` on the device; flags = the image's index, so that the repeat is seen"""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return codec.LevelRows(wrap(dev(signs)), wrap(dev(planes)), dev(lv.sum(axis=1).astype(np.int32)), dev((lv * lv).sum(axis=1).astype(np.int32)),
                           torch.arange(signs.shape[0], dtype=torch.int32).cuda())


# ------------------------------------------------------------------------------------------------------------ 1. rows against the restatement
# C, H, W, l, P, B, A (a number: `_align_list`; "d4": all of alignments("d4", 2, ...)).  6-byte rows: shorter than head + one word; 30-byte rows on a non-square
# lattice: output rows at phase 2, head and tail bytes, only even d; 32-byte rows at l = 4; 4 x 6 x 10 at both l (60 and 120 bytes); all 200 alignments at
# P = 4, B = 3; 17 x 400 on 32-byte rows: three alignments per workgroup with one in the last
ROW_CASES = [(1, 3, 8, 2, 1, 2, 5), (3, 5, 8, 2, 2, 3, 4), (1, 8, 8, 4, 3, 2, 9), (4, 6, 10, 2, 4, 3, 7), (4, 6, 10, 4, 2, 3, 7), (4, 16, 16, 4, 4, 3, "d4"),
             (1, 8, 8, 4, 1, 17, 400)]


@pytest.mark.parametrize("C,H,W,l,P,B,A", ROW_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}-l{c[3]}-P{c[4]}-B{c[5]}-A{c[6]}" for c in ROW_CASES])
def test_level_rows_align_l_matches_the_restatement(G, C, H, W, l, P, B, A):
    codec, AL = G[0], G[1]
    rng = np.random.default_rng(C + 3 * H + 7 * W + 11 * P + 13 * B + 17 * l)
    rb = C * H * W * l // 8
    signs, planes, lv = _random_rows(rng, B, P, rb)
    aligns = AL.alignments("d4", 2, H, W) if A == "d4" else _align_list(H, W, A)
    A = len(aligns)
    want_s, want_p = ALR.level_rows_align_l(signs, planes, (C, H, W), l, aligns)
    assert np.array_equal(want_s[:, 0], signs) and np.array_equal(want_p[:, 0], planes) and want_s.shape == (B, A, rb)
    table = torch.tensor(aligns, dtype=torch.int32).cuda()
    for name, pattern in (("NAN", NAN), ("FINITE", FINITE)):
        L = Ledger(pattern)
        try:
            with poisoned(L):
                out = codec.level_rows_align_l(_rows(codec, signs, planes, lv, L.wrap), (C, H, W), l, L.wrap(table) if pattern == NAN else aligns)
            torch.cuda.synchronize()
            L.check()
            assert L.untouched(out.signs) == _by_chance(want_s, pattern), f"signs never written ({name} run) -- {L.where(out.signs)}"
            assert L.untouched(out.planes) == _by_chance(want_p, pattern), f"planes never written ({name} run) -- {L.where(out.planes)}"
            got_s, got_p = out.signs.cpu().numpy(), out.planes.cpu().numpy()
            rest = [t.cpu().numpy() for t in (out.wsum, out.wsq, out.flags)]
        finally:
            L.release()
        assert got_s.dtype == np.uint8 and got_s.shape == (B * A, rb) and got_p.dtype == np.uint8 and got_p.shape == (B * A, P, rb)
        assert np.array_equal(got_s.reshape(B, A, rb), want_s), (name, np.argwhere(got_s.reshape(B, A, rb) != want_s)[:5])
        assert np.array_equal(got_p.reshape(B, A, P, rb), want_p), (name, np.argwhere(got_p.reshape(B, A, P, rb) != want_p)[:5])
        for g, w in zip(rest, (lv.sum(axis=1), (lv * lv).sum(axis=1), np.arange(B))):              # a permutation keeps them: image b's value, A times
            assert g.dtype == np.int32 and np.array_equal(g, np.repeat(w, A))


def test_rows_are_rows_align_of_every_row_and_an_entry_without_a_map_writes_zeros(G):
    """device against device: every one of the 1 + P rows is `rows_align`'s at that l; behind `align_table`'s back a quarter turn on a non-square lattice and a d
    outside 0..7 write zero rows, the entries between them what they should, nothing outside the outputs"""
    codec = G[0]
    rng = np.random.default_rng(3)
    for (C, H, W), l, P in (((3, 5, 8), 2, 2), ((4, 6, 10), 4, 3), ((2, 8, 8), 2, 4)):
        rb = C * H * W * l // 8
        signs, planes, lv = _random_rows(rng, 3, P, rb)
        rows = _rows(codec, signs, planes, lv)
        aligns = _align_list(H, W, 9)
        out = codec.level_rows_align_l(rows, (C, H, W), l, aligns)
        assert torch.equal(out.signs.view(3, 9, rb), codec.rows_align(rows.signs, (C, H, W), l, aligns))
        for k in range(P):
            assert torch.equal(out.planes.view(3, 9, P, rb)[:, :, k], codec.rows_align(rows.planes[:, k].contiguous(), (C, H, W), l, aligns))
    C, H, W, l, P = 3, 5, 8, 2, 2
    rb = C * H * W * l // 8
    signs, planes, lv = _random_rows(rng, 2, P, rb)
    aligns = [(0, 0, 0), (1, 0, 0), (2, 1, 1), (9, 0, 0), (-1, 2, 2)]
    want_s, want_p = ALR.level_rows_align_l(signs, planes, (C, H, W), l, [aligns[0], aligns[2]])
    L = Ledger(NAN)
    try:
        with poisoned(L):
            table = L.wrap(torch.tensor(aligns, dtype=torch.int32).cuda())
            s, p = codec._level_rows_align_launch(_rows(codec, signs, planes, lv, L.wrap), (C, H, W), table, l)
        torch.cuda.synchronize()
        L.check()
        s, p = s.cpu().numpy(), p.cpu().numpy()
    finally:
        L.release()
    assert np.array_equal(s[:, [0, 2]], want_s) and np.array_equal(p[:, [0, 2]], want_p)
    assert not s[:, [1, 3, 4]].any() and not p[:, [1, 3, 4]].any()


# ------------------------------------------------------------------------------------------------------------ 2. rows against the packer
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("l", [2, 4])
def test_rows_are_the_packer_s_of_the_aligned_latent(G, dtype, l):
    """row (b, a) is level_pack_l(align.apply(z[b], a), thr[b], l), signs and planes, over every alignment of d4 with shifts up to 2"""
    codec, AL, S = G[0], G[1], G[2]
    z = torch.randn(3, 4, 16, 16, generator=torch.Generator().manual_seed(l), dtype=torch.float64).to(dtype).cuda()
    aligns = AL.alignments("d4", 2, 16, 16)
    for thr in (S.window_thresholds(z, l, 15), S.window_thresholds(z, l, 5)[0].contiguous()):           # a table per image at P = 4, one for all at P = 3
        rows = codec.level_pack_l(z, thr, l)
        assert int(rows.flags.abs().sum()) == 0
        out = codec.level_rows_align_l(rows, (4, 16, 16), l, aligns)
        A, P, rb = len(aligns), rows.planes.shape[1], rows.signs.shape[1]
        for i, a in enumerate(aligns):
            want = codec.level_pack_l(AL.apply(z, a).contiguous(), thr, l)
            assert torch.equal(out.signs.view(3, A, rb)[:, i], want.signs) and torch.equal(out.planes.view(3, A, P, rb)[:, i], want.planes), (dtype, a)
            assert torch.equal(want.wsq, rows.wsq) and torch.equal(want.wsum, rows.wsum)


# ------------------------------------------------------------------------------------------------------------ 3. the SG path and the domain
def test_rows_read_in_place_beyond_the_lds_bound_and_the_domain_ends(G):
    """4 x 128 x 128 at l = 4 and P = 2: three rows of 32 KiB, 96 KiB padded, read in place from global memory; at P = 4 the same lattice is the first past
    n l (1 + P) <= 1 048 576 and is refused before a launch"""
    codec = G[0]
    from gswm_amd import _native as N
    C, H, W, l, P = 4, 128, 128, 4, 2
    rng = np.random.default_rng(5)
    rb = C * H * W * l // 8
    assert 3 * rb == 96 * 1024
    signs, planes, lv = _random_rows(rng, 1, P, rb)
    aligns = [(0, 0, 0), (5, 3, -2), (2, -1, 130)]
    want_s, want_p = ALR.level_rows_align_l(signs, planes, (C, H, W), l, aligns)
    L = Ledger(FINITE)
    try:
        with poisoned(L):
            out = codec.level_rows_align_l(_rows(codec, signs, planes, lv, L.wrap), (C, H, W), l, aligns)
        torch.cuda.synchronize()
        L.check()
        got_s, got_p = out.signs.cpu().numpy(), out.planes.cpu().numpy()
    finally:
        L.release()
    assert np.array_equal(got_s.reshape(1, 3, rb), want_s) and np.array_equal(got_p.reshape(1, 3, P, rb), want_p)
    z = lambda *s, dt=torch.uint8: torch.zeros(*s, dtype=dt).cuda()
    past = codec.LevelRows(z(1, rb), z(1, 4, rb), z(1, dt=torch.int32), z(1, dt=torch.int32), z(1, dt=torch.int32))
    with pytest.raises(ValueError, match="1 \\+ P"):
        codec.level_rows_align_l(past, (C, H, W), l, aligns)
    with pytest.raises(ValueError, match="1 \\+ P"):
        codec.level_counts_align_l(past, (C, H, W), l, aligns, bytes(32), bytes(16), 256)
    table = torch.tensor(aligns, dtype=torch.int32).cuda()
    with torch.cuda.device(0):
        st = N.lib().gsw_level_rows_align_l(past.signs.data_ptr(), past.planes.data_ptr(), 4, l, 1, C, H, W, table.data_ptr(), 3, past.signs.data_ptr(),
                                            past.planes.data_ptr(), None)
    assert st == N.GSW_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------------------ 4. l = 1 through the new C entry points
def test_l_1_through_the_new_entry_points_is_the_l_1_entry_points(G):
    codec = G[0]
    from gswm_amd import _native as N
    lib = N.lib()
    rng = np.random.default_rng(4)
    key, nonce = _key(rng)
    for (C, H, W), P, B, A, M in (((3, 5, 8), 2, 3, 7, 24), ((4, 16, 16), 4, 2, 20, 64), ((1, 2, 4), 1, 2, 3, 8)):
        rb = C * H * W // 8
        signs, planes, lv = _random_rows(rng, B, P, rb)
        rows = _rows(codec, signs, planes, lv)
        table = torch.tensor(_align_list(H, W, A), dtype=torch.int32).cuda()
        outs = []
        for window in ((), (1,)):
            s = torch.full((B, A, rb), 0x5A, dtype=torch.uint8).cuda()
            p = torch.full((B, A, P, rb), 0x5A, dtype=torch.uint8).cuda()
            score = torch.full((B, A, M), 12345, dtype=torch.int32).cuda()
            wsum = torch.full((B, A, M), 12345, dtype=torch.int32).cuda()
            stream = torch.cuda.current_stream().cuda_stream
            with torch.cuda.device(0):
                fn = lib.gsw_level_rows_align_l if window else lib.gsw_level_rows_align
                assert fn(rows.signs.data_ptr(), rows.planes.data_ptr(), P, *window, B, C, H, W, table.data_ptr(), A, s.data_ptr(), p.data_ptr(), stream) == N.GSW_OK
                fn = lib.gsw_level_counts_align_l if window else lib.gsw_level_counts_align
                assert fn(rows.signs.data_ptr(), rows.planes.data_ptr(), P, *window, B, C, H, W, table.data_ptr(), A, key, nonce, M, 77, score.data_ptr(),
                          wsum.data_ptr(), stream) == N.GSW_OK
            torch.cuda.synchronize()
            outs.append((s, p, score, wsum))
        for a, b in zip(*outs):
            assert torch.equal(a, b)
        want_s, want_w = TS.level_counts_align(signs, lv, (C, H, W), _align_list(H, W, A), R.keystreams([(key, nonce)], C * H * W)[0], M)
        assert np.array_equal(outs[1][2].cpu().numpy(), want_s + 77) and np.array_equal(outs[1][3].cpu().numpy(), want_w)


# ------------------------------------------------------------------------------------------------------------ 5. counts against the restatement
# C, H, W, l, M, P, B, A, levels ("random" or "top").  The word path: one message word; two message words with all 200 alignments at P = 4; 4 x 6 x 10 at l = 2
# (480 bits) on 32 bits; V = 1 at the longest message.  The byte path: M = 40 on 4 x 5 x 8 at l = 4 (16 copies; 255 of 256 lanes), M = 24 on a non-square lattice at
# l = 2, M = 8.  Three alignments per workgroup with one in the last.  Every level 15 on a row of 131 072 bits at l = 4: 16 words per lane, the cap of LDS at P = 4
COUNT_CASES = [(1, 8, 8, 4, 32, 1, 1, 1, "random"), (4, 16, 16, 4, 64, 4, 3, "d4", "random"), (4, 6, 10, 2, 32, 3, 3, 8, "random"), (2, 16, 16, 4, 2048, 2, 2, 8, "random"),
               (4, 5, 8, 4, 40, 4, 3, 7, "random"), (3, 5, 8, 2, 24, 2, 3, 4, "random"), (1, 3, 8, 2, 8, 1, 2, 5, "random"), (1, 8, 8, 4, 64, 2, 17, 400, "random"),
               (4, 64, 128, 4, 32, 4, 1, 2, "top"), (4, 64, 128, 4, 8, 4, 1, 2, "top")]


@pytest.mark.parametrize("C,H,W,l,M,P,B,A,levels", COUNT_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}-l{c[3]}-M{c[4]}-P{c[5]}-B{c[6]}-A{c[7]}" for c in COUNT_CASES])
def test_level_counts_align_l_matches_the_restatement(G, C, H, W, l, M, P, B, A, levels):
    codec, AL = G[0], G[1]
    rng = np.random.default_rng(C + 3 * H + 7 * W + 11 * P + 13 * B + 17 * M + l)
    nb = C * H * W * l
    signs = rng.integers(0, 256, (B, nb // 8), dtype=np.uint8)
    top = (1 << P) - 1
    lv = np.full((B, nb), top, dtype=np.int64) if levels == "top" else rng.integers(0, top + 1, (B, nb), dtype=np.int64)
    planes = KS.planes_of_levels(lv, P)
    key, nonce = _key(rng)
    aligns = AL.alignments("d4", 2, H, W) if A == "d4" else _align_list(H, W, A)
    A = len(aligns)
    bias = top * (nb // M) + 3
    want_s, want_w = ALR.level_counts_align_l(signs, lv, (C, H, W), l, aligns, R.keystreams([(key, nonce)], nb)[0], M)
    assert want_s.shape == want_w.shape == (B, A, M) and (np.abs(want_s) <= want_w).all() and int(want_w.max()) <= top * (nb // M)
    table = torch.tensor(aligns, dtype=torch.int32).cuda()
    for name, pattern in (("NAN", NAN), ("FINITE", FINITE)):
        L = Ledger(pattern)
        try:
            with poisoned(L):
                wrapped = _rows(codec, signs, planes, lv, L.wrap)
                score, wsum = codec.level_counts_align_l(wrapped, (C, H, W), l, L.wrap(table) if pattern == NAN else aligns, key, nonce, M, bias=bias,
                                                         return_wsum=True)                                   # a device table, a list
                alone = codec.level_counts_align_l(wrapped, (C, H, W), l, aligns, key, nonce, M)              # no wsum, no bias
            torch.cuda.synchronize()
            L.check()
            for out in (score, wsum, alone):
                assert L.untouched(out) == 0, f"never written ({name} run) -- {L.where(out)}"              # (no value is 0x7FFF7FFF or 0x4D4D4D4D)
            got_s, got_w, got_a = score.cpu().numpy(), wsum.cpu().numpy(), alone.cpu().numpy()
        finally:
            L.release()
        assert got_s.dtype == got_w.dtype == np.int32 and got_s.shape == got_w.shape == (B, A, M)
        assert np.array_equal(got_w, want_w), (name, np.argwhere(got_w != want_w)[:5])
        assert np.array_equal(got_s, want_s + bias), (name, np.argwhere(got_s != want_s + bias)[:5])
        assert np.array_equal(got_a, want_s), name


def test_counts_of_an_entry_without_a_map_are_the_bias_and_zeros(G):
    codec = G[0]
    rng = np.random.default_rng(11)
    C, H, W, l, M, P = 3, 5, 8, 2, 24, 2
    nb = C * H * W * l
    signs = rng.integers(0, 256, (2, nb // 8), dtype=np.uint8)
    lv = rng.integers(0, 4, (2, nb), dtype=np.int64)
    key, nonce = _key(rng)
    aligns = [(0, 0, 0), (1, 0, 0), (2, 1, 1), (9, 0, 0), (-1, 2, 2)]
    ok = [0, 2]
    want_s, want_w = ALR.level_counts_align_l(signs, lv, (C, H, W), l, [aligns[i] for i in ok], R.keystreams([(key, nonce)], nb)[0], M)
    L = Ledger(NAN)
    try:
        with poisoned(L):
            table = L.wrap(torch.tensor(aligns, dtype=torch.int32).cuda())
            score, wsum = codec._level_counts_align_launch(_rows(codec, signs, KS.planes_of_levels(lv, P), lv, L.wrap), (C, H, W), table, key, nonce, M, 77, True, l)
        torch.cuda.synchronize()
        L.check()
        assert L.untouched(score) == 0 and L.untouched(wsum) == 0
        score, wsum = score.cpu().numpy(), wsum.cpu().numpy()
    finally:
        L.release()
    assert np.array_equal(score[:, ok], want_s + 77) and np.array_equal(wsum[:, ok], want_w)
    assert (score[:, [1, 3, 4]] == 77).all() and not wsum[:, [1, 3, 4]].any()


@pytest.mark.parametrize("l", [2, 4])
def test_counts_are_the_soft_vote_of_the_aligned_latent_and_counts_align_on_unit_levels(G, l):
    codec, AL, S = G[0], G[1], G[2]
    key, nonce = _key(np.random.default_rng(1))
    aligns = [(d, 0, 0) for d in range(4)] + [(d, -3, 5) for d in range(4, 8)]
    for dtype in (torch.float16, torch.float32):
        z = torch.randn(3, 4, 16, 16, generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dtype).cuda()
        for thr in (S.window_thresholds(z, l, 15), S.window_thresholds(z, l, 5)[0].contiguous()):
            rows = codec.level_pack_l(z, thr, l)
            score, wsum = codec.level_counts_align_l(rows, (4, 16, 16), l, aligns, key, nonce, 64, return_wsum=True)
            for i, a in enumerate(aligns):
                vote = S.extract_soft_l(AL.apply(z, a).contiguous(), key, nonce, 64, l, thresholds=thr)
                assert torch.equal(score[:, i], vote.score) and torch.equal(wsum[:, i], vote.wsum), (dtype, a)
    rng = np.random.default_rng(2)
    for (C, H, W), M in (((4, 16, 16), 64), ((4, 5, 8), 40 if l == 4 else 80)):
        nb = C * H * W * l
        signs = rng.integers(0, 256, (5, nb // 8), dtype=np.uint8)
        ones = np.ones((5, nb), dtype=np.int64)
        rows = _rows(codec, signs, KS.planes_of_levels(ones, 1), ones)
        al = _align_list(H, W, 9)
        score, wsum = codec.level_counts_align_l(rows, (C, H, W), l, al, key, nonce, M, return_wsum=True)
        counts = codec.counts_align(rows.signs, (C, H, W), l, al, key, nonce, M)
        assert torch.equal(score, 2 * counts - nb // M) and bool((wsum == nb // M).all())
        assert torch.equal(codec.level_counts_align_l(rows, (C, H, W), l, al, key, nonce, M, bias=nb // M), 2 * counts)


# ------------------------------------------------------------------------------------------------------------ 6. the searches
@pytest.fixture(scope="module", params=[4, 2])
def SEARCH(request, G):
    """4 x 16 x 16, five noise images, 202 alignments of which the last two repeat entries 0 and 100, nine records / keys of which rows 2 and 6 are the same; the
    restatement's scores under the table that the device is given, computed once"""
    codec, AL, S, T, D = G
    l = request.param
    rng = np.random.default_rng(428 + l)
    z = torch.randn(5, 4, 16, 16, generator=torch.Generator().manual_seed(428 + l)).half()
    thr = S.window_thresholds(z, l, 15)
    aligns = AL.alignments("d4", 2, 16, 16)
    assert aligns[100] == (4, 0, 0)
    aligns = aligns + [(0, 16, -16), (4, 0, 16)]
    key, nonce = _key(rng)
    nb = 1024 * l
    msgs = [bytes(rng.integers(0, 256, 8, dtype=np.uint8)) for _ in range(9)]
    reg = T.Registry(8)
    for u, m in enumerate(msgs):
        reg.add(f"user-{u}", m)
    reg._messages[6] = reg._messages[2]
    reg._device_cache.clear()
    registry = np.stack([np.frombuffer(m, dtype=np.uint8) for m in reg._messages])
    _, Sh, wsq = ALR.shared_search(z, thr.numpy(), l, aligns, R.keystreams([(key, nonce)], nb)[0], registry)
    records = [(*_key(rng), m) for m in msgs]
    kreg = T.KeyedRegistry(8)
    for u, r in enumerate(records):
        kreg.add(f"user-{u}", *r)
    records[6] = kreg._records[6] = records[2]
    kreg._device_cache.clear()
    Kh, _ = ALR.keyed_search(z, thr.numpy(), l, aligns, TR.codewords(records, nb))
    pairs = [r[:2] for r in records]
    signs, lv, _ = ALR.rows_of(z, thr.numpy(), l)
    Dh = ALR.key_stats(signs, lv, (4, 16, 16), l, aligns, R.keystreams(pairs, nb), 8)
    keys_dev = torch.from_numpy(np.stack([np.frombuffer(k + n, dtype=np.uint8) for k, n in pairs]).copy()).cuda()
    return dict(l=l, z=z.cuda(), thr=thr.cuda(), aligns=aligns, key=key, nonce=nonce, reg=reg, S=Sh, wsq=wsq, kreg=kreg, KS=Kh, DS=Dh, keys_dev=keys_dev)


def _found(results):
    return [[(c.index, c.alignment, c.score) for c in r.candidates] for r in results]


@pytest.mark.parametrize("which", ["keys", "shared", "keyed"])
@pytest.mark.parametrize("k", [1, 3])
def test_the_searches_match_the_restatement(G, SEARCH, which, k):
    codec, AL, S, T, D = G
    l, aligns = SEARCH["l"], SEARCH["aligns"]
    A = len(aligns)
    Sc = SEARCH[{"keys": "DS", "shared": "S", "keyed": "KS"}[which]]
    rec, al, sc = (AR.merge if which == "keys" else ALR.merge)(Sc, k)
    assert np.array_equal(Sc[:, :, 2], Sc[:, :, 6]) and np.array_equal(Sc[:, 0], Sc[:, 200]) and np.array_equal(Sc[:, 100], Sc[:, 201])       # the forced ties
    assert (al < 200).all()
    rb = 128 * l
    per_image = 4 * 64 if which == "shared" else 5 * rb                              # bytes of one aligned image: its 64 scores, or its row and four planes
    for budget in (None, 2 * A * per_image, 70 * per_image):                         # one chunk; three chunks of images; the alignments of ONE image cut in three
        if which == "keys":
            key, aidx, stat = AL.search_keys_soft_l(SEARCH["z"], SEARCH["keys_dev"], 8, aligns, l, thresholds=SEARCH["thr"], k=k, budget_bytes=budget)
            assert np.array_equal(key.cpu().numpy(), rec) and np.array_equal(aidx.cpu().numpy(), al) and np.array_equal(stat.cpu().numpy(), sc), budget
            continue
        if which == "keyed":
            got = T.trace_latents_keyed_aligned_soft_l(SEARCH["z"], SEARCH["kreg"], aligns, l, thresholds=SEARCH["thr"], k=k, budget_bytes=budget)
        else:
            got = T.trace_latents_aligned_soft_l(SEARCH["z"], SEARCH["key"], SEARCH["nonce"], SEARCH["reg"], aligns, l, thresholds=SEARCH["thr"], k=k, budget_bytes=budget)
        want = [[(int(rec[b, j]), aligns[int(al[b, j])], int(sc[b, j])) for j in range(k)] for b in range(5)]
        assert _found(got) == want, (budget, _found(got), want)
        for b, r in enumerate(got):
            assert r.attributed is None and r.alignment is None                     # noise names nobody
            assert all(c.log10_p_any == T.log10_p_any(S.log10_p(c.score, int(SEARCH["wsq"][b])), 9 * A) for c in r.candidates)


# ------------------------------------------------------------------------------------------------------------ 7. end to end
@pytest.fixture(scope="module", params=[4, 2])
def E2E(request, G):
    codec, AL, S, T, D = G
    l = request.param
    E = ALR.E2E
    s = ALR.e2e_setup(l)
    cands = AL.alignments("d4", E["shift"], E["shape"][1], E["shape"][2])
    n = int(np.prod(E["shape"]))
    return dict(l=l, s=s, cands=cands, cw=TR.codewords(s["records"], n * l), want_al=ALR.restoring(cands), limit=math.log10(E["fpr"]), mods=(S, T, D))


def _close(a, b):
    return abs(a - b) <= 1e-9


def test_detect_reproduces_the_restatement(G, E2E):
    codec, AL, S, T, D = G
    e, l, E = E2E, E2E["l"], ALR.E2E
    z = ALR.attack(e["s"]["clean"], e["s"]["noise"], ALR.SIGMA)
    thr = S.window_thresholds(z.cuda(), l, E["levels"]).cpu().numpy()                                  # the table the detection takes by itself, as the device computes it
    h = dict(z=z, rows=E["rows"], levels=ALR.detect_host(z, thr, l, e["cands"], e["s"]["ks"], E["msg_bytes"], T.log10_p_any))
    assert ALR.named(h["levels"], h["rows"], e["want_al"], e["limit"]) == (6, 0)                       # the restatement alone meets the case
    ring = D.Keyring()
    for i, (key, nonce) in enumerate(e["s"]["pairs"]):
        ring.add(f"key-{i}", key, nonce)
    dev = D.detect_latents_aligned_soft_l(h["z"].cuda(), ring, 64, e["cands"], l, levels=15, fpr=E["fpr"])
    print(f"l = {l}: levels, log10 p over K A pairs:", [round(x[3], 1) for x in h["levels"]])
    for b, (d, x) in enumerate(zip(dev, h["levels"])):
        c = d.candidates[0]
        assert d.key_id == f"key-{E['rows'][b]}" and (c.index, c.stat) == (x[0], x[2]) and _close(c.log10_p_any, x[3]) and c.log10_p_any <= e["limit"]
        assert d.alignment == c.alignment == e["cands"][x[1]] == AL.inverse(E["attacks"][b], 32, 32) and d.message == x[4]
    out = AL.extract_aligned_soft_l(h["z"][:2].cuda(), *e["s"]["pairs"][E["rows"][1]], 64, e["cands"], l, fpr=E["fpr"])
    assert out[1].detected and out[1].alignment == e["cands"][h["levels"][1][1]] and out[1].bits.tobytes() == h["levels"][1][4] and not out[0].detected
    # unwatermarked latents name no key
    blank = TS.hold(e["s"]["blank"]).clone()
    none = D.detect_latents_aligned_soft_l(blank.cuda(), ring, 64, e["cands"], l, levels=15, fpr=E["fpr"])
    assert [r.key_id for r in none] == [None] * 4 and all(r.message is None and r.alignment is None for r in none)


@pytest.mark.parametrize("keyed", [False, True])
def test_the_traces_reproduce_the_restatement(G, E2E, keyed):
    codec, AL, S, T, D = G
    e, l, E = E2E, E2E["l"], ALR.E2E
    h = ALR.e2e_host("keyed" if keyed else "shared", e["s"], l, ALR.SIGMA, e["cands"], e["cw"], e["mods"])
    assert ALR.named(h["levels"], h["rows"], e["want_al"], e["limit"]) == (6, 0)                       # the restatement alone meets the case
    key, nonce = e["s"]["pairs"][0]
    if keyed:
        reg = T.KeyedRegistry(E["msg_bytes"])
        for u, r in enumerate(e["s"]["records"]):
            reg.add(f"user-{u}", *r)
        run = lambda z, **kw: T.trace_latents_keyed_aligned_soft_l(z.cuda(), reg, e["cands"], l, fpr=E["fpr"], **kw)
    else:
        reg = T.Registry(E["msg_bytes"])
        for u, m in enumerate(e["s"]["registry"]):
            reg.add(f"user-{u}", bytes(m))
        run = lambda z, **kw: T.trace_latents_aligned_soft_l(z.cuda(), key, nonce, reg, e["cands"], l, fpr=E["fpr"], **kw)
    dev = run(h["z"], thresholds=torch.from_numpy(h["thr"]).cuda())
    print(f"l = {l}, keyed = {keyed}: levels, log10 p over U A pairs:", [round(x[3], 1) for x in h["levels"]])
    signs, lv, _ = ALR.rows_of(h["z"], h["thr"], l)
    for b, (d, x) in enumerate(zip(dev, h["levels"])):
        top = d.candidates[0]
        assert d.attributed == f"user-{h['rows'][b]}" == top.user_id and len(d.candidates) == 1
        assert (top.index, top.score) == (x[0], x[2]) and _close(top.log10_p_any, x[3]) and top.log10_p_any <= e["limit"]
        assert d.alignment == top.alignment == e["cands"][x[1]] == AL.inverse(E["attacks"][b], 32, 32)
        rec = e["s"]["records"][x[0]] if keyed else (key, nonce, bytes(e["s"]["registry"][x[0]]))
        s_al, w_al = ALR.aligned_rows(signs[b:b + 1], lv[b:b + 1], E["shape"], l, [e["cands"][x[1]]])
        voted = KS.voted_message(s_al[0, 0], w_al[0, 0], R.keystreams([rec[:2]], 4096 * l)[0], E["msg_bytes"])
        assert top.agree == 64 - int(np.unpackbits(np.frombuffer(voted, dtype=np.uint8) ^ np.frombuffer(rec[2], dtype=np.uint8)).sum()) and top.agree > 32
    own = run(h["z"])                                                                                  # the table the tracer takes by itself names the same six
    assert [(d.attributed, d.alignment) for d in own] == [(d.attributed, d.alignment) for d in dev]
    blank = TS.hold(e["s"]["blank"]).clone()
    blank[3, 0, 0, 0] = float("nan")
    none = run(blank)
    assert all(r.attributed is None and r.alignment is None for r in none[:3])
    assert isinstance(none[3], ValueError) and "NaN" in str(none[3])
    raw = blank.clone()
    raw[3, 0, 0, 0] = 9.0                                                                              # saturated: the reference cannot read the element
    out = run(raw)
    assert isinstance(out[3], ValueError) and "invalid literal for int() with base 2" in str(out[3]) and not isinstance(out[0], Exception)


# ------------------------------------------------------------------------------------------------------------ 8. the tamper map and the front ends
def _mirrored_half(e, l, keyed):
    """image 1 as embedded, its top 16 lattice rows replaced by noise, THEN mirrored"""
    src = e["s"]["clean"] if keyed else e["s"]["shared_clean"]
    z = torch.from_numpy(src[1]).clone()
    z[:, :16, :] = torch.randn(4, 16, 32, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    return torch.flip(z, dims=(-1,)).half()[None].contiguous()


@pytest.mark.parametrize("keyed", [False, True])
def test_tamper_map_under_an_alignment(G, E2E, keyed):
    """the level-weighted tracers at l still attribute the image, and its map -- in the coordinates of the lattice as embedded -- marks intact tiles in the surviving
    lower half only and equals the map of the restatement's quantised row"""
    codec, AL, S, T, D = G
    from gswm_amd import tamper as TM
    e, l, E = E2E, E2E["l"], ALR.E2E
    z16 = _mirrored_half(e, l, keyed)
    if keyed:
        row = E["keyed_rows"][1]
        rec = e["s"]["records"][row]
        reg = T.KeyedRegistry(E["msg_bytes"])
        reg.add("someone", bytes(range(32)), bytes(range(16)), bytes(8))
        reg.add("issuer", *rec)
        (r,) = T.trace_latents_keyed_aligned_soft_l(z16.cuda(), reg, e["cands"], l, fpr=E["fpr"], tamper_tile=8)
        assert r.attributed == "issuer"
    else:
        row = E["shared_rows"][1]
        rec = (*e["s"]["pairs"][0], bytes(e["s"]["registry"][row]))
        reg = T.Registry(E["msg_bytes"])
        for u, m in enumerate(e["s"]["registry"]):
            reg.add(f"user-{u}", bytes(m))
        (r,) = T.trace_latents_aligned_soft_l(z16.cuda(), rec[0], rec[1], reg, e["cands"], l, fpr=E["fpr"], tamper_tile=8)
        assert r.attributed == f"user-{row}"
    assert r.alignment == (4, 0, 0) and r.tamper is not None and r.tamper.source == "registry"
    back = AR.rows_align(ALR.quant_rows(z16, l), E["shape"], l, [r.alignment])[0, 0]
    cw = TR.codewords([rec], 4096 * l)[0]
    eq = (np.unpackbits(back) == np.unpackbits(cw)).reshape(4, 4, 8, 4, 8, l)                           # (C, H / 8, 8, W / 8, 8, l)
    agree = eq.sum(axis=(0, 2, 4, 5)).astype(np.int64)
    want = TM.make_map(agree, 4 * 64 * l, 8, E["fpr"], "registry")
    assert np.array_equal(r.tamper.agree, agree) and np.array_equal(r.tamper.intact, want.intact)
    assert not r.tamper.intact[:2].any() and r.tamper.intact[2:].all()                                 # only the surviving half, and all of it (no noise was added)
    assert f", intact tiles 8/16, alignment: {AL.describe((4, 0, 0))}" in T.format_line("x.png", r, 64)


@pytest.mark.parametrize("keyed", [False, True])
def test_trace_cli_with_align_window_reliability(G, E2E, keyed, tmp_path, monkeypatch, capsys):
    """The front end with --align d4 --align_shift 2 --align_window_reliability 15 --l l --tamper_map on two generated files.  The inversion is replaced by latents
    (the mirrored image and an unwatermarked one) and no model is built; registry, candidates, search, trace.txt and the maps are the real run."""
    from PIL import Image
    from gswm_amd import extract as X
    codec, AL, S, T, D = G
    e, l, E = E2E, E2E["l"], ALR.E2E
    d = tmp_path / "imgs"
    d.mkdir()
    rng = np.random.RandomState(5)
    for i in range(2):
        Image.fromarray(rng.randint(0, 256, (64, 64, 3), dtype=np.uint8)).save(str(d / f"img{i}.png"))
    src = e["s"]["clean"] if keyed else e["s"]["shared_clean"]
    mirrored = torch.flip(torch.from_numpy(src[1]), dims=(-1,)).half()[None]
    latents = torch.cat([mirrored, e["s"]["blank"][:1]]).cuda()
    monkeypatch.setattr(X, "invert_decoded_images", lambda arrs, args, **kw: latents[:len(arrs)].clone())
    monkeypatch.setattr(X, "load_models", lambda *a, **kw: None)               # (nothing is inverted: building the synthetic UNet would be most of the test's time)
    reg_file = tmp_path / "registry.tsv"
    key, nonce = e["s"]["pairs"][0]
    if keyed:
        reg = T.KeyedRegistry(E["msg_bytes"])
        base = E["keyed_rows"][1] - 7
        for u in range(20):
            reg.add(f"user-{u}", *e["s"]["records"][base + u])
        extra, user = ["--per_record_keys"], "user-7"
    else:
        reg = T.Registry(E["msg_bytes"])
        for u, m in enumerate(e["s"]["registry"]):
            reg.add(f"user-{u}", bytes(m))
        extra, user = ["--key_hex", key.hex(), "--nonce_hex", nonce.hex()], f"user-{E['shared_rows'][1]}"
    reg.save(reg_file)
    maps = tmp_path / "maps"
    T.main(["--images_directory_path", str(d), "--registry", str(reg_file), "--allow_synthetic_weights", "--num_inference_steps", "2", "--width", "256",
            "--height", "256", "--strict_kernels", "0", "--align", "d4", "--align_shift", "2", "--align_window_reliability", "15", "--l", str(l), "--top", "2",
            "--tamper_map", str(maps)] + extra)
    out = capsys.readouterr().out
    lines = (d / "trace.txt").read_text().splitlines()
    start = lines.index("=" * 40 + "Batch Start" + "=" * 40)
    info = dict(ln.split(",", 1) for ln in lines[1:start])
    assert info["statistic"] == "soft, 15 reliability levels per window bit over 200 alignments" and info["alignments"] == "200" and info["users"] == str(len(reg))
    body = lines[start + 2:-1]
    files = X._DirJob(str(d)).files
    assert len(body) == len(files) == 2
    if keyed:
        want = T.trace_latents_keyed_aligned_soft_l(latents, reg, e["cands"], l, levels=15, k=2, tamper_tile=8)
    else:
        want = T.trace_latents_aligned_soft_l(latents, key, nonce, reg, e["cands"], l, levels=15, k=2, tamper_tile=8)
    for f, line, w in zip(files, body, want):
        assert line == T.format_line(os.path.basename(f), w, 64) and line in out
    assert body[0].startswith(f"{os.path.basename(files[0])}, user: {user}, agreement, 1.0, log10 p, -") and body[0].endswith(", intact tiles 16/16, alignment: hflip")
    assert body[1].startswith(f"{os.path.basename(files[1])}, user: none, ") and "alignment" not in body[1]
    stem = os.path.splitext(os.path.basename(files[0]))[0]
    assert sorted(os.listdir(maps)) == [f"{stem}.tamper.npy", f"{stem}.tamper.png"]                    # the attributed image alone has a map
    for bad in (["--align_window_reliability", "15", "--l", str(l)], ["--align", "d4", "--align_window_reliability", "15", "--l", "1"]):
        with pytest.raises(SystemExit):
            T.main(["--images_directory_path", str(d), "--registry", str(reg_file)] + bad + extra)


def test_detect_cli_with_align_window_reliability(G, E2E, tmp_path, monkeypatch, capsys):
    from PIL import Image
    from gswm_amd import extract as X
    codec, AL, S, T, D = G
    e, l, E = E2E, E2E["l"], ALR.E2E
    d = tmp_path / "imgs"
    d.mkdir()
    rng = np.random.RandomState(6)
    for i in range(2):
        Image.fromarray(rng.randint(0, 256, (64, 64, 3), dtype=np.uint8)).save(str(d / f"img{i}.png"))
    mirrored = torch.flip(torch.from_numpy(e["s"]["clean"][1]), dims=(-1,)).half()[None]
    latents = torch.cat([mirrored, e["s"]["blank"][:1]]).cuda()
    monkeypatch.setattr(X, "invert_decoded_images", lambda arrs, args, **kw: latents[:len(arrs)].clone())
    monkeypatch.setattr(X, "load_models", lambda *a, **kw: None)
    ring = D.Keyring()
    for i, (key, nonce) in enumerate(e["s"]["pairs"]):
        ring.add(f"key-{i}", key, nonce)
    ring_file = tmp_path / "ring.tsv"
    ring.save(ring_file)
    D.main(["--images_directory_path", str(d), "--keyring", str(ring_file), "--allow_synthetic_weights", "--num_inference_steps", "2", "--width", "256", "--height", "256",
            "--strict_kernels", "0", "--message_length", "64", "--align", "d4", "--align_shift", "2", "--align_window_reliability", "15", "--l", str(l)])
    out = capsys.readouterr().out
    lines = (d / "detect.txt").read_text().splitlines()
    start = lines.index("=" * 40 + "Batch Start" + "=" * 40)
    info = dict(ln.split(",", 1) for ln in lines[1:start])
    assert info["align_window_reliability"] == "15" and info["l"] == str(l) and info["align"] == "d4"
    body = lines[start + 2:-1]
    files = X._DirJob(str(d)).files
    want = D.detect_latents_aligned_soft_l(latents, ring, 64, e["cands"], l, levels=15)
    for f, line, w in zip(files, body, want):
        assert line == D.format_line(os.path.basename(f), w) and line in out
    assert f"key: key-{E['rows'][1]}, " in body[0] and body[0].endswith(", alignment: hflip") and e["s"]["msgs"][1].hex() in body[0]
    assert "key: none" in body[1]
