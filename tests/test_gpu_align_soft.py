"""GPU: the alignment search ranked by reliability levels -- codec.level_rows_align bit for bit against the NumPy restatement of
tests/align_soft_reference.py on poisoned, guard-banded buffers (tests/poison.py), through the C ABI at unaligned pointers, with unmappable entries, against
codec.rows_align and against the device's own level_pack of the aligned latents; align.search_keys_soft against its restatement (ties and chunking
included) and against the searches it generalises; then detect_latents_aligned_soft and align.extract_aligned_soft end to end on attacked latents under
noise of sigma 4, and the front end.  EXACT equality everywhere except the bounds (abs 1e-9 decades, as the other bound tests)."""
import math
import os

import numpy as np
import pytest
import torch

import align_reference as AR
import align_soft_reference as ASR
import gs_oracle as O
import key_search_reference as R
import key_search_soft_reference as KS
from poison import FINITE, NAN, Ledger, poisoned

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gswm_amd  # noqa: F401
    from gswm_amd import align, codec, detect, trace
    return codec, align, detect, trace


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


def _random_rows(rng, B, P, rowbytes):
    """-> (signs uint8 [B, rowbytes], planes uint8 [B, P, rowbytes], wsum, wsq int32 [B]): random bits, the sums those of the levels they encode"""
    signs = rng.integers(0, 256, (B, rowbytes), dtype=np.uint8)
    planes = rng.integers(0, 256, (B, P, rowbytes), dtype=np.uint8)
    lv = KS.levels_of_planes(planes)
    return signs, planes, lv.sum(axis=1).astype(np.int32), (lv * lv).sum(axis=1).astype(np.int32)


def _level_rows(codec, signs, planes, wsum, wsq, wrap=lambda t: t):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return codec.LevelRows(wrap(dev(signs)), wrap(dev(planes)), dev(wsum), dev(wsq), torch.arange(signs.shape[0], dtype=torch.int32).cuda())


def _cands(group, shift):
    def make(AL, H, W):
        return AL.alignments(group, shift, H, W)
    return make


# C, H, W, P, B, the list of alignments (a number: `_align_list`).  The issue's table: one byte and no whole word; 15-byte rows on a non-square lattice with
# the flips and shifts up to 1; odd W; all 72 candidates of d4 with shift 1; A = 200.  Then, at P = 3 (four rows), the largest lattice whose rows are staged
# in LDS (4 x 16 384 bytes) and the smallest that is not (rows of 16 385 bytes pad to 16 400); the top of the domain; and on 8-byte rows 17 x 200 (chunk 1),
# 34 x 200 (chunk 3, the last one holds 2) and 300 x 120 (chunk 16, the last one holds 8).
CASES = [(1, 2, 4, 1, 1, 3), (3, 5, 8, 2, 3, _cands("flips", 1)), (1, 8, 9, 3, 2, 5), (4, 8, 8, 4, 3, _cands("d4", 1)), (4, 32, 32, 4, 2, _cands("d4", 2)),
         (4, 128, 256, 3, 1, 3), (1, 8, 16385, 3, 1, 3), (4, 256, 256, 3, 1, 3),
         (1, 8, 8, 1, 17, 200), (1, 8, 8, 2, 34, 200), (1, 8, 8, 1, 300, 120)]


@pytest.mark.parametrize("C,H,W,P,B,A", CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}-P{c[3]}-B{c[4]}-{i}" for i, c in enumerate(CASES)])
def test_level_rows_align_matches_the_restatement(G, C, H, W, P, B, A):
    codec, AL = G[0], G[1]
    rng = np.random.default_rng(C + 3 * H + 7 * W + 11 * P + 13 * B)
    rowbytes = C * H * W // 8
    signs, planes, wsum, wsq = _random_rows(rng, B, P, rowbytes)
    aligns = _align_list(H, W, A) if isinstance(A, int) else A(AL, H, W)
    A = len(aligns)
    assert aligns[0] == (0, 0, 0)
    want_s, want_p = ASR.level_rows_align(signs, planes, (C, H, W), aligns)
    assert np.array_equal(want_s[:, 0], signs) and np.array_equal(want_p[:, 0], planes)
    table = torch.tensor(aligns, dtype=torch.int32).cuda()
    for name, pattern in (("NAN", NAN), ("FINITE", FINITE)):
        L = Ledger(pattern)
        try:
            with poisoned(L):
                out = codec.level_rows_align(_level_rows(codec, signs, planes, wsum, wsq, L.wrap), (C, H, W), L.wrap(table) if pattern == NAN else aligns)
            torch.cuda.synchronize()
            L.check()
            assert L.untouched(out.signs) == _by_chance(want_s, pattern), f"signs never written ({name} run) -- {L.where(out.signs)}"
            assert L.untouched(out.planes) == _by_chance(want_p, pattern), f"planes never written ({name} run) -- {L.where(out.planes)}"
            got_s, got_p = out.signs.cpu().numpy(), out.planes.cpu().numpy()
            rest = [t.cpu().numpy() for t in (out.wsum, out.wsq, out.flags)]
        finally:
            L.release()
        assert got_s.dtype == np.uint8 and got_s.shape == (B * A, rowbytes) and got_p.dtype == np.uint8 and got_p.shape == (B * A, P, rowbytes)
        assert np.array_equal(got_s.reshape(B, A, rowbytes), want_s), (name, np.argwhere(got_s.reshape(B, A, rowbytes) != want_s)[:5])
        assert np.array_equal(got_p.reshape(B, A, P, rowbytes), want_p), (name, np.argwhere(got_p.reshape(B, A, P, rowbytes) != want_p)[:5])
        for g, w in zip(rest, (wsum, wsq, np.arange(B, dtype=np.int32))):                      # a permutation keeps them: image b's value, A times
            assert g.dtype == np.int32 and np.array_equal(g, np.repeat(w, A))


def test_every_output_byte_is_written(G):
    """constant rows: all zeros permute to all zeros, which no byte of either pattern (0xFF / 0x7F, 0x4D) equals, so `untouched` must be exactly 0.  15-byte
    rows start at every address modulo 4, and the planes' rows at other phases than the sign rows'."""
    codec, AL = G[0], G[1]
    for C, H, W, P, B, A in ((3, 5, 8, 2, 3, 7), (1, 2, 4, 1, 5, 3), (4, 8, 8, 4, 17, 200)):
        aligns = _align_list(H, W, A)
        rb = C * H * W // 8
        z = np.zeros
        for pattern in (NAN, FINITE):
            L = Ledger(pattern)
            try:
                with poisoned(L):
                    out = codec.level_rows_align(_level_rows(codec, z((B, rb), np.uint8), z((B, P, rb), np.uint8), z(B, np.int32), z(B, np.int32), L.wrap), (C, H, W), aligns)
                torch.cuda.synchronize()
                L.check()
                assert L.untouched(out.signs) == 0, L.where(out.signs)
                assert L.untouched(out.planes) == 0, L.where(out.planes)
                assert not out.signs.any() and not out.planes.any()
            finally:
                L.release()


@pytest.mark.parametrize("offsets", [(1, 3, 3, 1), (3, 1, 1, 1), (1, 1, 3, 3)], ids=lambda o: "".join(map(str, o)))
def test_unaligned_pointers_through_the_c_abi(G, offsets):
    """input and output base pointers 1 and 3 bytes past a 4-byte boundary, the sign rows and the plane rows at the same phase and at different ones; the bytes
    in front of and behind every output stay pattern"""
    from gswm_amd import _native as N
    codec = G[0]
    o_s, o_p, o_os, o_op = offsets
    for (C, H, W), P, B, A in (((3, 5, 8), 2, 3, 7), ((4, 8, 8), 4, 2, 16), ((1, 2, 4), 1, 2, 3)):
        rng = np.random.default_rng(sum(offsets) + C + P)
        rb = C * H * W // 8
        signs, planes, _, _ = _random_rows(rng, B, P, rb)
        aligns = _align_list(H, W, A)
        want_s, want_p = ASR.level_rows_align(signs, planes, (C, H, W), aligns)
        table = torch.tensor(aligns, dtype=torch.int32).cuda()
        L = Ledger(FINITE)
        try:
            def place(a, off):
                buf = L.empty((a.size + 8,), torch.uint8, "cuda")
                buf[off:off + a.size] = torch.from_numpy(a.reshape(-1)).cuda()
                return buf
            in_s, in_p = place(signs, o_s), place(planes, o_p)
            out_s, out_p = L.empty((want_s.size + 8,), torch.uint8, "cuda"), L.empty((want_p.size + 8,), torch.uint8, "cuda")
            torch.cuda.synchronize()
            with torch.cuda.device(0):
                st = N.lib().gsw_level_rows_align(in_s.data_ptr() + o_s, in_p.data_ptr() + o_p, P, B, C, H, W, table.data_ptr(), A, out_s.data_ptr() + o_os,
                                                  out_p.data_ptr() + o_op, torch.cuda.current_stream().cuda_stream)
            assert st == N.GSW_OK
            torch.cuda.synchronize()
            L.check()
            for buf, off, want in ((out_s, o_os, want_s), (out_p, o_op, want_p)):
                assert L.untouched(buf[:off]) == off and L.untouched(buf[off + want.size:]) == 8 - off, (C, H, W, L.where(buf, untouched=False))
                assert np.array_equal(buf[off:off + want.size].cpu().numpy(), want.reshape(-1)), (C, H, W, offsets)
        finally:
            L.release()


def test_an_unmappable_entry_writes_zeros_and_leaves_its_neighbours(G):
    """a device table is not read on the host by the entry point: d = 9, and d = 1 on a non-square lattice, give rows of zeros in all 1 + P outputs"""
    codec = G[0]
    for (C, H, W), P, bad in (((4, 8, 8), 3, (9, 0, 0)), ((4, 8, 8), 1, (-1, 1, 1)), ((3, 5, 8), 2, (1, 0, 0)), ((3, 5, 8), 4, (7, 2, -1))):
        rng = np.random.default_rng(C * H + P)
        rb = C * H * W // 8
        B = 3
        signs, planes, wsum, wsq = _random_rows(rng, B, P, rb)
        good = [(0, 0, 0), (2, 1, -1), (6, -2, 3), (4, 0, 5)]
        aligns = good[:2] + [bad] + good[2:]
        want_s, want_p = ASR.level_rows_align(signs, planes, (C, H, W), good)
        want_s, want_p = np.insert(want_s, 2, 0, axis=1), np.insert(want_p, 2, 0, axis=1)
        L = Ledger(NAN)
        try:
            with poisoned(L):
                s, p = codec._level_rows_align_launch(_level_rows(codec, signs, planes, wsum, wsq, L.wrap), (C, H, W), L.wrap(torch.tensor(aligns, dtype=torch.int32).cuda()))
            torch.cuda.synchronize()
            L.check()
            assert L.untouched(s) == _by_chance(want_s, NAN) and L.untouched(p) == _by_chance(want_p, NAN)
            assert np.array_equal(s.cpu().numpy(), want_s) and np.array_equal(p.cpu().numpy(), want_p), (C, H, W, bad)
            assert not s[:, 2].any() and not p[:, 2].any()
        finally:
            L.release()
        with pytest.raises(ValueError):                                                    # the wrapper refuses the same list before any launch
            codec.level_rows_align(_level_rows(codec, signs, planes, wsum, wsq), (C, H, W), torch.tensor(aligns, dtype=torch.int32).cuda())


def test_level_rows_align_is_rows_align_of_every_row(G):
    codec, AL = G[0], G[1]
    for (C, H, W), P, B in (((4, 16, 16), 4, 3), ((3, 5, 8), 2, 2)):
        rng = np.random.default_rng(H)
        signs, planes, wsum, wsq = _random_rows(rng, B, P, C * H * W // 8)
        rows = _level_rows(codec, signs, planes, wsum, wsq)
        aligns = _align_list(H, W, 24)
        out = codec.level_rows_align(rows, (C, H, W), aligns)
        A = len(aligns)
        assert torch.equal(out.signs.view(B, A, -1), codec.rows_align(rows.signs, (C, H, W), 1, aligns))
        for q in range(P):
            assert torch.equal(out.planes.view(B, A, P, -1)[:, :, q], codec.rows_align(rows.planes[:, q].contiguous(), (C, H, W), 1, aligns))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float64])
@pytest.mark.parametrize("levels", [15, 5])
def test_level_rows_align_is_level_pack_of_the_aligned_latent(G, dtype, levels):
    """with the thresholds of the UN-aligned latents passed explicitly (a recomputed fp32 RMS of a permuted image may differ in the last bit); one NaN element"""
    from gswm_amd import soft
    codec, AL = G[0], G[1]
    z = (torch.randn(3, 4, 16, 16, generator=torch.Generator().manual_seed(levels), dtype=torch.float64) * 1.2).to(dtype)
    z[1, 2, 3, 5] = float("nan")
    z = z.cuda()
    thr = soft.uniform_thresholds(z, levels)
    rows = codec.level_pack(z, thr)
    assert rows.flags.tolist() == [0, 2, 0]
    aligns = [(d, 0, 0) for d in range(8)] + [(d, -3, 5) for d in range(8)]
    out = codec.level_rows_align(rows, (4, 16, 16), aligns)
    A, P = len(aligns), codec.level_planes(levels)
    for i, a in enumerate(aligns):
        want = codec.level_pack(AL.apply(z, a).contiguous(), thr)
        assert torch.equal(out.signs.view(3, A, -1)[:, i], want.signs), (dtype, a)
        assert torch.equal(out.planes.view(3, A, P, -1)[:, i], want.planes), (dtype, a)
        for g, w in ((out.wsum, want.wsum), (out.wsq, want.wsq), (out.flags, want.flags)):
            assert torch.equal(g.view(3, A)[:, i], w)


def test_level_rows_align_refuses_before_any_launch(G):
    codec = G[0]
    zeros = lambda *s, dt=torch.uint8: torch.zeros(*s, dtype=dt).cuda()
    rows = lambda B=2, P=2, rb=8: codec.LevelRows(zeros(B, rb), zeros(B, P, rb), zeros(B, dt=torch.int32), zeros(B, dt=torch.int32), zeros(B, dt=torch.int32))
    ident = [(0, 0, 0)]
    assert codec.level_rows_align(rows(), (1, 8, 8), ident).signs.shape == (2, 8)
    with pytest.raises(ValueError, match="whole bytes"):
        codec.level_rows_align(rows(rb=2), (1, 3, 3), ident)                                          # 9 bits
    with pytest.raises(ValueError, match="square"):
        codec.level_rows_align(rows(), (1, 4, 16), [(0, 0, 0), (3, 0, 0)])
    with pytest.raises(ValueError, match="0..7"):
        codec.level_rows_align(rows(), (1, 8, 8), [(8, 0, 0)])
    with pytest.raises(ValueError, match="0..7"):
        codec.level_rows_align(rows(), (1, 8, 8), torch.tensor([[0, 0, 0], [-1, 0, 0]], dtype=torch.int32).cuda())
    with pytest.raises(ValueError, match="at least one"):
        codec.level_rows_align(rows(), (1, 8, 8), [])
    with pytest.raises(ValueError):
        codec.level_rows_align(rows(), (1, 8, 16), ident)                                             # rows of 8 bytes, a lattice of 16
    with pytest.raises(ValueError, match="P in 1..4"):
        codec.level_rows_align(rows(P=5), (1, 8, 8), ident)
    with pytest.raises(ValueError, match="rows.planes"):
        r = rows()
        codec.level_rows_align(r._replace(planes=r.planes[:1]), (1, 8, 8), ident)
    with pytest.raises(ValueError, match="rows.wsum"):
        r = rows()
        codec.level_rows_align(r._replace(wsum=r.wsum.long()), (1, 8, 8), ident)
    with pytest.raises(ValueError, match="beyond the search's domain"):
        codec.level_rows_align(rows(B=1, P=4, rb=32768), (4, 256, 256), ident)                       # 262 144 x 5 bits
    with pytest.raises(ValueError):
        codec.level_rows_align(rows(), (1, 8, 8), torch.zeros(1, 3, dtype=torch.int64).cuda())
    with pytest.raises(RuntimeError):
        codec.level_rows_align(rows(), (1, 8, 8), torch.zeros(1, 3, dtype=torch.int32))              # a host table next to device rows
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r = rows()
        codec.level_rows_align(r._replace(planes=r.planes.cpu()), (1, 8, 8), ident)


# ------------------------------------------------------------------------------------------------------------ the search
def _pairs(rng, K):
    return [(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8))) for _ in range(K)]


def _key_rows(pairs):
    return torch.from_numpy(np.stack([np.frombuffer(k + n, dtype=np.uint8) for k, n in pairs]).copy()).cuda()


@pytest.fixture(scope="module")
def SEARCH(G):
    """4 x 8 x 8, six images, five keys of which rows 1 and 3 are the same (key, nonce), the 72 candidates of d4 with shift 1; image 2 is symmetric under the
    mirror of its last axis, so alignments (0, 0, 0) and (4, 0, 0) give it the same rows.  The restatement's statistics, computed once."""
    from gswm_amd import soft
    codec, AL = G[0], G[1]
    rng = np.random.default_rng(422)
    pairs = _pairs(rng, 5)
    pairs[3] = pairs[1]
    z = torch.randn(6, 4, 8, 8, generator=torch.Generator().manual_seed(422)).half()
    z[2, :, :, 4:] = torch.flip(z[2, :, :, :4], dims=(-1,))
    aligns = AL.alignments("d4", 1, 8, 8)
    zd = z.cuda()
    thr = soft.uniform_thresholds(zd, 15)
    signs, lv = ASR.rows_of(z, thr.cpu().numpy())
    S = ASR.search_stats(signs, lv, (4, 8, 8), aligns, R.keystreams(pairs, 256), 8)
    return dict(z=zd, thr=thr, keys=_key_rows(pairs), aligns=aligns, S=S)


@pytest.mark.parametrize("k", [1, 3])
def test_search_keys_soft_matches_the_restatement(G, SEARCH, k):
    codec, AL = G[0], G[1]
    S = SEARCH["S"]
    aligns = SEARCH["aligns"]
    want = AR.merge(S, k)
    assert np.array_equal(S[:, :, 1], S[:, :, 3])                                      # the forced key tie: row 3 never comes before row 1
    for order in want[0].tolist():
        assert 3 not in order or (1 in order and order.index(1) < order.index(3))
    i0, i4 = aligns.index((0, 0, 0)), aligns.index((4, 0, 0))
    assert i0 < i4 and np.array_equal(S[2, i0], S[2, i4])                               # the forced alignment tie: the mirror never comes before the identity
    assert not (want[1][2] == i4).any()
    A, per_row = len(aligns), 5 * 32                                                    # an aligned image: its sign row and four planes of 32 bytes
    assert A == 72
    for budget, launches in ((None, 1), (2 * A * per_row, 3), (24 * per_row, 18)):      # one chunk; the images cut in three; the alignments of ONE image cut in three
        calls = []
        real = codec.key_search_soft_topk
        codec.key_search_soft_topk = lambda *a, **kw: (calls.append(a[0].signs.shape[0]), real(*a, **kw))[1]
        try:
            got = AL.search_keys_soft(SEARCH["z"], SEARCH["keys"], 8, aligns, k=k, budget_bytes=budget)
        finally:
            codec.key_search_soft_topk = real
        assert len(calls) == launches and sum(calls) == 6 * A, (budget, calls)
        for g, w, name in zip(got, want, ("key", "align", "stat")):
            assert g.dtype == torch.int32 and tuple(g.shape) == (6, k)
            assert np.array_equal(g.cpu().numpy(), w), (budget, name, g, w)
    explicit = AL.search_keys_soft(SEARCH["z"], SEARCH["keys"], 8, aligns, thresholds=SEARCH["thr"], k=k)          # the default table is uniform_thresholds(z, 15)
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(explicit, want))


@pytest.mark.parametrize("k", [1, 3])
def test_search_keys_soft_generalises_the_searches_it_is_built_from(G, SEARCH, k):
    codec, AL = G[0], G[1]
    z, keys, aligns = SEARCH["z"], SEARCH["keys"], SEARCH["aligns"]
    # one plane of all ones (thresholds [0.0] on NaN-free images): the sign search, exactly
    unit = AL.search_keys_soft(z, keys, 8, aligns, thresholds=torch.zeros(1, dtype=torch.float32).cuda(), k=k)
    sign = AL.search_keys(z, keys, 8, aligns, k=k)
    for g, w in zip(unit, sign):
        assert torch.equal(g, w)
    # the identity alone: the soft key search on level_pack's rows
    one = AL.search_keys_soft(z, keys, 8, [(0, 0, 0)], k=k)
    idx, stat = codec.key_search_soft_topk(codec.level_pack(z, SEARCH["thr"]), 256, keys, 8, k=k)
    assert torch.equal(one[0], idx) and torch.equal(one[2], stat) and torch.equal(one[1], torch.where(idx >= 0, 0, -1).int())


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def E2E(G):
    """tests/align_soft_reference.py's experiment on latents from codec.embed_records with the same uniforms and the same noise"""
    codec, AL, D, T = G
    E = ASR.E2E
    pairs, msgs, u, noise, blank = ASR.e2e_setup()
    ring = D.Keyring()
    for i, (key, nonce) in enumerate(pairs):
        ring.add(f"key-{i}", key, nonce)
    stride = codec.keyed_record_stride(E["msg_bytes"])
    rows = np.zeros((len(msgs), stride), dtype=np.uint8)
    for b, (r, m) in enumerate(zip(E["rows"], msgs)):
        rows[b, :48 + len(m)] = np.frombuffer(pairs[r][0] + pairs[r][1] + m, dtype=np.uint8)
    clean = codec.embed_records(torch.from_numpy(rows).cuda(), E["msg_bytes"], E["shape"], u=torch.from_numpy(u).cuda(), dtype=torch.float32).cpu()
    z16 = ASR.e2e_attack(clean.numpy(), noise)
    cands = AL.alignments("d4", E["shift"], E["shape"][1], E["shape"][2])
    assert len(cands) == 200
    ks = R.keystreams(pairs, int(np.prod(E["shape"])))
    return dict(ring=ring, pairs=pairs, msgs=msgs, clean=clean, z16=z16.cuda(), blank=blank.cuda(), cands=cands, ks=ks)


def _both_ways(G, S, z16, k=1):
    """-> (the restatement's answer on these very latents and the device's threshold tables, the device's)"""
    from gswm_amd import soft
    codec, AL, D, T = G
    E = ASR.E2E
    thr = soft.uniform_thresholds(z16, E["levels"]).cpu().numpy()
    host = ASR.detect_host(z16.cpu(), thr, S["cands"], S["ks"], E["msg_bytes"], T.log10_p_any)
    dev = D.detect_latents_aligned_soft(z16, S["ring"], 8 * E["msg_bytes"], S["cands"], levels=E["levels"], k=k, fpr=E["fpr"])
    for h, d in zip(host, dev):
        top = d.candidates[0]
        print(f"key {h[0]} alignment {h[1]} stat {h[2]}: restated {h[3]:.6f}, device {top.log10_p_any:.6f}")
        assert (top.index, top.alignment, top.stat) == (h[0], S["cands"][h[1]], h[2]) and top.key_id == f"key-{h[0]}" and len(d.candidates) == k
        assert top.log10_p_any == pytest.approx(h[3], abs=1e-9)
    return host, dev


def test_fifteen_levels_name_six_keys_through_the_attacks_where_the_signs_name_two(G, E2E):
    """six 4 x 32 x 32 latents under rows of a keyring of 12, 64-bit messages, each through its attack, z' = fp16(z + 4 n), A = 200, fpr 1e-6.  The conditions
    are decided by the restatement (tests/test_align_soft_host.py holds the same case on the oracle's latents): every soft bound at least 1 decade below the
    limit, every sign bound that misses at least 1 decade above it; the device must equal the restatement."""
    codec, AL, D, T = G
    E = ASR.E2E
    limit = math.log10(E["fpr"])
    host, dev = _both_ways(G, E2E, E2E["z16"])
    sign_host = AR.detect_host(E2E["z16"].cpu(), E2E["cands"], E2E["ks"], E["msg_bytes"], D.log10_p_blind, T.log10_p_any)
    print(f"15 levels: log10 p_any {[round(float(h[3]), 2) for h in host]}\nsigns:     log10 p_any {[round(float(h[3]), 2) for h in sign_host]}")
    # the conditions, on the restatement alone
    assert [h[0] for h in host] == list(E["rows"]) and all(h[3] <= limit - 1.0 for h in host)
    named = [h[3] <= limit for h in sign_host]
    assert sum(named) == 2 and all(h[3] >= limit + 1.0 for h, n in zip(sign_host, named) if not n)
    # the device
    saturated = (E2E["z16"].view(6, -1).double() >= O.Y2_THRESHOLD).any(dim=1).cpu().tolist()     # (noise of sigma 4 reaches the quantiser's last cell)
    for b, (d, h) in enumerate(zip(dev, host)):
        assert d.key_id == f"key-{E['rows'][b]}" and d.message == h[4] and d.flags == (1 if saturated[b] else 0)
        assert d.alignment == d.candidates[0].alignment == AL.inverse(E["attacks"][b], 32, 32)
        attacked = AL.apply(E2E["clean"][b], E["attacks"][b])
        assert torch.equal(AL.apply(attacked, d.alignment), E2E["clean"][b])                      # exactly the lattice as embedded
        assert D.format_line("x.png", d).endswith(f", alignment: {AL.describe(d.alignment)}")
    # the sign statistic through the same candidates names exactly the two the restatement says
    sign_dev = D.detect_latents(E2E["z16"], E2E["ring"], 8 * E["msg_bytes"], fpr=E["fpr"], align=E2E["cands"])
    assert [d.key_id for d in sign_dev] == [f"key-{h[0]}" if n else None for h, n in zip(sign_host, named)]
    assert [(d.candidates[0].index, d.candidates[0].stat) for d in sign_dev] == [(h[0], h[2]) for h in sign_host]
    # reliability levels without alignment name only the un-attacked image
    from gswm_amd import soft
    thr = soft.uniform_thresholds(E2E["z16"], E["levels"]).cpu().numpy()
    plain_host = KS.detect_soft_host(E2E["z16"].view(6, -1).cpu(), thr, E2E["ks"], E["msg_bytes"], T.log10_p_any)
    assert [h[2] <= limit for h in plain_host] == [True] + [False] * 5
    plain = D.detect_latents(E2E["z16"], E2E["ring"], 8 * E["msg_bytes"], fpr=E["fpr"], reliability=E["levels"])
    assert [d.key_id for d in plain] == [f"key-{E['rows'][0]}"] + [None] * 5
    # k = 3: the runners-up are other keys, each with its own best alignment and its own law, none significant
    more = D.detect_latents_aligned_soft(E2E["z16"], E2E["ring"], 8 * E["msg_bytes"], E2E["cands"], levels=E["levels"], k=3, fpr=E["fpr"])
    for d, one in zip(more, dev):
        assert d.candidates[0] == one.candidates[0] and len({c.index for c in d.candidates}) == 3
        assert all(c.log10_p_any > limit and c.alignment in E2E["cands"] for c in d.candidates[1:])


def test_unwatermarked_latents_name_no_key(G, E2E):
    E = ASR.E2E
    host, dev = _both_ways(G, E2E, E2E["blank"])
    print("blank log10 p_any:", [round(h[3], 2) for h in host])
    assert len(dev) == 4 and all(h[3] > math.log10(E["fpr"]) for h in host)                       # the restatement alone meets the case
    assert all(d.key_id is None and d.message is None and d.alignment is None for d in dev)
    with pytest.raises(IndexError):
        G[2].detect_latents_aligned_soft(torch.zeros(1, 4, 10, 10).half().cuda(), E2E["ring"], 256, [(0, 0, 0)])    # 400 lattice bits, 256-bit messages


def test_extract_aligned_soft_under_the_known_key(G, E2E):
    codec, AL, D, T = G
    E = ASR.E2E
    full = D.detect_latents_aligned_soft(E2E["z16"], E2E["ring"], 8 * E["msg_bytes"], E2E["cands"], levels=E["levels"], fpr=E["fpr"])
    for b in (1, 4):
        key, nonce = E2E["pairs"][E["rows"][b]]
        r, other = AL.extract_aligned_soft(E2E["z16"][[b, 0]].contiguous(), key, nonce, 8 * E["msg_bytes"], E2E["cands"], levels=E["levels"], fpr=E["fpr"])
        top = full[b].candidates[0]
        assert r.alignment == top.alignment == AL.inverse(E["attacks"][b], 32, 32) and E2E["cands"][r.align_index] == r.alignment and r.stat == top.stat
        assert r.log10_p == pytest.approx(top.log10_p_any - math.log10(12), abs=1e-9) and r.detected and r.flags == full[b].flags      # the same law, Bonferroni over A not K A
        assert r.bits.tobytes() == full[b].message
        assert not other.detected                                                                 # image 0 is under another key


def test_cli_with_align_reliability(G, E2E, tmp_path, monkeypatch, capsys):
    """The front end with --align d4 --align_reliability 15 on two generated files; as in test_gpu_align.py the inversion is replaced by latents (the mirrored
    image and an unwatermarked one) and no model is built.  The rest -- keyring, candidates, thresholds, search, bounds, detect.txt -- is the real run."""
    from PIL import Image
    from gswm_amd import extract as X
    codec, AL, D, T = G
    E = ASR.E2E
    ring_file = tmp_path / "ring.tsv"
    E2E["ring"].save(ring_file)
    d = tmp_path / "imgs"
    d.mkdir()
    rng = np.random.RandomState(5)
    for i in range(2):
        Image.fromarray(rng.randint(0, 256, (64, 64, 3), dtype=np.uint8)).save(str(d / f"img{i}.png"))
    latents = torch.cat([E2E["z16"][1:2], E2E["blank"][:1]])
    monkeypatch.setattr(X, "invert_decoded_images", lambda arrs, args, **kw: latents[:len(arrs)].clone())
    monkeypatch.setattr(X, "load_models", lambda *a, **kw: None)               # (nothing is inverted: building the synthetic UNet would be most of the test's time)
    D.main(["--images_directory_path", str(d), "--keyring", str(ring_file), "--message_length", "64", "--allow_synthetic_weights", "--num_inference_steps", "2",
            "--width", "256", "--height", "256", "--strict_kernels", "0", "--align", "d4", "--align_shift", "1", "--align_reliability", "15"])
    out = capsys.readouterr().out
    lines = (d / "detect.txt").read_text().splitlines()
    start = lines.index("=" * 40 + "Batch Start" + "=" * 40)
    info = dict(l.split(",", 1) for l in lines[1:start])
    assert info["align"] == "d4" and info["align_shift"] == "1" and info["align_reliability"] == "15" and "reliability" not in info
    body = lines[start + 2:-1]
    files = X._DirJob(str(d)).files
    assert len(body) == len(files) == 2
    want = D.detect_latents_aligned_soft(latents, E2E["ring"], 64, AL.alignments("d4", 1, 32, 32), levels=15)
    for f, line, w in zip(files, body, want):
        assert line == D.format_line(os.path.basename(f), w) and ", alignment: " in line and line in out
    assert body[0].startswith(f"{os.path.basename(files[0])}, key: key-{E['rows'][1]}, log10 p, -") and body[0].endswith(", alignment: hflip")
    assert body[1].startswith(f"{os.path.basename(files[1])}, key: none, ") and ", message: none, alignment: " in body[1]
