"""GPU: the tile agreement map (codec.tile_agreement) and the tile-weighted vote (codec.vote_tiled) against the NumPy restatement of
tests/tamper_reference.py (codewords from gs_oracle.cipher_bits / keystream_bits), the identities with extract_batch and trace_keyed_topk,
poisoned and guard-banded buffers, every refusal, then tamper.extract_robust, trace_latents(..., tamper_tile=) and the front end.
EXACT equality everywhere, no tolerance."""
import os

import numpy as np
import pytest
import torch

from conftest import README_KEY, README_NONCE

import gs_oracle as O
import tamper_reference as R
from poison import FINITE, NAN, Ledger, poisoned

pytestmark = pytest.mark.gpu

KEY, NONCE = bytes.fromhex(README_KEY), bytes.fromhex(README_NONCE)


@pytest.fixture(scope="module")
def G():
    import gswm_amd
    from gswm_amd import codec, tamper, trace
    return codec, tamper, trace


def _operands(seed, B, shape, l, M):
    """random packed rows (the kernels' operand is bits: any bits will do), a key, nonce and message per image; image 1 (image 0 when B == 1)
    starts at block counter 0xFFFFFFFF so that the 32-bit counter carries into the next word inside the row"""
    rng = np.random.default_rng(seed)
    nb = int(np.prod(shape)) * l
    packed = rng.integers(0, 256, (B, nb // 8), dtype=np.uint8)
    recs = []
    for b in range(B):
        key, nonce = bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8))
        if b == min(1, B - 1):
            nonce = b"\xff\xff\xff\xff" + nonce[4:]
        recs.append((key, nonce, bytes(rng.integers(0, 256, M // 8, dtype=np.uint8))))
    return rng, nb, packed, recs


def _dev(codec, tamper, packed, recs):
    keys = tamper.keys_tensor([(k, n) for k, n, _ in recs], "cuda")
    msgs = torch.from_numpy(np.frombuffer(b"".join(m for _, _, m in recs), dtype=np.uint8).reshape(len(recs), -1).copy()).cuda()
    return torch.from_numpy(packed).cuda(), keys, msgs


CASES = [((4, 8, 8), 8, 32),               # one tile
         ((4, 16, 24), 8, 64),             # not square, several tiles
         ((4, 64, 64), 8, 256), ((4, 64, 64), 16, 256),
         ((4, 96, 96), 16, 256), ((4, 96, 96), 32, 256), ((4, 96, 96), 16, 1024), ((4, 96, 96), 32, 1024),      # ChaCha blocks straddle rows and tiles
         ((1, 32, 32), 32, 128)]


@pytest.mark.parametrize("l", [1, 2, 4])
@pytest.mark.parametrize("shape,tile,M", CASES)
def test_map_and_vote_match_the_restatement(G, shape, tile, M, l):
    codec, tamper, T = G
    B = 3
    rng, nb, packed, recs = _operands(1000 * l + tile + M + shape[1], B, shape, l, M)
    assert nb % M == 0
    th, tw = shape[1] // tile, shape[2] // tile
    weights = rng.choice(np.array([0, 1, 2, 77, 4096, 65535], dtype=np.uint16), size=(B, th, tw))
    want_agree, want_vote = [], []
    for b, (key, nonce, msg) in enumerate(recs):
        q = np.unpackbits(packed[b])
        want_agree.append(R.tile_agree(q, R.codeword(msg, key, nonce, nb), shape, l, tile))
        want_vote.append(R.vote(q, O.keystream_bits(key, nonce, nb), weights[b], M, shape, l, tile))
    for Bn in (3, 1):                      # B == 1: image 0 alone (the image whose counter carries is image 1; alone, in the test below)
        p, k, m = _dev(codec, tamper, packed[:Bn], recs[:Bn])
        agree = codec.tile_agreement(p, k, m, M, shape, l, tile)
        assert agree.dtype == torch.int32 and agree.shape == (Bn, th, tw)
        assert np.array_equal(agree.cpu().numpy(), np.stack(want_agree[:Bn]))
        bits, score, wsum = codec.vote_tiled(p, k, torch.from_numpy(weights[:Bn].copy()).cuda(), M, shape, l, tile)
        assert bits.dtype == torch.uint8 and bits.shape == (Bn, M // 8) and score.dtype == wsum.dtype == torch.int32 and score.shape == wsum.shape == (Bn, M)
        for b in range(Bn):
            wb, ws, ww = want_vote[b]
            assert np.array_equal(score[b].cpu().numpy(), ws) and np.array_equal(wsum[b].cpu().numpy(), ww)
            assert np.array_equal(bits[b].cpu().numpy(), np.packbits(wb))


def test_single_image_under_a_carrying_counter(G):
    """B == 1 with the initial counter 0xFFFFFFFF (in the case above the carrying image is image 1 of 3)"""
    codec, tamper, T = G
    shape, l, tile, M = (4, 16, 24), 2, 8, 64
    rng, nb, packed, recs = _operands(5, 1, shape, l, M)
    assert recs[0][1][:4] == b"\xff\xff\xff\xff"
    p, k, m = _dev(codec, tamper, packed, recs)
    q = np.unpackbits(packed[0])
    assert np.array_equal(codec.tile_agreement(p, k, m, M, shape, l, tile)[0].cpu().numpy(), R.tile_agree(q, R.codeword(recs[0][2], recs[0][0], recs[0][1], nb), shape, l, tile))
    ones = torch.ones((1, 2, 3), dtype=torch.int16).view(torch.uint16).cuda()
    bits, score, wsum = codec.vote_tiled(p, k, ones, M, shape, l, tile)
    wb, ws, ww = R.vote(q, O.keystream_bits(recs[0][0], recs[0][1], nb), np.ones((2, 3)), M, shape, l, tile)
    assert np.array_equal(score[0].cpu().numpy(), ws) and np.array_equal(wsum[0].cpu().numpy(), ww) and np.array_equal(bits[0].cpu().numpy(), np.packbits(wb))


FULL_ROWS = [((4, 512, 512), 1, 32, 4096),         # 256 tiles of 4096 bits; dword segments, 256 copies (x 65535 fits int32)
             ((1, 512, 512), 4, 8, 1024)]          # 4096 tiles: the tile loop runs 128 passes; 4-byte segments, 1024 copies


@pytest.mark.parametrize("shape,l,tile,M", FULL_ROWS)
def test_the_row_that_fills_lds(G, shape, l, tile, M):
    """Nb = 2^20, the edge of both kernels' domain: the row alone is the 131 072 bytes of LDS a launch may take, so neither kernel has a byte beside it"""
    codec, tamper, T = G
    rng, nb, packed, recs = _operands(31 + l, 1, shape, l, M)
    assert nb == 1 << 20 and nb % M == 0
    th, tw = shape[1] // tile, shape[2] // tile
    weights = rng.choice(np.array([0, 1, 65535], dtype=np.uint16), size=(1, th, tw))
    key, nonce, msg = recs[0]
    q, ks = np.unpackbits(packed[0]), O.keystream_bits(key, nonce, nb)
    want_agree = R.tile_agree(q, R.message_codeword(np.unpackbits(np.frombuffer(msg, dtype=np.uint8)), ks), shape, l, tile)
    wb, ws, ww = R.vote(q, ks, weights[0], M, shape, l, tile)
    assert int(ww.max()) < 2 ** 31
    p, k, m = _dev(codec, tamper, packed, recs)
    assert np.array_equal(codec.tile_agreement(p, k, m, M, shape, l, tile)[0].cpu().numpy(), want_agree)
    bits, score, wsum = codec.vote_tiled(p, k, torch.from_numpy(weights.copy()).cuda(), M, shape, l, tile)
    assert np.array_equal(score[0].cpu().numpy(), ws) and np.array_equal(wsum[0].cpu().numpy(), ww) and np.array_equal(bits[0].cpu().numpy(), np.packbits(wb))


def test_decode_robust_refuses_the_row_that_fills_lds(G):
    """the two families differ there on purpose: the robust decode keeps weights and message beside the row"""
    codec, tamper, T = G
    shape, l, tile, M = FULL_ROWS[0]
    p, k = torch.zeros((1, 1 << 17), dtype=torch.uint8).cuda(), torch.zeros((1, 48), dtype=torch.uint8).cuda()
    with pytest.raises(ValueError, match="bytes of LDS"):
        codec.decode_robust(p, None, k, M, shape, l, tile)


@pytest.mark.parametrize("l", [1, 2, 4])
def test_unit_weights_are_the_plain_vote_and_the_map_sums_to_the_keyed_score(G, l):
    codec, tamper, T = G
    shape, M, B, tile = (4, 64, 64), 256, 3, 8
    msg = codec.pad_message("lthero", 32)
    z = codec.embed_batch(KEY, NONCE, msg, B, shape, seed=3, l=l)
    g = torch.Generator().manual_seed(l)
    z = (z + 1.2 * torch.randn(z.shape, generator=g).cuda()).contiguous()
    bits0, flags, counts = codec.extract_batch(z, KEY, NONCE, M, return_counts=True, l=l)
    assert int(flags.abs().sum()) == 0
    packed, _ = codec.quant_pack(z, l)
    keys = tamper.keys_tensor([(KEY, NONCE)] * B, "cuda")
    ones = torch.ones((B, 8, 8), dtype=torch.int16).view(torch.uint16).cuda()
    bits, score, wsum = codec.vote_tiled(packed, keys, ones, M, shape, l, tile)
    copies = codec.vote_copies(4 * 64 * 64, M, l)
    assert torch.equal(score, 2 * counts - copies) and torch.equal(bits, bits0) and bool((wsum == copies).all())
    # sum of the map over the tiles == agreeing bits of the whole row == (Nb + keyed score) / 2 for the same record
    reg = T.KeyedRegistry()
    reg.add("u", KEY, NONCE, msg)
    nb = 4 * 64 * 64 * l
    _, s_keyed = codec.trace_keyed_topk(packed, nb, reg.to_device("cuda"), 32, k=1)
    agree = codec.tile_agreement(packed, keys, tamper._message_rows([msg] * B, M, "cuda"), M, shape, l, tile)
    assert torch.equal(agree.sum(dim=(1, 2)) * 2, nb + s_keyed[:, 0].long())


def test_zero_and_saturated_weights(G):
    codec, tamper, T = G
    shape, l, tile, M, B = (4, 64, 64), 1, 16, 256, 2
    rng, nb, packed, recs = _operands(9, B, shape, l, M)
    p, k, m = _dev(codec, tamper, packed, recs)
    w = np.zeros((B, 4, 4), dtype=np.uint16)
    w[0, :2] = 65535                       # image 0: the upper half at full weight, the lower half silent; image 1: no weight at all
    bits, score, wsum = codec.vote_tiled(p, k, torch.from_numpy(w).cuda(), M, shape, l, tile)
    wb, ws, ww = R.vote(np.unpackbits(packed[0]), O.keystream_bits(recs[0][0], recs[0][1], nb), w[0], M, shape, l, tile)
    assert int(ww.max()) == 32 * 65535 and int(np.abs(ws).max()) > 2 ** 16
    assert np.array_equal(score[0].cpu().numpy(), ws) and np.array_equal(wsum[0].cpu().numpy(), ww) and np.array_equal(bits[0].cpu().numpy(), np.packbits(wb))
    assert int(score[1].abs().sum()) == 0 and int(wsum[1].abs().sum()) == 0 and int(bits[1].sum()) == 0


@pytest.mark.parametrize("shape,l,tile,M", [((4, 16, 24), 1, 8, 64), ((4, 64, 64), 2, 16, 256)])
def test_poisoned_guard_banded_buffers(G, shape, l, tile, M):
    """both kernels with every operand inside banded buffers and every output served pattern-filled, under both patterns: the bands stay intact,
    no int32 output element keeps the pattern, and the bits of every output are those of the clean run"""
    codec, tamper, T = G
    B = 3
    rng, nb, packed, recs = _operands(21, B, shape, l, M)
    th, tw = shape[1] // tile, shape[2] // tile
    weights = torch.from_numpy(rng.integers(0, 65536, (B, th, tw)).astype(np.uint16)).cuda()
    ops = _dev(codec, tamper, packed, recs) + (weights,)

    def run(p, k, m, w):
        return (codec.tile_agreement(p, k, m, M, shape, l, tile),) + codec.vote_tiled(p, k, w, M, shape, l, tile)

    clean = run(*ops)
    torch.cuda.synchronize()
    for pattern in (NAN, FINITE):
        L = Ledger(pattern)
        try:
            with poisoned(L):
                outs = run(*[L.wrap(t) for t in ops])
            torch.cuda.synchronize()
            L.check()
            for name, o, c in zip(("agree", "bits", "score", "wsum"), outs, clean):
                if o.element_size() > 1:
                    assert L.untouched(o) == 0, f"{name}: {L.where(o)}"
                assert torch.equal(o, c), name
        finally:
            L.release()


def test_every_refusal(G):
    codec, tamper, T = G
    shape, l, tile, M, B = (4, 16, 16), 1, 8, 64, 2
    rng, nb, packed, recs = _operands(2, B, shape, l, M)
    p, k, m = _dev(codec, tamper, packed, recs)
    w = torch.ones((B, 2, 2), dtype=torch.int16).view(torch.uint16).cuda()
    both = [lambda **kw: codec.tile_agreement(kw.get("p", p), kw.get("k", k), kw.get("m", m), kw.get("M", M), kw.get("shape", shape), kw.get("l", l), kw.get("tile", tile)),
            lambda **kw: codec.vote_tiled(kw.get("p", p), kw.get("k", k), kw.get("w", w), kw.get("M", M), kw.get("shape", shape), kw.get("l", l), kw.get("tile", tile))]
    for f in both:
        f()
        for bad_tile in (4, 12, 64, True):
            with pytest.raises(ValueError, match="tile must be one of"):
                f(tile=bad_tile)
        with pytest.raises(ValueError, match="whole number"):
            f(tile=32)                                          # 16 x 16 is not whole 32 x 32 tiles
        for bad_l in (0, 3, 8):
            with pytest.raises(ValueError, match="l must be one of"):
                f(l=bad_l)
        with pytest.raises(ValueError, match="multiple of 8"):
            f(M=60)
        with pytest.raises(ValueError, match="packed rows hold"):
            f(shape=(4, 16, 24))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(p=p.cpu())
        with pytest.raises(ValueError, match="keys must be uint8"):
            f(k=k[:, :32].contiguous())
        with pytest.raises(ValueError, match="packed must be uint8"):
            f(p=p.view(torch.int8))
    with pytest.raises(ValueError, match="messages must be uint8"):
        both[0](m=m[:1].contiguous())
    with pytest.raises(ValueError, match="weights must be uint16"):
        both[1](w=w.view(torch.int16))
    # ragged: 1024 bits do not split into 384-bit messages -> the IndexError extract_batch raises for such a length
    m48 = torch.zeros((B, 48), dtype=torch.uint8).cuda()
    with pytest.raises(IndexError, match="string index out of range"):
        both[0](M=384, m=m48)
    with pytest.raises(IndexError, match="string index out of range"):
        both[1](M=384)
    with pytest.raises(IndexError):
        codec.extract_batch(torch.zeros(B, *shape).cuda(), KEY, NONCE, 384)

    # the C ABI's own status codes (include/gswm.h), called directly
    from gswm_amd import _native as N
    lib = N.lib()
    a = torch.empty((B, 2, 2), dtype=torch.int32).cuda()
    bits, sc, ws = torch.empty((B, M // 8), dtype=torch.uint8).cuda(), torch.empty((B, M), dtype=torch.int32).cuda(), torch.empty((B, M), dtype=torch.int32).cuda()

    def agree_rc(P=p.data_ptr(), B_=B, C=4, h=16, w_=16, l_=1, t=8, K=k.data_ptr(), Mp=m.data_ptr(), M_=M, A=a.data_ptr()):
        return lib.gsw_tile_agree(P, B_, C, h, w_, l_, t, K, Mp, M_, A, None)

    def vote_rc(P=p.data_ptr(), B_=B, C=4, h=16, w_=16, l_=1, t=8, K=k.data_ptr(), W=w.data_ptr(), M_=M, b=bits.data_ptr(), s=sc.data_ptr(), x=ws.data_ptr()):
        return lib.gsw_vote_tiled(P, B_, C, h, w_, l_, t, K, W, M_, b, s, x, None)

    for rc in (agree_rc, vote_rc):
        assert rc() == N.GSW_OK
        assert rc(P=None) == rc(K=None) == rc(B_=0) == rc(l_=3) == rc(l_=0) == N.GSW_ERR_BAD_ARG
        assert rc(t=4) == rc(t=64) == rc(h=12) == rc(w_=20) == rc(M_=60) == N.GSW_ERR_UNSUPPORTED
        assert rc(C=4, h=512, w_=520) == N.GSW_ERR_UNSUPPORTED                 # 1 064 960 bits > 1 048 576
        assert rc(M_=384) == N.GSW_ERR_RAGGED
    assert agree_rc(Mp=None) == agree_rc(A=None) == N.GSW_ERR_BAD_ARG
    assert vote_rc(W=None) == vote_rc(b=None) == vote_rc(s=None) == vote_rc(x=None) == N.GSW_ERR_BAD_ARG
    assert vote_rc(C=4, h=512, w_=512, M_=8) == N.GSW_ERR_UNSUPPORTED          # 131 072 copies x 65535 does not fit int32
    torch.cuda.synchronize()


def _damaged(n_images=3):
    msg = bytes(np.random.default_rng(77).integers(0, 256, 32, dtype=np.uint8))
    return msg, R.synthetic_latents(msg, KEY, NONCE, (4, 64, 64), 1.0, 0, n_images, replaced_rows=48)


def test_extract_robust(G):
    codec, tamper, T = G
    shape, M = (4, 64, 64), 256
    msg, z64 = _damaged()
    z = torch.from_numpy(z64).cuda()
    for l in (1, 2):
        b0, f0 = codec.extract_batch(z, KEY, NONCE, M, l=l)
        bits, flags, score, wsum, agree = tamper.extract_robust(z, KEY, NONCE, M, l=l, iters=0)
        assert torch.equal(bits, b0) and torch.equal(flags, f0) and bool((wsum == 64 * l).all())
    bits, flags, score, wsum, agree = tamper.extract_robust(z, KEY, NONCE, M, iters=2)
    assert agree.shape == (3, 8, 8) and int(flags.abs().sum()) == 0
    for b in range(3):
        wb, ws, ww, wa = R.robust(R.quantise_bits(z64[b]), KEY, NONCE, M, shape, 1, 8, 2)
        assert np.array_equal(bits[b].cpu().numpy(), np.packbits(wb)) and np.array_equal(score[b].cpu().numpy(), ws)
        assert np.array_equal(wsum[b].cpu().numpy(), ww) and np.array_equal(agree[b].cpu().numpy(), wa)
    with pytest.raises(ValueError, match=r"\[B, C, h, w\]"):
        tamper.extract_robust(z.view(3, -1), KEY, NONCE, M)


def test_tamper_map_reports_the_reference_errors(G):
    codec, tamper, T = G
    msg, z64 = _damaged()
    z = torch.from_numpy(z64).cuda()
    z[1, 0, 60, 0] = 9.0
    z[2, 1, 2, 3] = float("nan")
    maps = tamper.tamper_map(z, KEY, NONCE, msg)
    assert isinstance(maps[1], ValueError) and "invalid literal" in str(maps[1]) and isinstance(maps[2], ValueError) and "NaN" in str(maps[2])
    tm = maps[0]
    assert tm.source == "message" and tm.n_t == 256 and tm.tile == 8 and tm.agree.dtype == np.int32 and tm.log10_p.shape == (8, 8)
    assert np.array_equal(tm.agree, R.tile_agree(R.quantise_bits(z64[0]), R.codeword(msg, KEY, NONCE, 16384), (4, 64, 64), 1, 8))
    assert np.array_equal(tm.intact, tm.agree >= tamper.tile_threshold(256, 64, 1e-6))
    assert tm.log10_p[0, 0] == T.log10_p_soft(2 * int(tm.agree[0, 0]) - 256, 256)


def _planted(codec, T, keyed):
    rng = np.random.default_rng(8)
    shape = (4, 64, 64)
    reg = T.KeyedRegistry() if keyed else T.Registry()
    recs = []
    for u in range(6):
        msg = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
        key, nonce = (bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8))) if keyed else (KEY, NONCE)
        recs.append((key, nonce, msg))
        reg.add(f"u{u}", key, nonce, msg) if keyed else reg.add(f"u{u}", msg)
    users = [4, 1, 2]
    z = torch.cat([codec.embed_batch(*recs[u][:2], recs[u][2], 1, shape, seed=11, image_index0=i) for i, u in enumerate(users)])
    g = torch.Generator().manual_seed(3)
    z[0, :, :40, :] = torch.randn(4, 40, 64, generator=g).cuda()           # image 0: the top 40 rows pasted over
    z[2] = torch.randn(4, 64, 64, generator=g).cuda()                       # image 2: no watermark at all -> not attributed, no map
    return reg, recs, users, z.contiguous()


@pytest.mark.parametrize("keyed", [False, True])
def test_trace_attaches_the_map_of_the_attributed_record(G, keyed):
    codec, tamper, T = G
    reg, recs, users, z = _planted(codec, T, keyed)
    plain = T.trace_latents_keyed(z, reg, k=2) if keyed else T.trace_latents(z, KEY, NONCE, reg, k=2)
    mapped = T.trace_latents_keyed(z, reg, k=2, tamper_tile=8) if keyed else T.trace_latents(z, KEY, NONCE, reg, k=2, tamper_tile=8)
    packed, _ = codec.quant_pack(z, 1)
    best = [recs[users[0]], recs[users[1]], (bytes(32), bytes(16), bytes(32))]
    want = codec.tile_agreement(packed, tamper.keys_tensor([(k, n) for k, n, _ in best], "cuda"), tamper._message_rows([m for _, _, m in best], 256, "cuda"),
                                256, (4, 64, 64), 1, 8).cpu().numpy()
    for b, (p, m) in enumerate(zip(plain, mapped)):
        assert p.tamper is None and p.candidates == m.candidates and p.attributed == m.attributed          # field by field what it is without the flag
        if b == 2:
            assert m.attributed is None and m.tamper is None
            continue
        assert m.attributed == f"u{users[b]}" and m.tamper.source == "registry" and m.tamper.log10_p is not None
        assert np.array_equal(m.tamper.agree, want[b]) and m.tamper.n_t == 256 and m.tamper.tile == 8
        assert T.format_line("x.png", m, 256) == T.format_line("x.png", p, 256) + f", intact tiles {m.tamper.n_intact}/64"
    assert mapped[0].tamper.intact[:5].sum() == 0 and mapped[0].tamper.intact[5:].all() and mapped[1].tamper.intact.all()


def test_cli_writes_the_maps(G, tmp_path, capsys):
    """Synthetic weights are not an autoencoder and the images are noise: --fpr 1 attributes every image to its best candidate so that the
    maps are written.  Only the plumbing is asserted: one .npy and one .png per image, of the stated shapes, and the line's suffix."""
    from PIL import Image
    codec, tamper, T = G
    d, maps = tmp_path / "imgs", tmp_path / "maps"
    d.mkdir()
    rng = np.random.RandomState(4)
    for i in range(2):
        Image.fromarray(rng.randint(0, 256, (80, 96, 3), dtype=np.uint8)).save(str(d / f"img{i}.png"))
    reg = T.Registry()
    for i in range(5):
        reg.add(f"u{i}", bytes(rng.randint(0, 256, 32, dtype=np.uint8)))
    reg.save(str(tmp_path / "registry.txt"))
    T.main(["--images_directory_path", str(d), "--key_hex", README_KEY, "--nonce_hex", README_NONCE, "--registry", str(tmp_path / "registry.txt"),
            "--allow_synthetic_weights", "--num_inference_steps", "2", "--width", "128", "--height", "128", "--strict_kernels", "0", "--fpr", "1.0",
            "--tamper_map", str(maps), "--tile", "8"])
    out = capsys.readouterr().out
    assert sorted(os.listdir(maps)) == ["img0.tamper.npy", "img0.tamper.png", "img1.tamper.npy", "img1.tamper.png"]
    for i in range(2):
        a = np.load(str(maps / f"img{i}.tamper.npy"))
        assert a.dtype == np.int32 and a.shape == (2, 2) and a.min() >= 0 and a.max() <= 256
        im = Image.open(str(maps / f"img{i}.tamper.png"))
        assert im.mode == "L" and im.size == (128, 128)
        assert np.array_equal(np.asarray(im)[::64, ::64] == 255, a >= tamper.tile_threshold(256, 4, 1.0))
        line = [ln for ln in out.splitlines() if ln.startswith(f"img{i}.png, user: ")]
        assert len(line) == 1 and ", intact tiles " in line[0] and line[0].endswith("/4")


def test_extract_flags_decode_robustly_and_write_the_map(G, tmp_path):
    """extract's --robust 1 and --tamper_map on latents (no model runs): the batch and the single-image decode are extract_robust's bits, the map is
    tamper_map's against --original_message_hex; with the flags off both decodes are extract_batch's, as before"""
    import types
    from gswm_amd import extract as X
    codec, tamper, T = G
    msg, z64 = _damaged()
    z = torch.from_numpy(z64).cuda().float()
    args = types.SimpleNamespace(key=KEY, nonce=NONCE, message_length=256, l=1)
    plain = [codec.bits_to_str(r) for r in codec.extract_batch(z, KEY, NONCE, 256)[0].cpu().numpy()]
    assert X.recover_exactracted_message_batch(z, args) == plain and X.recover_exactracted_message(z[:1], args) == plain[0]
    args.robust, args.tile = 1, 8
    robust = [codec.bits_to_str(r) for r in tamper.extract_robust(z, KEY, NONCE, 256)[0].cpu().numpy()]
    assert X.recover_exactracted_message_batch(z, args) == robust and X.recover_exactracted_message(z[:1], args) == robust[0]
    want = "".join(format(b, "08b") for b in msg)
    assert sum(a == b for a, b in zip(robust[0], want)) > sum(a == b for a, b in zip(plain[0], want))       # (sigma 1.0, 48 of 64 rows replaced)
    args.tamper_map, args.original_message_hex, args.width, args.height = str(tmp_path / "maps"), msg.hex(), 512, 512
    X.write_tamper_maps(z, ["/x/a.png", "/x/b.jpg", "/x/c.png"], args)
    assert sorted(os.listdir(tmp_path / "maps")) == ["a.tamper.npy", "a.tamper.png", "b.tamper.npy", "b.tamper.png", "c.tamper.npy", "c.tamper.png"]
    maps = tamper.tamper_map(z, KEY, NONCE, msg)
    assert all(np.array_equal(np.load(str(tmp_path / "maps" / f"{n}.tamper.npy")), m.agree) for n, m in zip("abc", maps))
