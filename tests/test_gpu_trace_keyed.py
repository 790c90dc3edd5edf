"""GPU: tracing against records that carry their own keys -- codec.sign_pack against the oracle's quantiser, the keyed search kernel
(codec.trace_keyed_topk) against codewords of the oracle's ChaCha20 (gs_oracle.cipher_bits / chacha20_keystream) scored on the host,
the identity with the single-key search, planted watermarks, then trace_latents_keyed and the front end on a gs_insert log.
EXACT equality of bits, flags, indices and scores everywhere, no tolerance."""
import os
import types

import numpy as np
import pytest
import torch

from conftest import README_KEY, README_NONCE

import gs_oracle as O

pytestmark = pytest.mark.gpu

KEY, NONCE = bytes.fromhex(README_KEY), bytes.fromhex(README_NONCE)
INT32_MIN = -2 ** 31


@pytest.fixture(scope="module")
def G():
    import gswm_amd
    from gswm_amd import codec, trace
    return codec, trace


# ------------------------------------------------------------------------------------------------------------ sign_pack
def _edge_scalars(dtype):
    """the values either side of the quantiser's two thresholds in this dtype, +-0, the smallest magnitudes, NaN excluded"""
    y1, y2 = -6.957291061679417e-17, 8.292361075813597
    if dtype == torch.float64:
        near = [np.nextafter(y1, -np.inf), y1, np.nextafter(y1, np.inf), np.nextafter(y2, -np.inf), y2, np.nextafter(y2, np.inf), 5e-324, -5e-324]
        return torch.tensor(near + [0.0, -0.0, 8.0, 9.0, -9.0, np.inf, -np.inf], dtype=dtype)
    t = torch.tensor([y1, y2], dtype=torch.float64).to(dtype)
    info = torch.finfo(dtype)
    out = [torch.tensor([0.0, -0.0, 8.0, 8.25, 8.3125, 8.5, 9.0, -9.0, float("inf"), float("-inf"), info.tiny, -info.tiny,
                         info.smallest_normal, -info.smallest_normal, info.max, -info.max], dtype=dtype), t]
    ints = torch.int32 if dtype == torch.float32 else torch.int16
    for step in (-2, -1, 1, 2):                                               # the neighbours of both thresholds, by bit pattern
        out.append((t.view(ints) + step).view(dtype))
    if dtype == torch.float16:
        out.append(torch.tensor([5.96e-8, -5.96e-8, 8.2890625, 8.296875], dtype=dtype))          # the smallest subnormals; the halves around y2
    if dtype == torch.bfloat16:
        out.append(torch.tensor([8.25, 8.3125, -6.9e-17, -7.0e-17, -1e-38, 1e-38], dtype=dtype))
    if dtype == torch.float32:
        out.append(torch.tensor([1e-45, -1e-45, -6.9572907e-17, -6.957292e-17, 8.29236, 8.292361, 8.292362], dtype=dtype))
    e = torch.cat(out)
    return e[~torch.isnan(e)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64])
@pytest.mark.parametrize("B,shape", [(5, (4, 64, 64)), (3, (4, 13, 10)), (2, (1, 1, 8))])
def test_sign_pack_is_the_oracles_quantiser(G, dtype, B, shape):
    codec, T = G
    n = int(np.prod(shape))
    g = torch.Generator().manual_seed(n + B)
    z = torch.randn(B, n, generator=g, dtype=torch.float64).to(dtype)
    edges = _edge_scalars(dtype)
    if n >= 4 * edges.numel():
        pos = torch.randperm(n, generator=g)[:edges.numel()]
        z[1, pos] = edges                                                     # image 1: every edge scalar (saturates)
        z[2, 0:n:3] = 0.0
        z[2, 1:n:3] = -0.0                                                    # image 2: +-0 throughout, no flag
    if B >= 4:
        z[3, n // 2] = float("nan")                                           # image 3: NaN
        z[4, 5] = float("nan")
        z[4, 6] = 9.0                                                         # image 4: both flags
    zd = z.view(B, *shape).cuda()
    signs, flags = codec.sign_pack(zd)
    assert signs.dtype == torch.uint8 and signs.shape == (B, n // 8) and flags.dtype == torch.int32 and flags.shape == (B,)
    z64 = z.double().numpy()
    nan = np.isnan(z64)
    want = np.stack([np.packbits(O.quantise(np.where(nan[b], -1.0, z64[b])).astype(np.uint8)) for b in range(B)])       # a NaN packs as 0; y == 2 as 1
    assert np.array_equal(signs.cpu().numpy(), want)
    want_flags = [(1 if (O.quantise(np.where(nan[b], -1.0, z64[b])) >= 2).any() else 0) | (2 if nan[b].any() else 0) for b in range(B)]
    assert flags.cpu().tolist() == want_flags
    assert torch.equal(flags, codec.extract_batch(zd, KEY, NONCE, 8)[1])         # extract_batch's flags on the same input


def test_sign_pack_wrapper_refuses_bad_operands(G):
    codec, T = G
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.sign_pack(torch.zeros(2, 16))
    with pytest.raises(ValueError, match="multiple of 8"):
        codec.sign_pack(torch.zeros(2, 12).cuda())
    with pytest.raises(ValueError, match="unsupported dtype"):
        codec.sign_pack(torch.zeros(2, 16, dtype=torch.int32).cuda())


# ------------------------------------------------------------------------------------------------------------ keyed search
def _records_and_codewords(rng, U, n, msg_bytes):
    """U records and their packed codewords.  Up to 4097 records: independent random keys and nonces (every tenth with the initial
    counter 0xFFFFFFFF), each codeword from gs_oracle.cipher_bits.  Larger U: eight random keys; a key's records take consecutive
    initial counters (so record j of it owns blocks j nblk .. of ONE oracle keystream, starting just below the 32-bit carry), and a
    sample is compared with cipher_bits record by record."""
    nbytes, nblk = n // 8, (n // 8 + 63) // 64
    msgs = rng.integers(0, 256, (U, msg_bytes), dtype=np.uint8)
    recs, cw = [], np.empty((U, nbytes), dtype=np.uint8)
    if U <= 4097:
        for u in range(U):
            key, nonce = bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8))
            if u % 10 == 3:
                nonce = b"\xff\xff\xff\xff" + nonce[4:]
            recs.append((key, nonce, msgs[u].tobytes()))
            cw[u] = np.packbits(O.cipher_bits(msgs[u].tobytes(), key, nonce, n))
        return recs, cw
    groups = np.array_split(np.arange(U), 8)
    for ids in groups:
        key, tail = bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 8, dtype=np.uint8))
        c0 = 0xFFFFFFFF - 5 * nblk + (int(rng.integers(0, 2 ** 31)) << 32)
        ks = np.frombuffer(O.chacha20_keystream(key, int(c0).to_bytes(8, "little") + tail, len(ids) * nblk * 64), dtype=np.uint8)
        ks = ks.reshape(len(ids), nblk * 64)[:, :nbytes]
        cw[ids] = ks ^ np.tile(msgs[ids], (1, nbytes // msg_bytes))
        recs += [(key, int(c0 + j * nblk).to_bytes(8, "little") + tail, msgs[u].tobytes()) for j, u in enumerate(ids)]
    for u in rng.choice(U, 40, replace=False).tolist() + [int(g[5]) for g in groups]:
        assert np.array_equal(cw[u], np.packbits(O.cipher_bits(recs[u][2], recs[u][0], recs[u][1], n))), u
    return recs, cw


def _rows(T, recs, msg_bytes):
    reg = T.KeyedRegistry(msg_bytes)
    for u, (key, nonce, msg) in enumerate(recs):
        reg.add(f"u{u}", key, nonce, msg)
    return reg


# U x n x msg_bytes x B x k, a sparse product: every value of each axis appears, the corners too; n = 262144 is a 2048^2 image
CASES = [(1, 8, 1, 1, 1), (2, 256, 32, 3, 4), (63, 520, 5, 64, 8), (64, 16384, 32, 130, 1), (65, 36864, 128, 1, 4), (1000, 65536, 256, 3, 8),
         (4097, 256, 8, 64, 1), (2 ** 17 + 3, 520, 5, 3, 4), (2 ** 17 + 3, 8, 1, 130, 8), (1000, 16384, 128, 64, 4), (4097, 256, 32, 130, 8),
         (65, 65536, 32, 64, 1), (63, 36864, 8, 130, 4), (2, 262144, 256, 3, 1), (1000, 256, 1, 1, 8), (64, 16384, 8, 4, 8), (2 ** 17 + 3, 256, 32, 64, 1),
         (5, 1048576, 32, 2, 4)]
# every tile (1, 4, 16, 64 images: B = 1, 2, 5, 17) x message form (dwords at 4 bytes, byte by byte at 3) of csrc/gswm_search_plan.h at the smallest lattice that has
# them (one ChaCha block, whole at 512 bits, partial at 504 = 21 x 24: 512 is no multiple of 24); 9 records: one wave takes a second record; 5 with k = 8: an empty tail
CASES += [(9 if B in (1, 5) else 5, 512 if mb == 4 else 504, mb, B, 3 if B in (1, 5) else 8) for B in (1, 2, 5, 17) for mb in (4, 3)]


@pytest.mark.parametrize("U,n,msg_bytes,B,k", CASES)
def test_keyed_search_matches_oracle_codewords(G, U, n, msg_bytes, B, k):
    codec, T = G
    rng = np.random.default_rng(U * 7 + n + msg_bytes + B)
    recs, cw = _records_and_codewords(rng, U, n, msg_bytes)
    signs = rng.integers(0, 256, (B, n // 8), dtype=np.uint8)
    signs[0] = 0x00                                                           # all sign bits 0
    if B > 1:
        signs[-1] = 0xFF                                                      # all sign bits 1
    if B > 2:
        signs[1] = cw[U // 2]                                                 # a perfect match
        signs[1, 0] ^= 0x80 if n > 8 else 0x00
    rows = _rows(T, recs, msg_bytes).to_device()
    idx, score = codec.trace_keyed_topk(torch.from_numpy(signs).cuda(), n, rows, msg_bytes, k=k)
    want_idx, want_score = T.keyed_topk_host(signs, cw, k)
    got_idx, got_score = idx.cpu().numpy(), score.cpu().numpy()
    assert got_idx.dtype == np.int32 and got_score.dtype == np.int32 and got_idx.shape == (B, k)
    assert np.array_equal(got_score, want_score), (np.argwhere(got_score != want_score)[:5], got_score[:2], want_score[:2])
    assert np.array_equal(got_idx, want_idx), (np.argwhere(got_idx != want_idx)[:5], got_idx[:2], want_idx[:2])
    if B > 2 and n > 8:
        assert got_idx[1, 0] == U // 2 and got_score[1, 0] == n - 2


def test_wider_record_stride_and_side_stream(G):
    """rows padded beyond the minimum stride; the same call twice and on a side stream"""
    codec, T = G
    rng = np.random.default_rng(8)
    U, n, mb, B = 3000, 4096, 16, 20
    recs, cw = _records_and_codewords(rng, U, n, mb)
    rows = _rows(T, recs, mb).packed()
    wide = np.full((U, 128), 0xA5, dtype=np.uint8)
    wide[:, :48 + mb] = rows[:, :48 + mb]
    signs = rng.integers(0, 256, (B, n // 8), dtype=np.uint8)
    s, r, w = torch.from_numpy(signs).cuda(), torch.from_numpy(rows).cuda(), torch.from_numpy(wide).cuda()
    a = codec.trace_keyed_topk(s, n, r, mb, k=8)
    b = codec.trace_keyed_topk(s, n, w, mb, k=8)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = codec.trace_keyed_topk(s, n, r, mb, k=8)
    side.synchronize()
    want = T.keyed_topk_host(signs, cw, 8)
    for x in (a, b, c):
        assert np.array_equal(x[0].cpu().numpy(), want[0]) and np.array_equal(x[1].cpu().numpy(), want[1])


def test_single_shared_key_equals_trace_topk(G):
    """Records that share one key: the keyed search returns codec.trace_topk(soft) on extract_batch's counts, indices and scores"""
    codec, T = G
    rng = np.random.default_rng(12)
    for shape, M, U, B, k in (((4, 64, 64), 256, 5000, 16, 8), ((4, 96, 96), 1024, 300, 5, 4), ((4, 16, 16), 64, 4097, 64, 1)):
        n, mb = int(np.prod(shape)), M // 8
        msgs = rng.integers(0, 256, (U, mb), dtype=np.uint8)
        single, keyed = T.Registry(mb), T.KeyedRegistry(mb)
        for u in range(U):
            single.add(f"u{u}", msgs[u].tobytes())
            keyed.add(f"u{u}", KEY, NONCE, msgs[u].tobytes())
        z = torch.cat([codec.embed_batch(KEY, NONCE, msgs[(37 * b) % U].tobytes(), 1, shape, seed=3, image_index0=b) for b in range(B)])
        flip = torch.from_numpy(rng.random((B, n)) < 0.35).cuda().view(z.shape)
        z = torch.where(flip, -z, z).half().contiguous()
        V = codec.vote_copies(n, M)
        counts = codec.extract_batch(z, KEY, NONCE, M, return_counts=True)[2]
        want_idx, want_score = codec.trace_topk(counts, V, single.to_device(), k=k, soft=True)
        signs, flags = codec.sign_pack(z)
        assert int(flags.abs().sum()) == 0
        idx, score = codec.trace_keyed_topk(signs, n, keyed.to_device(), mb, k=k)
        assert torch.equal(idx, want_idx) and torch.equal(score, want_score)
        assert idx[:, 0].tolist() == [(37 * b) % U for b in range(B)]


def _planted(codec, rng, B, U, shape=(4, 64, 64), mb=32):
    recs = [(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8)),
             bytes(rng.integers(0, 256, mb, dtype=np.uint8))) for _ in range(U)]
    owners = rng.choice(U, B, replace=False)
    z = torch.cat([codec.embed_batch(*recs[u], 1, shape, seed=11, image_index0=b) for b, u in enumerate(owners)])
    return recs, owners, z


def test_planted_watermarks_score_n_and_flips_cost_two_each(G):
    codec, T = G
    rng = np.random.default_rng(21)
    B, U, n = 24, 2000, 16384
    recs, owners, z = _planted(codec, rng, B, U)
    rows = _rows(T, recs, 32).to_device()
    idx, score = codec.trace_keyed_topk(codec.sign_pack(z)[0], n, rows, 32, k=2)
    assert idx[:, 0].tolist() == owners.tolist() and score[:, 0].tolist() == [n] * B
    assert int(score[:, 1].max()) < n // 8                                     # the runner-up is another key: an unrelated codeword
    f = [0, 1, 7, 100, 1000, 4096, 8191, 8192] * 3
    flat = z.view(B, n).clone()
    for b in range(B):
        pos = torch.from_numpy(rng.choice(n, f[b], replace=False)).cuda()
        flat[b, pos] = -flat[b, pos]
    idx2, score2 = codec.trace_keyed_topk(codec.sign_pack(flat.view_as(z).contiguous())[0], n, rows, 32, k=1)
    own = torch.from_numpy(owners).cuda()
    scores_of_owner = [n - 2 * x for x in f]
    for b in range(B):
        if f[b] < 8000:                                                        # (at half the lattice flipped the owner scores ~0 and need not win)
            assert int(idx2[b, 0]) == int(own[b]) and int(score2[b, 0]) == scores_of_owner[b]
        else:
            single = rows[int(own[b]):int(own[b]) + 1].clone()
            s1 = codec.trace_keyed_topk(codec.sign_pack(flat.view_as(z).contiguous())[0][b:b + 1].clone(), n, single, 32, k=1)[1]
            assert int(s1[0, 0]) == scores_of_owner[b]


def test_two_halves_merged_on_the_host_equal_one_call(G):
    codec, T = G
    rng = np.random.default_rng(31)
    U, n, mb, B, k = 7001, 2048, 32, 40, 8
    recs, cw = _records_and_codewords(rng, U, n, mb)
    rows = _rows(T, recs, mb).to_device()
    signs = torch.from_numpy(rng.integers(0, 256, (B, n // 8), dtype=np.uint8)).cuda()
    signs[3] = torch.from_numpy(cw[6000]).cuda()
    whole = [t.cpu().numpy() for t in codec.trace_keyed_topk(signs, n, rows, mb, k=k)]
    h = 3333
    lo = [t.cpu().numpy() for t in codec.trace_keyed_topk(signs, n, rows[:h], mb, k=k)]
    hi = [t.cpu().numpy() for t in codec.trace_keyed_topk(signs, n, rows[h:], mb, k=k)]
    for b in range(B):
        both = sorted([(-int(s), int(i)) for i, s in zip(lo[0][b], lo[1][b])] + [(-int(s), int(i) + h) for i, s in zip(hi[0][b], hi[1][b])])[:k]
        assert [i for _, i in both] == whole[0][b].tolist() and [-s for s, _ in both] == whole[1][b].tolist()
    assert whole[0][3, 0] == 6000 and whole[1][3, 0] == n


def test_keyed_wrapper_refuses_bad_operands(G):
    codec, T = G
    s = torch.zeros(2, 32, dtype=torch.uint8).cuda()
    r = torch.zeros(10, 80, dtype=torch.uint8).cuda()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.trace_keyed_topk(s.cpu(), 256, r, 32)
    with pytest.raises(ValueError, match="n_bits"):
        codec.trace_keyed_topk(s, 512, r, 32)
    with pytest.raises(ValueError, match="record rows"):
        codec.trace_keyed_topk(s, 256, r[:, :64].contiguous(), 32)
    with pytest.raises(ValueError, match="msg_bytes"):
        codec.trace_keyed_topk(s, 256, r, 0)
    with pytest.raises(ValueError):
        codec.trace_keyed_topk(s, 256, r, 32, k=9)
    with pytest.raises(ValueError):
        codec.trace_keyed_topk(s.int(), 256, r, 32)
    with pytest.raises(IndexError):
        codec.trace_keyed_topk(s, 256, r, 24)                                  # 256 bits are not a multiple of 192


# ------------------------------------------------------------------------------------------------------------ end to end
def _issue_log(tmp_path, messages):
    """one gs_insert call per message with blank key and nonce: a fresh random key and nonce per call, logged to info_data.txt"""
    from gswm_amd import gs_insert
    log = tmp_path / "info_data.txt"
    opt = types.SimpleNamespace(key_hex="", nonce_hex="")
    np.random.seed(1234)
    z = np.stack([gs_insert.gs_watermark_init_noise(opt, m, log_path=str(log)) for m in messages])
    return log, torch.from_numpy(z).cuda()


def test_trace_latents_keyed_end_to_end(G, tmp_path):
    codec, T = G
    messages = ["alice", "bob", "carol", "alice", "dave"]                      # 'alice' twice: two records, two keys
    log, z = _issue_log(tmp_path, messages)
    reg = T.KeyedRegistry.from_info_data(log)
    assert reg.user_ids == [f"info:{i}" for i in range(1, 6)] and reg.n_keys == 5
    assert T.detect_format(log) == "info_data"
    with pytest.raises(ValueError, match="no record"):
        T.Registry.from_info_data(log, KEY, NONCE)                             # no tool for this log without per-record keys
    n, M = 16384, 256
    limit = np.log10(1e-6)
    for zz in (z, z.float(), z.half()):
        res = T.trace_latents_keyed(zz, reg, k=3)
        for b, r in enumerate(res):
            top = r.candidates[0]
            assert r.attributed == f"info:{b + 1}" == top.user_id and top.index == b and top.score == n and top.agree == M
            assert top.log10_p_any == T.log10_p_any(T.log10_p_soft(n, n), 5) <= limit
            assert len(r.candidates) == 3 and all(c.log10_p_any > limit for c in r.candidates[1:])
            for c in r.candidates[1:]:                                          # agreement under the candidate's OWN key, as the reference counts it
                key, nonce, msg = reg.record_at(c.index)
                assert c.agree == sum(x == y for x, y in zip(O.recover_bits(zz[b].double().cpu().numpy(), key, nonce, M), codec.bits_to_str(msg)))
    # noisy: a third of the signs flipped still attributes
    g = torch.Generator().manual_seed(9)
    noisy = torch.where((torch.rand(z.shape, generator=g) < 0.33).cuda(), -z, z).float().contiguous()
    assert [r.attributed for r in T.trace_latents_keyed(noisy, reg)] == [f"info:{i}" for i in range(1, 6)]
    # unwatermarked latents: nobody, and the host agrees on index and score
    noise = torch.randn(8, 4, 64, 64, generator=torch.Generator().manual_seed(5)).cuda()
    res = T.trace_latents_keyed(noise, reg)
    cw = np.stack([np.packbits(O.cipher_bits(m, k_, n_, n)) for k_, n_, m in (reg.record_at(i) for i in range(5))])
    h = np.stack([np.packbits(O.quantise(noise[b].cpu().numpy()).astype(np.uint8)) for b in range(8)])
    wi, ws = T.keyed_topk_host(h, cw, 1)
    assert all(r.attributed is None for r in res)
    assert [r.candidates[0].index for r in res] == wi[:, 0].tolist() and [r.candidates[0].score for r in res] == ws[:, 0].tolist()
    assert all(T.format_line(f"{b}.png", r, M).startswith(f"{b}.png, user: none, agreement, ") for b, r in enumerate(res))
    # the reference's errors
    bad = z.float().clone()
    bad[1, 0, 0, 0] = 9.0
    bad[2, 1, 2, 3] = float("nan")
    out = T.trace_latents_keyed(bad, reg)
    assert out[0].attributed == "info:1" and out[3].attributed == "info:4"
    assert isinstance(out[1], ValueError) and "invalid literal for int() with base 2" in str(out[1])
    assert isinstance(out[2], ValueError) and "NaN" in str(out[2])
    with pytest.raises(IndexError):
        T.trace_latents_keyed(torch.zeros(1, 4, 10, 10).cuda(), reg)           # 400 lattice bits, 256-bit messages


def test_cli_per_record_keys(G, tmp_path, monkeypatch, capsys):
    """The front end on a gs_insert log.  Synthetic weights are not an autoencoder, so the inversion is replaced by the latents that
    were issued (two images) and seeded noise (the third): the rest -- registry, search, statistics, trace.txt -- is the real run."""
    from PIL import Image
    from gswm_amd import extract as X
    codec, T = G
    log, z = _issue_log(tmp_path, ["first user", "second user", "third user"])
    d = tmp_path / "imgs"
    d.mkdir()
    rng = np.random.RandomState(4)
    for i in range(3):
        Image.fromarray(rng.randint(0, 256, (80, 96, 3), dtype=np.uint8)).save(str(d / f"img{i}.png"))
    (d / "broken.png").write_bytes(b"not an image")
    latents = torch.cat([z[2:3].float(), z[0:1].float(), torch.randn(1, 4, 64, 64, generator=torch.Generator().manual_seed(5)).cuda()])
    calls = []

    def fake_inversion(arrs, args, **kw):
        calls.append(len(arrs))
        return latents[:len(arrs)].clone()

    monkeypatch.setattr(X, "invert_decoded_images", fake_inversion)
    T.main(["--images_directory_path", str(d), "--per_record_keys", "--registry", str(log), "--allow_synthetic_weights", "--num_inference_steps", "3",
            "--width", "128", "--height", "128", "--strict_kernels", "0", "--top", "2", "--fpr", "1e-6"])
    out = capsys.readouterr().out
    assert calls == [3]
    lines = (d / "trace.txt").read_text().splitlines()
    start = lines.index("=" * 40 + "Batch Start" + "=" * 40)
    info = dict(l.split(",", 1) for l in lines[1:start])
    assert info["keys"] == "3" and info["users"] == "3" and info["statistic"] == "soft" and info["key_hex"] == "per record" and info["message_length"] == "256"
    assert lines[start + 1].startswith("SYNTHETIC WEIGHTS,")
    body = lines[start + 2:-1]
    files = X._DirJob(str(d)).files
    assert len(body) == len(files) == 4
    reg = T.KeyedRegistry.from_info_data(log)
    want = iter(T.trace_latents_keyed(latents, reg, k=2))
    users = iter(["info:3", "info:1", "none"])
    for f, line in zip(files, body):
        if f.endswith("broken.png"):
            assert line.startswith(f"Error processing {f}: ")
        else:
            assert line == T.format_line(os.path.basename(f), next(want), 256)
            assert line.startswith(f"{os.path.basename(f)}, user: {next(users)}, agreement, ")
        assert line in out
    with pytest.raises(SystemExit):
        T.main(["--images_directory_path", str(d), "--per_record_keys", "--registry", str(log), "--hard"])
    assert "--hard" in capsys.readouterr().err


def test_cli_per_record_keys_through_the_real_inversion(G, tmp_path, monkeypatch, capsys):
    """Plumbing only (synthetic weights recover nothing): the front end decodes, inverts and traces for real; trace.txt equals
    trace_latents_keyed on the very latents the run inverted."""
    from PIL import Image
    from gswm_amd import extract as X
    codec, T = G
    log, _ = _issue_log(tmp_path, ["first user", "second user", "third user"])
    d = tmp_path / "imgs"
    d.mkdir()
    rng = np.random.RandomState(4)
    for i in range(3):
        Image.fromarray(rng.randint(0, 256, (80, 96, 3), dtype=np.uint8)).save(str(d / (f"img{i}.png" if i != 1 else f"img{i}.jpg")))
    (d / "broken.png").write_bytes(b"not an image")
    seen = []
    real = X.invert_decoded_images

    def spy(arrs, args, **kw):
        lat = real(arrs, args, **kw)
        seen.append(lat.clone())
        return lat

    monkeypatch.setattr(X, "invert_decoded_images", spy)
    T.main(["--images_directory_path", str(d), "--per_record_keys", "--registry", str(log), "--allow_synthetic_weights", "--num_inference_steps", "3",
            "--width", "512", "--height", "512", "--strict_kernels", "0", "--top", "3"])
    out = capsys.readouterr().out
    assert len(seen) == 1 and seen[0].shape == (3, 4, 64, 64)
    lines = (d / "trace.txt").read_text().splitlines()
    start = lines.index("=" * 40 + "Batch Start" + "=" * 40)
    assert "keys,3" in lines[1:start] and lines[start + 1].startswith("SYNTHETIC WEIGHTS,")
    body = lines[start + 2:-1]
    files = X._DirJob(str(d)).files
    assert len(body) == len(files) == 4
    want = iter(T.trace_latents_keyed(seen[0], T.KeyedRegistry.from_info_data(log), k=3))
    for f, line in zip(files, body):
        if f.endswith("broken.png"):
            assert line.startswith(f"Error processing {f}: ")
        else:
            assert line == T.format_line(os.path.basename(f), next(want), 256)
        assert line in out
