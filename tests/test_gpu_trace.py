"""GPU: the registry search kernel (codec.trace_topk) against the NumPy restatement trace.topk_host -- EXACT equality of indices and
scores, no tolerance -- then trace_latents end to end on the codec (no UNet) and the `python -m gswm_amd.trace` front end."""
import os

import numpy as np
import pytest
import torch

from conftest import README_KEY, README_NONCE

pytestmark = pytest.mark.gpu

KEY, NONCE = bytes.fromhex(README_KEY), bytes.fromhex(README_NONCE)


@pytest.fixture(scope="module")
def G():
    import gswm_amd
    from gswm_amd import codec, trace
    return codec, trace


def _case(U, M, B, V, seed, extremes=True):
    rng = np.random.default_rng(seed)
    reg = rng.integers(0, 256, (U, M // 8), dtype=np.uint8)
    counts = rng.integers(0, V + 1, (B, M)).astype(np.int32)
    if extremes:
        counts[0] = 0                                  # all votes '0'
        if B > 1:
            counts[-1] = V                             # all votes '1'
    return counts, reg


def _check(G, counts, reg, V, k, soft):
    codec, T = G
    idx, score = codec.trace_topk(torch.from_numpy(counts).cuda(), V, torch.from_numpy(reg).cuda(), k=k, soft=soft)
    want_idx, want_score = T.topk_host(counts, V, reg, k, soft)
    got_idx, got_score = idx.cpu().numpy(), score.cpu().numpy()
    assert got_idx.dtype == np.int32 and got_score.dtype == np.int32 and got_idx.shape == (counts.shape[0], k)
    assert np.array_equal(got_score, want_score), (np.argwhere(got_score != want_score)[:5], got_score[:2], want_score[:2])
    assert np.array_equal(got_idx, want_idx), (np.argwhere(got_idx != want_idx)[:5], got_idx[:2], want_idx[:2])


# U x M x B, a sparse product: every value of each axis appears, the corners (one user, one image, widest message, largest batch) too
SHAPES = [(1, 8, 1), (2, 64, 3), (63, 200, 64), (64, 256, 130), (65, 1024, 1), (1000, 2048, 3), (4097, 256, 64), (2 ** 17 + 3, 256, 64),
          (2 ** 17 + 3, 8, 3), (1000, 200, 130), (4097, 1024, 64), (65, 2048, 64), (1, 2048, 130), (2, 256, 1), (63, 64, 130), (64, 1024, 3),
          (4097, 64, 1), (2 ** 17 + 3, 1024, 3)]


@pytest.mark.parametrize("U,M,B", SHAPES)
def test_soft_one_plane_matches_host(G, U, M, B):
    for i, V in enumerate((1, 16, 64, 127)):
        k = (1, 4, 8)[(i + U + B) % 3]
        counts, reg = _case(U, M, B, V, seed=U * 31 + M + B + V)
        _check(G, counts, reg, V, k, True)


@pytest.mark.parametrize("U,M,B", SHAPES[:12])
def test_soft_beyond_int8_is_exact(G, U, M, B):
    for i, V in enumerate((128, 144, 256, 2047)):
        k = (8, 1, 4)[(i + U + B) % 3]
        counts, reg = _case(U, M, B, V, seed=U * 17 + M + B + V)
        _check(G, counts, reg, V, k, True)


def test_soft_three_planes(G):
    counts, reg = _case(1000, 64, 3, 100000, seed=5)           # M V = 6.4e6: the third base-128 digit is in use
    _check(G, counts, reg, 100000, 4, True)


@pytest.mark.parametrize("U,M,B", SHAPES[:12])
def test_hard_matches_host(G, U, M, B):
    for i, V in enumerate((1, 4, 5, 64, 144, 2047)):            # even V: counts == V / 2 are ties, which vote 0
        k = (4, 8, 1)[(i + U + B) % 3]
        counts, reg = _case(U, M, B, V, seed=U * 13 + M + B + V)
        if V % 2 == 0:
            counts[:, ::3] = V // 2
        _check(G, counts, reg, V, k, False)


def test_hard_score_is_bit_matches(G):
    codec, T = G
    V, M = 64, 256
    counts, reg = _case(300, M, 5, V, seed=9, extremes=False)
    idx, score = codec.trace_topk(torch.from_numpy(counts).cuda(), V, torch.from_numpy(reg).cuda(), k=1, soft=False)
    voted = np.packbits((2 * counts > V).astype(np.uint8), axis=1)
    bits = torch.from_numpy(voted).cuda()
    for b in range(5):
        u = int(idx[b, 0])
        agree = int(codec.bit_matches(bits[b:b + 1].contiguous().clone(), M, reg[u].tobytes())[0])
        assert int(score[b, 0]) == 2 * agree - M


def test_ties_at_scale_lowest_indices_in_order(G):
    """Many equal-score rows spread over the ranges of different workgroups: the k lowest indices, in order"""
    codec, T = G
    U, M, V, B = 2 ** 17 + 3, 256, 64, 4
    rng = np.random.default_rng(3)
    reg = rng.integers(0, 256, (U, M // 8), dtype=np.uint8)
    best = rng.integers(0, 256, M // 8, dtype=np.uint8)
    winners = np.sort(rng.choice(U, 40, replace=False))
    reg[winners] = best                                          # 40 identical rows, far apart
    counts = rng.integers(0, V + 1, (B, M)).astype(np.int32)
    counts[0] = np.unpackbits(best).astype(np.int32) * V          # image 0 matches them perfectly
    counts[1] = V // 2                                            # image 1: all margins 0 -> every user ties at score 0
    _check(G, counts, reg, V, 8, True)
    _check(G, counts, reg, V, 8, False)
    idx, score = codec.trace_topk(torch.from_numpy(counts).cuda(), V, torch.from_numpy(reg).cuda(), k=8, soft=True)
    assert idx[0].tolist() == winners[:8].tolist() and score[0].tolist() == [M * V] * 8
    assert idx[1].tolist() == list(range(8)) and score[1].tolist() == [0] * 8


def test_large_registry_sampled_floor(G):
    """Registries of 2^19 rows and more are searched with a per-image floor taken from a sample of the rows: same answer, also when
    the best rows lie outside the sample, when everything ties, and in every plane / mode"""
    U, M, B = 2 ** 19 + 5, 64, 20
    for V, k, soft in ((64, 8, True), (144, 3, True), (5, 8, False)):
        counts, reg = _case(U, M, B, V, seed=V)
        target = np.packbits((2 * counts[3] > V).astype(np.uint8))
        reg[[U - 1, U - 77, 40000, U // 2]] = target                  # the winners of image 3: two in the last rows, far beyond the sample
        counts[5] = V // 2 if V % 2 == 0 else counts[5]                # an image whose scores all tie (soft, even V)
        _check(G, counts, reg, V, k, soft)


def test_same_call_twice_and_on_a_side_stream(G):
    codec, T = G
    counts, reg = _case(50000, 256, 64, 64, seed=11)
    c, r = torch.from_numpy(counts).cuda(), torch.from_numpy(reg).cuda()
    a = codec.trace_topk(c, 64, r, k=8)
    b = codec.trace_topk(c, 64, r, k=8)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d = codec.trace_topk(c, 64, r, k=8)
    s.synchronize()
    for x, y in ((a, b), (a, d)):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    want = T.topk_host(counts, 64, reg, 8, True)
    assert np.array_equal(a[0].cpu().numpy(), want[0]) and np.array_equal(a[1].cpu().numpy(), want[1])


def test_unaligned_registry_view(G):
    """rows of 25 bytes (M = 200) are never 8-byte aligned: the byte-wise loader"""
    counts, reg = _case(777, 200, 20, 16, seed=2)
    _check(G, counts, reg, 16, 4, True)


def test_wrapper_refuses_bad_operands(G):
    codec, T = G
    c = torch.zeros(2, 256, dtype=torch.int32).cuda()
    r = torch.zeros(10, 32, dtype=torch.uint8).cuda()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.trace_topk(c.cpu(), 64, r)
    with pytest.raises(ValueError):
        codec.trace_topk(c, 64, r[:, :16].contiguous())
    with pytest.raises(ValueError):
        codec.trace_topk(c, 64, r, k=9)
    with pytest.raises(ValueError):
        codec.trace_topk(c.float(), 64, r)


# ------------------------------------------------------------------------------------------------------------ end to end on the codec
def _end_to_end_inputs(T, codec):
    rng = np.random.default_rng(2024)
    U, B, shape = 4096, 16, (4, 64, 64)
    msgs = rng.integers(0, 256, (U, 32), dtype=np.uint8)
    reg = T.Registry()
    for u in range(U):
        reg.add(f"user{u:04d}", msgs[u].tobytes())
    users = rng.choice(U, B, replace=False)
    flip = rng.random((B, 4 * 64 * 64)) < 0.30
    return reg, msgs, users, flip, shape


def test_trace_latents_end_to_end(G):
    codec, T = G
    reg, msgs, users, flip, shape = _end_to_end_inputs(T, codec)
    B, M = len(users), 256
    z = torch.cat([codec.embed_batch(KEY, NONCE, msgs[u].tobytes(), 1, shape, seed=7, image_index0=i) for i, u in enumerate(users)])
    z = torch.where(torch.from_numpy(flip).cuda().view(z.shape), -z, z).contiguous()
    V = codec.vote_copies(z[0].numel(), M)
    assert V == 64

    # what the CPU says about these very inputs: host top-k + statistics alone must attribute every image to its user
    bits, flags, counts = codec.extract_batch(z, KEY, NONCE, M, return_counts=True)
    assert int(flags.abs().sum()) == 0
    counts_h = counts.cpu().numpy()
    want_idx, want_score = T.topk_host(counts_h, V, reg.packed(), 2, True)
    limit = np.log10(1e-6)
    for b in range(B):
        assert want_idx[b, 0] == users[b]
        assert T.log10_p_any(T.log10_p_soft(int(want_score[b, 0]), M * V), len(reg)) <= limit
        assert want_score[b, 1] < want_score[b, 0] // 3      # (the runner-up of a WATERMARKED image is not null either: random messages share bits)

    got = T.trace_latents(z, KEY, NONCE, reg, k=2)
    for b, r in enumerate(got):
        assert r.attributed == f"user{users[b]:04d}"
        assert [c.index for c in r.candidates] == want_idx[b].tolist() and [c.score for c in r.candidates] == want_score[b].tolist()
        top = r.candidates[0]
        assert top.agree == int(codec.bit_matches(bits[b:b + 1].clone(), M, msgs[users[b]].tobytes())[0])
        assert top.log10_p_any == T.log10_p_any(T.log10_p_soft(top.score, M * V), len(reg))

    # hard statistic: same users here (30 % flips leave the majority intact)
    hard = T.trace_latents(z, KEY, NONCE, reg, soft=False)
    hi, hs = T.topk_host(counts_h, V, reg.packed(), 1, False)
    for b, r in enumerate(hard):
        assert r.candidates[0].index == hi[b, 0] and r.candidates[0].score == hs[b, 0] == 2 * r.candidates[0].agree - M
        expect = T.log10_p_any(T.log10_p_hard(r.candidates[0].agree, M, V), len(reg)) <= limit
        assert (r.attributed is not None) == expect and hi[b, 0] == users[b]

    # unwatermarked latents: nobody
    g = torch.Generator().manual_seed(5)
    noise = torch.randn(B, *shape, generator=g).cuda()
    nc = codec.extract_batch(noise, KEY, NONCE, M, return_counts=True)[2].cpu().numpy()
    ni, ns = T.topk_host(nc, V, reg.packed(), 1, True)
    assert all(T.log10_p_any(T.log10_p_soft(int(s), M * V), len(reg)) > limit for s in ns[:, 0])      # the CPU verdict on these inputs
    res = T.trace_latents(noise, KEY, NONCE, reg)
    assert all(r.attributed is None for r in res)
    assert [r.candidates[0].index for r in res] == ni[:, 0].tolist() and [r.candidates[0].score for r in res] == ns[:, 0].tolist()


def test_trace_latents_message_length_multiple(G):
    """A 256-bit registry traced at message_length 1024: the soft scores are those at 256 (the margins of the repeats add up)"""
    codec, T = G
    reg, msgs, users, flip, shape = _end_to_end_inputs(T, codec)
    z = torch.cat([codec.embed_batch(KEY, NONCE, msgs[u].tobytes(), 1, shape, seed=7, image_index0=i) for i, u in enumerate(users[:4])])
    a = T.trace_latents(z, KEY, NONCE, reg, k=3)
    b = T.trace_latents(z, KEY, NONCE, reg, k=3, message_length=1024)
    for x, y in zip(a, b):
        assert [(c.index, c.score) for c in x.candidates] == [(c.index, c.score) for c in y.candidates]
        assert x.attributed == y.attributed and y.candidates[0].agree == 1024
    with pytest.raises(ValueError, match="multiple"):
        T.trace_latents(z, KEY, NONCE, reg, message_length=384)


def test_trace_latents_reports_the_reference_errors(G):
    codec, T = G
    reg = T.Registry()
    reg.add("a", "lthero")
    reg.add("b", "someone else")
    z = codec.embed_batch(KEY, NONCE, reg.message("a"), 3, (4, 64, 64), seed=1)
    z[1, 0, 0, 0] = 9.0                    # norm.cdf saturates: int(y) == 2 (extract.py:84-86)
    z[2, 1, 2, 3] = float("nan")
    out = T.trace_latents(z, KEY, NONCE, reg)
    assert out[0].attributed == "a" and out[0].candidates[0].agree == 256
    assert isinstance(out[1], ValueError) and "invalid literal for int() with base 2" in str(out[1])
    assert isinstance(out[2], ValueError) and "NaN" in str(out[2])


# ------------------------------------------------------------------------------------------------------------ front end
def test_cli_writes_trace_txt(G, tmp_path, monkeypatch, capsys):
    """Synthetic weights are not an autoencoder: this checks plumbing and format (trace.txt == trace_latents on the very latents the run
    inverted), not recovery."""
    from PIL import Image
    from gswm_amd import extract as X
    codec, T = G
    d = tmp_path / "imgs"
    d.mkdir()
    rng = np.random.RandomState(4)
    for i in range(3):
        Image.fromarray(rng.randint(0, 256, (80, 96, 3), dtype=np.uint8)).save(str(d / (f"img{i}.png" if i != 1 else f"img{i}.jpg")))
    (d / "broken.png").write_bytes(b"not an image")
    reg = T.Registry()
    for i in range(100):
        reg.add(f"u{i}", bytes(rng.randint(0, 256, 32, dtype=np.uint8)))
    reg_path = tmp_path / "registry.txt"
    reg.save(str(reg_path))

    seen = []
    real = X.invert_decoded_images

    def spy(arrs, args, **kw):
        lat = real(arrs, args, **kw)
        seen.append(lat.clone())
        return lat

    monkeypatch.setattr(X, "invert_decoded_images", spy)
    T.main(["--images_directory_path", str(d), "--key_hex", README_KEY, "--nonce_hex", README_NONCE, "--registry", str(reg_path), "--allow_synthetic_weights",
            "--num_inference_steps", "3", "--width", "128", "--height", "128", "--strict_kernels", "0", "--top", "2"])
    out = capsys.readouterr().out
    assert len(seen) == 1 and seen[0].shape == (3, 4, 16, 16)
    lines = (d / "trace.txt").read_text().splitlines()
    assert lines[0] == "=" * 40 + "Batch Info" + "=" * 40 and lines[-1] == "=" * 40 + "Batch End" + "=" * 40
    start = lines.index("=" * 40 + "Batch Start" + "=" * 40)
    assert lines[start + 1].startswith("SYNTHETIC WEIGHTS,")
    body = lines[start + 2:-1]
    files = X._DirJob(str(d)).files
    assert len(body) == len(files) == 4
    want = iter(T.trace_latents(seen[0], KEY, NONCE, reg, k=2))
    for f, line in zip(files, body):
        if f.endswith("broken.png"):
            assert line.startswith(f"Error processing {f}: ")
        else:
            assert line == T.format_line(os.path.basename(f), next(want), 256)
            assert line.startswith(os.path.basename(f) + ", user: ") and ", agreement, " in line and ", log10 p, " in line
        assert line in out
