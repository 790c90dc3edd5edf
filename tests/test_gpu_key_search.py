"""GPU: blind detection -- the key search kernel (codec.key_search_topk) bit for bit against the NumPy restatement of tests/key_search_reference.py
on poisoned, guard-banded buffers (tests/poison.py), ties, the identity with the keyed registry search on the device's own voted message, then
detect_latents end to end under noise and the front end.  EXACT equality of indices, statistics and messages everywhere, no tolerance."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import gs_oracle as O
import key_search_reference as R
from poison import FINITE, NAN, Ledger, poisoned

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gswm_amd  # noqa: F401
    from gswm_amd import codec, detect, trace
    return codec, detect, trace


def _pairs(rng, K):
    """K random (key, nonce) pairs; every seventh starts at the 32-bit counter's last value (the carry goes into the next word)"""
    out = []
    for u in range(K):
        key, nonce = bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8))
        if u % 7 == 3:
            nonce = b"\xff\xff\xff\xff" + nonce[4:]
        out.append((key, nonce))
    return out


def _key_rows(rng, pairs, stride):
    """uint8 [K, stride]: key | nonce, garbage after byte 48"""
    rows = rng.integers(0, 256, (len(pairs), stride), dtype=np.uint8)
    for u, (key, nonce) in enumerate(pairs):
        rows[u, :48] = np.frombuffer(key + nonce, dtype=np.uint8)
    return rows


def _poisoned_search(codec, signs, n_bits, rows, mb, k, want):
    """the search under both patterns, operands wrapped: no band written, every output element written, the restatement's result"""
    s_dev, r_dev = torch.from_numpy(signs).cuda(), torch.from_numpy(rows).cuda()
    for name, pattern in (("NAN", NAN), ("FINITE", FINITE)):
        L = Ledger(pattern)
        try:
            with poisoned(L):
                idx, stat = codec.key_search_topk(L.wrap(s_dev), n_bits, L.wrap(r_dev), mb, k=k)
            torch.cuda.synchronize()
            L.check()
            for what, t in (("idx", idx), ("stat", stat)):
                assert L.untouched(t) == 0, f"{what}: never written ({name} run) -- {L.where(t)}"
            got_idx, got_stat = idx.cpu().numpy(), stat.cpu().numpy()
        finally:
            L.release()
        assert got_idx.dtype == np.int32 and got_stat.dtype == np.int32 and got_idx.shape == (signs.shape[0], k)
        assert np.array_equal(got_stat, want[1]), (name, np.argwhere(got_stat != want[1])[:5], got_stat[:2], want[1][:2])
        assert np.array_equal(got_idx, want[0]), (name, np.argwhere(got_idx != want[0])[:5], got_idx[:2], want[0][:2])


# n_bits x msg_bytes x B x keys x k x key_stride, a sparse product: every value of each axis appears; both counting paths (msg_bytes % 4 == 0: the
# bit-sliced counters, else bit by bit) at B = 1, 3, 17 and 70.  144 bits: one partial ChaCha block; 576: two, the last partial; k > keys twice.
CASES = [(144, 3, 1, 1, 1, 48), (144, 6, 3, 5, 3, 64), (144, 18, 17, 64, 8, 80), (256, 1, 70, 257, 1, 48), (256, 4, 1, 5, 8, 64),
         (256, 32, 3, 3001, 3, 48), (576, 8, 17, 64, 1, 80), (576, 9, 70, 5, 3, 48), (576, 24, 3, 257, 8, 64), (576, 72, 1, 64, 3, 48),
         (1024, 16, 70, 64, 8, 48), (1024, 128, 17, 5, 1, 64), (16384, 32, 17, 257, 3, 48), (16384, 32, 70, 5, 8, 80), (16384, 256, 3, 64, 8, 80),
         # beyond the issue's list: 4096 and more copies (16 counter planes); the largest lattice whose row shares the LDS with a keystream; rows
         # read from global memory, both counting paths
         (131072, 4, 1, 3, 1, 48), (523264, 4, 2, 2, 3, 64), (1048576, 32, 2, 3, 3, 48), (1044480, 255, 1, 2, 2, 48),
         # the plan classes of csrc/gswm_search_plan.h the cases above do not launch: 16, 256 and 4095 copies of a 4-byte message (8 and 12 counter planes, at
         # their first and last count); the first lattice past 523 264 bits (rows read from global memory, the word path); a tile of 16 images on the bit-by-bit
         # path with a partial block (504 = 21 x 24 bits) and k past the keys; one key per step with grid_x at its cap of 512
         (512, 4, 2, 9, 8, 48), (8192, 4, 5, 9, 3, 64), (131040, 4, 1, 5, 8, 48), (523296, 4, 1, 2, 1, 48), (504, 3, 5, 5, 8, 48), (4096, 256, 3, 600, 1, 48)]


@pytest.mark.parametrize("n_bits,mb,B,K,k,stride", CASES)
def test_key_search_matches_the_restatement(G, n_bits, mb, B, K, k, stride):
    codec, D, T = G
    rng = np.random.default_rng(n_bits + 7 * mb + 31 * B + K)
    pairs = _pairs(rng, K)
    signs = rng.integers(0, 256, (B, n_bits // 8), dtype=np.uint8)
    ks = R.keystreams(pairs, n_bits)
    signs[0] = ks[K // 2]                                                      # decrypts to all zeros under that key: every position unanimous
    if B > 2:
        signs[1] = 0x00
        signs[-1] = 0xFF
    want = R.topk(R.stats(signs, ks, mb), k)
    assert want[1][0, 0] == n_bits                                             # (with one copy every key scores n_bits, the lowest index wins)
    _poisoned_search(codec, signs, n_bits, _key_rows(rng, pairs, stride), mb, k, want)


def test_key_search_on_quant_pack_rows_at_l_4(G):
    """65536 bits from quant_pack(z, 4), 32-byte messages: 256 copies, twelve counter planes"""
    codec, D, T = G
    rng = np.random.default_rng(65536)
    z = torch.randn(3, 4, 64, 64, generator=torch.Generator().manual_seed(4)).half().cuda()
    packed, flags = codec.quant_pack(z, 4)
    assert tuple(packed.shape) == (3, 8192) and int(flags.abs().sum()) == 0
    pairs = _pairs(rng, 5)
    signs = packed.cpu().numpy()
    want = R.topk(R.stats(signs, R.keystreams(pairs, 65536), 32), 1)
    _poisoned_search(codec, signs, 65536, _key_rows(rng, pairs, 48), 32, 1, want)


def test_ties_go_to_the_lower_index(G):
    codec, D, T = G
    rng = np.random.default_rng(77)
    a, b, c = _pairs(rng, 3)
    pairs = [a, b, a, c, b, a, a]
    signs = rng.integers(0, 256, (3, 128), dtype=np.uint8)
    want = R.topk(R.stats(signs, R.keystreams(pairs, 1024), 16), 7)
    for row in range(3):                                                       # equal rows are adjacent in the result, ascending
        order = want[0][row].tolist()
        assert order.index(0) < order.index(2) < order.index(5) < order.index(6) and order.index(1) < order.index(4)
    _poisoned_search(codec, signs, 1024, _key_rows(rng, pairs, 48), 16, 7, want)
    # one copy: |2 c - 1| = 1 at every position, every key scores n_bits
    pairs = _pairs(rng, 10)
    signs = rng.integers(0, 256, (4, 32), dtype=np.uint8)
    idx, stat = codec.key_search_topk(torch.from_numpy(signs).cuda(), 256, torch.from_numpy(_key_rows(rng, pairs, 48)).cuda(), 32, k=8)
    assert idx.cpu().tolist() == [list(range(8))] * 4 and stat.cpu().tolist() == [[256] * 8] * 4


def test_unaligned_sign_rows_through_the_c_abi(G):
    """the wrapper only hands over 16-byte aligned rows; the C ABI takes any alignment (staged byte by byte)"""
    codec, D, T = G
    from gswm_amd import _native as N
    lib = N.lib()
    rng = np.random.default_rng(5)
    for n_bits, mb in ((576, 8), (144, 3), (523296, 4)):        # (the last: rows read in place from global memory lose the word path to the misalignment)
        B, K, k = 5, 9, 4
        pairs = _pairs(rng, K)
        signs = rng.integers(0, 256, (B, n_bits // 8), dtype=np.uint8)
        want = R.topk(R.stats(signs, R.keystreams(pairs, n_bits), mb), k)
        buf = torch.zeros(B * (n_bits // 8) + 16, dtype=torch.uint8, device="cuda")
        buf[1:1 + signs.size] = torch.from_numpy(signs.reshape(-1)).cuda()
        rows = torch.from_numpy(_key_rows(rng, pairs, 64)).cuda()
        ws = torch.empty(lib.gsw_key_search_workspace_bytes(B, K, k) // 8, dtype=torch.int64, device="cuda")
        idx = torch.empty((B, k), dtype=torch.int32, device="cuda")
        stat = torch.empty((B, k), dtype=torch.int32, device="cuda")
        N.check(lib.gsw_key_search_topk(buf.data_ptr() + 1, B, n_bits, rows.data_ptr(), 64, mb, K, k, idx.data_ptr(), stat.data_ptr(), ws.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream))
        assert np.array_equal(idx.cpu().numpy(), want[0]) and np.array_equal(stat.cpu().numpy(), want[1])


def test_wrapper_refuses_bad_operands(G):
    codec, D, T = G
    s = torch.zeros(2, 32, dtype=torch.uint8).cuda()
    r = torch.zeros(10, 48, dtype=torch.uint8).cuda()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.key_search_topk(s, 256, r.cpu(), 32)
    with pytest.raises(ValueError, match="n_bits"):
        codec.key_search_topk(s, 512, r, 32)
    with pytest.raises(ValueError, match="key rows"):
        codec.key_search_topk(s, 256, r[:, :32].contiguous(), 32)
    with pytest.raises(ValueError, match="msg_bytes"):
        codec.key_search_topk(s, 256, r, 0)
    with pytest.raises(ValueError):
        codec.key_search_topk(s, 256, r, 32, k=9)
    with pytest.raises(ValueError):
        codec.key_search_topk(s.int(), 256, r, 32)
    with pytest.raises(IndexError):
        codec.key_search_topk(s, 256, r, 24)                                   # 256 bits are not a multiple of 192


# ------------------------------------------------------------------------------------------------------------ second oracle
@pytest.mark.parametrize("l", [1, 2, 4])
def test_statistic_is_the_keyed_score_of_the_devices_own_vote(G, l):
    """For every (image, key): a keyed record made of the key, the nonce and the message the device votes under them (extract_records) scores
    exactly `stat` in trace_keyed_topk, and the eight records rank as the eight keys do."""
    codec, D, T = G
    rng = np.random.default_rng(40 + l)
    B, K, mb, shape = 3, 8, 16, (4, 16, 16)
    n = int(np.prod(shape))
    nb = n * l
    z = torch.randn(B, *shape, generator=torch.Generator().manual_seed(l)).half().cuda()
    pairs = _pairs(rng, K)
    keys = torch.from_numpy(_key_rows(rng, pairs, 48)).cuda()
    packed, _ = codec.quant_pack(z, l)
    idx, stat = codec.key_search_topk(packed, nb, keys, mb, k=K)
    stride = codec.keyed_record_stride(mb)
    for b in range(B):
        rows = torch.zeros((K, stride), dtype=torch.uint8, device="cuda")
        rows[:, :48] = keys
        bits, _, _ = codec.extract_records(z[b:b + 1].expand(K, *shape).contiguous(), rows, mb, l=l)
        rows[:, 48:48 + mb] = bits
        ridx, rscore = codec.trace_keyed_topk(packed[b:b + 1].clone(), nb, rows, mb, k=K)
        assert torch.equal(ridx[0], idx[b]) and torch.equal(rscore[0], stat[b]), (b, ridx, idx[b], rscore, stat[b])
    ring = D.Keyring()
    for u, (key, nonce) in enumerate(pairs):
        ring.add(f"k{u}", key, nonce)
    res = D.detect_latents(z, ring, 8 * mb, k=3, l=l)
    assert [[c.index for c in r.candidates] for r in res] == idx[:, :3].cpu().tolist()
    assert [[c.stat for c in r.candidates] for r in res] == stat[:, :3].cpu().tolist()
    assert all(r.key_id is None and r.message is None and r.flags == 0 for r in res)      # noise: no key at 1e-6


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def E2E(G):
    codec, D, T = G
    E = R.E2E
    pairs, msgs, noise, blank = R.e2e_setup()
    ring = D.Keyring()
    for u, (key, nonce) in enumerate(pairs):
        ring.add(f"key-{u}", key, nonce)
    n = int(np.prod(E["shape"]))
    stride = codec.keyed_record_stride(E["msg_bytes"])
    rows = np.zeros((len(msgs), stride), dtype=np.uint8)
    for b, (r, m) in enumerate(zip(E["rows"], msgs)):
        rows[b, :48 + len(m)] = np.frombuffer(pairs[r][0] + pairs[r][1] + m, dtype=np.uint8)
    clean = codec.embed_records(torch.from_numpy(rows).cuda(), E["msg_bytes"], E["shape"], seed=E["seed"], dtype=torch.float32)
    return dict(ring=ring, pairs=pairs, msgs=msgs, noise=noise.cuda(), blank=blank, clean=clean, ks=R.keystreams(pairs, n), n=n)


def _detect_both_ways(G, S, z16):
    """-> (the restatement's answer on these very latents, the device's)"""
    codec, D, T = G
    E = R.E2E
    host = R.detect_host(z16.view(z16.shape[0], -1).cpu(), S["ks"], E["msg_bytes"], D.log10_p_blind, T.log10_p_any)
    dev = D.detect_latents(z16, S["ring"], 8 * E["msg_bytes"], k=2, fpr=E["fpr"])
    saturated = (z16.view(z16.shape[0], -1).double() >= O.Y2_THRESHOLD).any(dim=1).cpu().tolist()       # (noise of sigma 4 reaches 8.29 now and then)
    for h, d, sat in zip(host, dev, saturated):
        top = d.candidates[0]
        assert (top.index, top.stat, top.log10_p_any) == h[:3] and top.key_id == f"key-{h[0]}" and len(d.candidates) == 2
        assert d.flags == (1 if sat else 0)                                      # GSW_FLAG_SATURATED, as extract_batch reports it
        assert d.candidates[1].log10_p_any > math.log10(E["fpr"])                # the runner-up is another key
    return host, dev


@pytest.mark.parametrize("sigma", [1.0, 4.0])
def test_detect_latents_names_the_key_under_noise(G, E2E, sigma):
    """six images under rows [0, 3, 50, 50, 117, 199] of a keyring of 200, unregistered messages, z' = fp16(z + sigma n): the right key first and
    named at fpr 1e-6; at sigma 1 the message is the embedded one, at sigma 4 it is the restatement's vote"""
    E = R.E2E
    z16 = (E2E["clean"].view(6, -1) + sigma * E2E["noise"]).half().view(6, *E["shape"])
    limit = math.log10(E["fpr"])
    host, dev = _detect_both_ways(G, E2E, z16)
    print(f"sigma {sigma}: log10 p_any {[round(h[2], 1) for h in host]}")
    assert [h[0] for h in host] == list(E["rows"]) and all(h[2] <= limit for h in host)           # the restatement alone meets the case
    if sigma == 1.0:
        assert [h[3] for h in host] == E2E["msgs"]
    assert [d.key_id for d in dev] == [f"key-{r}" for r in E["rows"]]
    assert [d.message for d in dev] == [h[3] for h in host]
    if sigma == 1.0:
        assert [d.message for d in dev] == E2E["msgs"]


def test_detect_latents_names_no_key_for_unwatermarked_images(G, E2E):
    E = R.E2E
    z16 = E2E["blank"].half().view(2, *E["shape"]).cuda()
    host, dev = _detect_both_ways(G, E2E, z16)
    assert all(h[2] > math.log10(E["fpr"]) for h in host)                                          # the restatement alone meets the case
    assert all(d.key_id is None and d.message is None for d in dev)
    with pytest.raises(IndexError):
        G[1].detect_latents(torch.zeros(1, 4, 10, 10).cuda(), E2E["ring"], 256)                    # 400 lattice bits, 256-bit messages


def test_cli_over_latents(G, E2E, tmp_path, monkeypatch, capsys):
    """The front end on a keyring file.  Synthetic weights are not an autoencoder, so the inversion is replaced by latents (two issued ones and
    an unwatermarked one): the rest -- keyring, search, statistics, detect.txt -- is the real run."""
    from PIL import Image
    from gswm_amd import extract as X
    codec, D, T = G
    E = R.E2E
    ring_file = tmp_path / "ring.tsv"
    E2E["ring"].save(ring_file)
    d = tmp_path / "imgs"
    d.mkdir()
    rng = np.random.RandomState(4)
    for i in range(3):
        Image.fromarray(rng.randint(0, 256, (80, 96, 3), dtype=np.uint8)).save(str(d / f"img{i}.png"))
    (d / "broken.png").write_bytes(b"not an image")
    latents = torch.cat([E2E["clean"][4:5], E2E["clean"][1:2], E2E["blank"][:1].view(1, *E["shape"]).cuda()]).half()
    calls = []

    def fake_inversion(arrs, args, **kw):
        calls.append(len(arrs))
        return latents[:len(arrs)].clone()

    monkeypatch.setattr(X, "invert_decoded_images", fake_inversion)
    D.main(["--images_directory_path", str(d), "--keyring", str(ring_file), "--message_length", "256", "--allow_synthetic_weights",
            "--num_inference_steps", "3", "--width", "128", "--height", "128", "--strict_kernels", "0", "--top", "2", "--fpr", "1e-6"])
    out = capsys.readouterr().out
    assert calls == [3]
    lines = (d / "detect.txt").read_text().splitlines()
    start = lines.index("=" * 40 + "Batch Start" + "=" * 40)
    info = dict(l.split(",", 1) for l in lines[1:start])
    assert info["keys"] == "200" and info["message_length"] == "256" and info["l"] == "1" and info["fpr"] == "1e-06"
    assert lines[start + 1].startswith("SYNTHETIC WEIGHTS,")
    body = lines[start + 2:-1]
    files = X._DirJob(str(d)).files
    assert len(body) == len(files) == 4
    want = iter(D.detect_latents(latents, E2E["ring"], 256, k=2))
    named = iter([(f"key-{E['rows'][4]}", E2E["msgs"][4].hex()), (f"key-{E['rows'][1]}", E2E["msgs"][1].hex()), ("none", "none")])
    for f, line in zip(files, body):
        if f.endswith("broken.png"):
            assert line.startswith(f"Error processing {f}: ")
        else:
            assert line == D.format_line(os.path.basename(f), next(want))
            key_id, msg = next(named)
            assert line.startswith(f"{os.path.basename(f)}, key: {key_id}, log10 p, ") and f", message: {msg}" in line
        assert line in out
    with pytest.raises(SystemExit):
        D.main(["--images_directory_path", str(d), "--keyring", str(ring_file), "--top", "9"])
    assert "--top" in capsys.readouterr().err
