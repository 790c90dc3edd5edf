"""GPU: blind detection ranked by reliability levels -- the level-weighted key search kernel (codec.key_search_soft_topk) bit for
bit against the NumPy restatement of tests/key_search_soft_reference.py on poisoned, guard-banded buffers (tests/poison.py), its identities with the sign
search, with the soft vote and with the level-weighted registry search, unaligned rows through the C ABI, the wrapper's refusals, then
detect_latents(reliability=15) end to end under noise and the front end.  EXACT equality of indices, statistics and messages everywhere; the bounds, two
minimisations of one convex function, to 1e-9 decades."""
import math
import os

import numpy as np
import pytest
import torch

import gs_oracle as O
import key_search_reference as R0
import key_search_soft_reference as R
from poison import FINITE, NAN, Ledger, poisoned
from test_gpu_key_search import _key_rows, _pairs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gswm_amd  # noqa: F401
    from gswm_amd import codec, detect, trace
    return codec, detect, trace


def _level_rows(codec, signs, planes):
    """the search's operand from host rows (wsum, wsq and flags are not read by it)"""
    zero = torch.zeros(signs.shape[0], dtype=torch.int32, device=signs.device)
    return codec.LevelRows(signs, planes, zero, zero, zero)


def _poisoned_search(codec, signs, planes, n_bits, rows, mb, k, want):
    """the search under both patterns, operands wrapped: no band written, every output element written, the restatement's result"""
    s_dev, p_dev, r_dev = torch.from_numpy(signs).cuda(), torch.from_numpy(planes).cuda(), torch.from_numpy(rows).cuda()
    for name, pattern in (("NAN", NAN), ("FINITE", FINITE)):
        L = Ledger(pattern)
        try:
            with poisoned(L):
                idx, stat = codec.key_search_soft_topk(_level_rows(codec, L.wrap(s_dev), L.wrap(p_dev)), n_bits, L.wrap(r_dev), mb, k=k)
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


# n_bits x msg_bytes x P x B x keys x k x key_stride, a sparse product: every value of each axis appears.  144 bits: one partial ChaCha block, the bit-by-bit
# path (3- and 9-byte messages); k past the keys twice.  Counter classes of csrc/gswm_keysearch_soft_plan.h: 4 (256 bits of 32-byte messages: one copy, all four
# planes through full adders alone), 8, 12, 16 (512 copies of 15 levels), 18 (4370 copies of 15 levels).
CASES = [(144, 3, 1, 1, 1, 1, 48), (144, 9, 2, 3, 5, 8, 64), (144, 3, 4, 17, 64, 3, 80), (256, 4, 1, 70, 257, 1, 48), (256, 8, 3, 1, 5, 8, 64),
         (256, 32, 4, 3, 64, 3, 48), (576, 8, 2, 17, 64, 1, 80), (576, 9, 3, 70, 5, 3, 48), (576, 4, 4, 3, 257, 8, 64), (576, 3, 1, 5, 64, 2, 48),
         (1024, 4, 2, 70, 64, 8, 48), (1024, 32, 3, 17, 5, 1, 64), (1024, 8, 1, 3, 257, 3, 80), (16384, 32, 4, 17, 257, 3, 48), (16384, 32, 1, 70, 5, 8, 80),
         (16384, 256, 2, 3, 64, 8, 64), (16384, 4, 3, 1, 64, 1, 48), (16384, 4, 4, 1, 64, 1, 48), (139840, 4, 4, 2, 3, 2, 48),
         # the LDS bound, 2 images x 3 keys: the last lattice whose three rows (P = 1) share the LDS with a keystream and W_t, and the first that is read from
         # global memory; then the bit-by-bit path, four planes and the largest lattice of the domain from global memory
         (348672, 4, 1, 2, 3, 2, 48), (349184, 4, 1, 2, 3, 2, 48), (349680, 3, 1, 2, 3, 2, 48), (176128, 32, 4, 2, 3, 3, 64), (524288, 32, 1, 2, 3, 2, 48)]


@pytest.mark.parametrize("n_bits,mb,P,B,K,k,stride", CASES)
def test_soft_key_search_matches_the_restatement(G, n_bits, mb, P, B, K, k, stride):
    codec, D, T = G
    rng = np.random.default_rng(n_bits + 7 * mb + 31 * B + K + 1000 * P)
    pairs = _pairs(rng, K)
    signs = rng.integers(0, 256, (B, n_bits // 8), dtype=np.uint8)
    lv = rng.integers(0, 1 << P, (B, n_bits), dtype=np.int64)
    ks = R.keystreams(pairs, n_bits)
    signs[0] = ks[K // 2]                                                      # decrypts to all zeros under that key: every position unanimous
    if B > 2:
        lv[1] = 0                                                              # no weight anywhere: S = 0 under every key, row 0 wins
        lv[-1] = (1 << P) - 1                                                  # planes of all ones
    planes = R.planes_of_levels(lv, P)
    want = R.topk(R.stats(signs, lv, ks, mb), k)
    assert want[1][0, 0] == lv[0].sum()                                        # |X_t| = W_t at every position
    if B > 2:
        assert want[1][1, 0] == 0 and want[0][1, 0] == 0
    _poisoned_search(codec, signs, planes, n_bits, _key_rows(rng, pairs, stride), mb, k, want)


@pytest.mark.parametrize("n_bits,mb", [(576, 9), (1024, 8), (16384, 32), (524288, 4)])
def test_one_plane_of_all_ones_is_the_sign_search(G, n_bits, mb):
    codec, D, T = G
    rng = np.random.default_rng(n_bits + mb)
    B, K, k = (2, 3, 3) if n_bits > 100000 else (5, 70, 8)
    signs = torch.from_numpy(rng.integers(0, 256, (B, n_bits // 8), dtype=np.uint8)).cuda()
    keys = torch.from_numpy(_key_rows(rng, _pairs(rng, K), 48)).cuda()
    ones = torch.full((B, 1, n_bits // 8), 0xFF, dtype=torch.uint8, device="cuda")
    idx, stat = codec.key_search_soft_topk(_level_rows(codec, signs, ones), n_bits, keys, mb, k=k)
    sidx, sstat = codec.key_search_topk(signs, n_bits, keys, mb, k=k)
    assert torch.equal(idx, sidx) and torch.equal(stat, sstat)


@pytest.mark.parametrize("levels,mb", [(15, 16), (3, 16), (7, 9), (1, 4)])
def test_statistic_is_the_soft_votes_and_the_level_weighted_registry_score(G, levels, mb):
    """On level_pack of random fp16 latents, for every (image, key): stat = sum_t |score[t]| of extract_soft under that key with the same thresholds, and a
    record made of the key and the soft-voted message scores exactly `stat` in trace_keyed_soft_topk; the records rank as the keys do."""
    codec, D, T = G
    from gswm_amd import soft
    rng = np.random.default_rng(50 + levels)
    B, K, shape = 3, 8, (4, 16, 18)
    n = int(np.prod(shape))
    z = (torch.randn(B, *shape, generator=torch.Generator().manual_seed(levels)) * 1.3).half().cuda()
    thr = soft.uniform_thresholds(z, levels)
    rows = codec.level_pack(z, thr)
    keys = torch.from_numpy(_key_rows(rng, _pairs(rng, K), 48)).cuda()
    idx, stat = codec.key_search_soft_topk(rows, n, keys, mb, k=K)
    stride = codec.keyed_record_stride(mb)
    for b in range(B):
        recs = torch.zeros((K, stride), dtype=torch.uint8, device="cuda")
        recs[:, :48] = keys
        vote = codec.extract_soft(z[b:b + 1].expand(K, *shape).contiguous(), recs, mb, thr[b:b + 1].expand(K, -1).contiguous())
        S = vote.score.abs().sum(dim=1)
        assert torch.equal(S[idx[b].long()].int(), stat[b]), (b, S, idx[b], stat[b])
        recs[:, 48:48 + mb] = vote.bits
        one = codec.LevelRows(*(t[b:b + 1].clone() for t in rows))
        ridx, rscore = codec.trace_keyed_soft_topk(one, n, recs, mb, k=K)
        assert torch.equal(ridx[0], idx[b]) and torch.equal(rscore[0], stat[b]), (b, ridx, idx[b], rscore, stat[b])


def test_unaligned_rows_through_the_c_abi(G):
    """the wrapper only hands over 16-byte aligned rows; the C ABI takes any alignment (staged byte by byte; read in place, rows lose the word path)"""
    codec, D, T = G
    from gswm_amd import _native as N
    lib = N.lib()
    rng = np.random.default_rng(6)
    for n_bits, mb, P in ((576, 8, 2), (144, 3, 3), (349184, 4, 1)):
        B, K, k = (2, 3, 2) if n_bits > 100000 else (5, 9, 4)
        pairs = _pairs(rng, K)
        rb = n_bits // 8
        signs = rng.integers(0, 256, (B, rb), dtype=np.uint8)
        lv = rng.integers(0, 1 << P, (B, n_bits), dtype=np.int64)
        planes = R.planes_of_levels(lv, P)
        want = R.topk(R.stats(signs, lv, R.keystreams(pairs, n_bits), mb), k)
        sbuf = torch.zeros(B * rb + 16, dtype=torch.uint8, device="cuda")
        sbuf[1:1 + signs.size] = torch.from_numpy(signs.reshape(-1)).cuda()
        pbuf = torch.zeros(B * P * rb + 16, dtype=torch.uint8, device="cuda")
        pbuf[3:3 + planes.size] = torch.from_numpy(planes.reshape(-1)).cuda()
        rows = torch.from_numpy(_key_rows(rng, pairs, 64)).cuda()
        ws = torch.empty(lib.gsw_key_search_soft_workspace_bytes(B, K, k) // 8, dtype=torch.int64, device="cuda")
        idx = torch.empty((B, k), dtype=torch.int32, device="cuda")
        stat = torch.empty((B, k), dtype=torch.int32, device="cuda")
        N.check(lib.gsw_key_search_soft_topk(sbuf.data_ptr() + 1, pbuf.data_ptr() + 3, P, B, n_bits, rows.data_ptr(), 64, mb, K, k, idx.data_ptr(), stat.data_ptr(),
                                             ws.data_ptr(), torch.cuda.current_stream().cuda_stream))
        assert np.array_equal(idx.cpu().numpy(), want[0]) and np.array_equal(stat.cpu().numpy(), want[1]), (n_bits, mb, P)


def test_wrapper_refuses_bad_operands(G):
    codec, D, T = G
    s = torch.zeros(2, 32, dtype=torch.uint8).cuda()
    p = torch.zeros(2, 2, 32, dtype=torch.uint8).cuda()
    r = torch.zeros(10, 48, dtype=torch.uint8).cuda()
    rows = _level_rows(codec, s, p)
    assert codec.key_search_soft_topk(rows, 256, r, 32)[1].cpu().tolist() == [[0], [0]]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.key_search_soft_topk(rows, 256, r.cpu(), 32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.key_search_soft_topk(_level_rows(codec, s, p.cpu()), 256, r, 32)
    with pytest.raises(ValueError, match="n_bits"):
        codec.key_search_soft_topk(rows, 512, r, 32)
    with pytest.raises(ValueError, match="key rows"):
        codec.key_search_soft_topk(rows, 256, r[:, :32].contiguous(), 32)
    with pytest.raises(ValueError, match="msg_bytes"):
        codec.key_search_soft_topk(rows, 256, r, 0)
    with pytest.raises(ValueError):
        codec.key_search_soft_topk(rows, 256, r, 32, k=9)
    with pytest.raises(ValueError, match="rows.signs"):
        codec.key_search_soft_topk(_level_rows(codec, s.int(), p), 256, r, 32)
    for bad in (p[:1], p[:, :, :16].contiguous(), torch.zeros(2, 5, 32, dtype=torch.uint8).cuda(), p.int(), p[:, 0]):
        with pytest.raises(ValueError, match="rows.planes"):
            codec.key_search_soft_topk(_level_rows(codec, s, bad), 256, r, 32)
    with pytest.raises(IndexError):
        codec.key_search_soft_topk(rows, 256, r, 24)                           # 256 bits are not a multiple of 192
    big = torch.zeros(1, 43776, dtype=torch.uint8).cuda()                      # 350 208 bits x (1 + 2) planes: past the domain
    with pytest.raises(ValueError, match="domain"):
        codec.key_search_soft_topk(_level_rows(codec, big, torch.zeros(1, 2, 43776, dtype=torch.uint8).cuda()), 350208, r, 32)


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def E2E(G):
    codec, D, T = G
    E = R.E2E
    pairs, msgs, u, noise, blank = R.e2e_setup()
    ring = D.Keyring()
    for i, (key, nonce) in enumerate(pairs):
        ring.add(f"key-{i}", key, nonce)
    n = u.shape[1]
    stride = codec.keyed_record_stride(E["msg_bytes"])
    rows = np.zeros((len(msgs), stride), dtype=np.uint8)
    for b, (r, m) in enumerate(zip(E["rows"], msgs)):
        rows[b, :48 + len(m)] = np.frombuffer(pairs[r][0] + pairs[r][1] + m, dtype=np.uint8)
    clean = codec.embed_records(torch.from_numpy(rows).cuda(), E["msg_bytes"], E["shape"], u=torch.from_numpy(u).cuda(), dtype=torch.float32)
    z16 = (clean.view(len(msgs), -1) + E["sigma"] * noise.cuda()).half().view(len(msgs), *E["shape"])
    return dict(ring=ring, pairs=pairs, msgs=msgs, z16=z16, blank=blank.half().view(-1, *E["shape"]).cuda(), ks=R.keystreams(pairs, n))


def _detect_both_ways(G, S, z16):
    """-> (the restatement's answer on these very latents and the device's threshold tables, the device's)"""
    codec, D, T = G
    from gswm_amd import soft
    E = R.E2E
    flat = z16.view(z16.shape[0], -1)
    thr = soft.uniform_thresholds(z16, E["levels"]).cpu().numpy()
    host = R.detect_soft_host(flat.cpu(), thr, S["ks"], E["msg_bytes"], T.log10_p_any)
    dev = D.detect_latents(z16, S["ring"], 8 * E["msg_bytes"], k=2, fpr=E["fpr"], reliability=E["levels"])
    saturated = (flat.double() >= O.Y2_THRESHOLD).any(dim=1).cpu().tolist()
    for h, d, sat in zip(host, dev, saturated):
        top = d.candidates[0]
        assert (top.index, top.stat) == h[:2] and top.key_id == f"key-{h[0]}" and len(d.candidates) == 2
        assert top.log10_p_any == pytest.approx(h[2], abs=1e-9)
        assert d.flags == (1 if sat else 0)
        assert d.candidates[1].log10_p_any > math.log10(E["fpr"])                # the runner-up is another key
    return host, dev


def test_fifteen_levels_name_six_keys_where_the_signs_name_three(G, E2E):
    """six 4 x 32 x 32 latents under six keys of a keyring of 12, 64-bit messages, z' = fp16(z + 5 n), fpr 1e-4.  The counts are decided by the restatement on
    the CPU (tests/test_detect_soft_host.py holds the same case on the oracle's latents); the device must only equal it."""
    codec, D, T = G
    E = R.E2E
    limit = math.log10(E["fpr"])
    host, dev = _detect_both_ways(G, E2E, E2E["z16"])
    sign_host = R0.detect_host(E2E["z16"].view(6, -1).cpu(), E2E["ks"], E["msg_bytes"], D.log10_p_blind, T.log10_p_any)
    print(f"15 levels: log10 p_any {[round(float(h[2]), 2) for h in host]}\nsigns:     log10 p_any {[round(float(h[2]), 2) for h in sign_host]}")
    assert [h[0] for h in host] == list(E["rows"]) and all(h[2] <= limit for h in host)           # the restatement alone: all six
    assert sum(1 for h in sign_host if h[2] <= limit) <= 3                                         # the restatement alone: at most three
    assert [d.key_id for d in dev] == [f"key-{r}" for r in E["rows"]]
    assert [d.message for d in dev] == [h[3] for h in host]
    sign_dev = D.detect_latents(E2E["z16"], E2E["ring"], 8 * E["msg_bytes"], fpr=E["fpr"], reliability=0)
    assert [d.key_id for d in sign_dev] == [f"key-{h[0]}" if h[2] <= limit else None for h in sign_host]
    assert [(d.candidates[0].index, d.candidates[0].stat) for d in sign_dev] == [h[:2] for h in sign_host]
    assert sum(1 for d in sign_dev if d.key_id is not None) <= 3


def test_unwatermarked_latents_name_no_key(G, E2E):
    E = R.E2E
    host, dev = _detect_both_ways(G, E2E, E2E["blank"])
    assert len(dev) == 4 and all(h[2] > math.log10(E["fpr"]) for h in host)                        # the restatement alone meets the case
    assert all(d.key_id is None and d.message is None for d in dev)
    with pytest.raises(IndexError):
        G[1].detect_latents(torch.zeros(1, 4, 10, 10).cuda(), E2E["ring"], 256, reliability=15)   # 400 lattice bits, 256-bit messages


def test_cli_over_latents(G, E2E, tmp_path, monkeypatch, capsys):
    """The front end with --reliability 15 on a keyring file; the inversion is replaced by latents (two issued ones and an unwatermarked one), the rest --
    keyring, thresholds, level rows, search, bounds, detect.txt -- is the real run."""
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
    latents = torch.cat([E2E["z16"][4:5], E2E["z16"][1:2], E2E["blank"][:1]])
    calls = []

    def fake_inversion(arrs, args, **kw):
        calls.append(len(arrs))
        return latents[:len(arrs)].clone()

    monkeypatch.setattr(X, "invert_decoded_images", fake_inversion)
    D.main(["--images_directory_path", str(d), "--keyring", str(ring_file), "--message_length", "64", "--allow_synthetic_weights", "--num_inference_steps", "3",
            "--width", "128", "--height", "128", "--strict_kernels", "0", "--top", "2", "--fpr", "1e-4", "--reliability", "15"])
    out = capsys.readouterr().out
    assert calls == [3]
    lines = (d / "detect.txt").read_text().splitlines()
    start = lines.index("=" * 40 + "Batch Start" + "=" * 40)
    info = dict(l.split(",", 1) for l in lines[1:start])
    assert info["keys"] == "12" and info["message_length"] == "64" and info["reliability"] == "15" and info["fpr"] == "0.0001"
    body = lines[start + 2:-1]
    files = X._DirJob(str(d)).files
    assert len(body) == len(files) == 3
    want = D.detect_latents(latents, E2E["ring"], 64, k=2, fpr=1e-4, reliability=15)
    named = [f"key-{E['rows'][4]}", f"key-{E['rows'][1]}", "none"]
    for f, line, w, key_id in zip(files, body, want, named):
        assert line == D.format_line(os.path.basename(f), w) and line in out
        assert line.startswith(f"{os.path.basename(f)}, key: {key_id}, log10 p, ")
        assert f", message: {w.message.hex() if w.message is not None else 'none'}" in line
