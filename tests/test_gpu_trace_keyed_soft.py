"""GPU: the keyed registry search ranked by reliability-weighted margins -- codec.level_pack against the NumPy
restatement of the levels (tests/soft_reference.py, tests/keyed_soft_reference.py), codec.trace_keyed_soft_topk against
trace.keyed_soft_topk_host on codewords of the oracle's ChaCha20, its identities with the sign search and with the shared-key reliability
search, the same parity on poisoned buffers, what the statistic buys under noise, then trace_latents_keyed_soft and the front end.
EXACT equality of bits, flags, sums, indices and scores everywhere, no tolerance."""
import os

import numpy as np
import pytest
import torch

from conftest import README_KEY, README_NONCE

import gs_oracle as O
import keyed_soft_reference as KR
import soft_reference as SR
from test_gpu_trace_keyed import _issue_log, _records_and_codewords, _rows

pytestmark = pytest.mark.gpu

KEY, NONCE = bytes.fromhex(README_KEY), bytes.fromhex(README_NONCE)
INT32_MIN = -2 ** 31


@pytest.fixture(scope="module")
def G():
    import gswm_amd  # noqa: F401
    from gswm_amd import codec, trace
    return codec, trace


# ------------------------------------------------------------------------------------------------------------ level_pack
def _tables(rng, B, levels):
    """float32 [B, levels], increasing per image; every other entry is representable in bf16 (hence in every input dtype), so that a planted
    element can EQUAL a threshold in every dtype"""
    t = np.sort(rng.uniform(0.05, 2.5, (B, levels)), axis=1).astype(np.float32)
    exact = torch.from_numpy(t).to(torch.bfloat16).to(torch.float32).numpy()
    t[:, ::2] = exact[:, ::2]
    return np.sort(t, axis=1)


def _planted(dtype, table):
    """NaN, +-inf, -0.0, and for every threshold the value of `dtype` nearest to it with its two neighbours by bit pattern"""
    t = torch.from_numpy(table).to(dtype)
    ints = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}[dtype]
    around = torch.cat([t, (t.view(ints) - 1).view(dtype), (t.view(ints) + 1).view(dtype), -t])
    return torch.cat([torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0, 0.0], dtype=dtype), around])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64])
@pytest.mark.parametrize("B,shape", [(5, (4, 64, 64)), (3, (4, 13, 10)), (2, (1, 1, 8))])
def test_level_pack_is_the_restated_quantiser_and_levels(G, dtype, B, shape):
    codec, T = G
    n = int(np.prod(shape))
    for levels in (1, 2, 3, 7, 8, 15):                                        # every P, both sides of each plane boundary
        for per_image in (False, True):
            rng = np.random.default_rng(1000 * n + 10 * levels + per_image)
            g = torch.Generator().manual_seed(n + levels)
            z = (torch.randn(B, n, generator=g, dtype=torch.float64) * 1.2).to(dtype)
            tables = _tables(rng, B, levels)
            table = tables if per_image else tables[0]
            own = tables[1] if per_image else tables[0]
            plant = _planted(dtype, own)[:n]
            z[1, torch.randperm(n, generator=g)[:plant.numel()]] = plant        # image 1: every planted scalar that fits (NaN and +inf: both flags)
            z[0, 0::3] = 0.0
            z[0, 1::3] = -0.0                                                  # image 0: +-0 throughout, no flag
            zd = z.view(B, *shape).cuda()
            rows = codec.level_pack(zd, torch.from_numpy(table).cuda())
            P = levels.bit_length()
            assert rows.signs.dtype == torch.uint8 and rows.signs.shape == (B, n // 8) and rows.planes.dtype == torch.uint8 and rows.planes.shape == (B, P, n // 8)
            assert all(t.dtype == torch.int32 and t.shape == (B,) for t in (rows.wsum, rows.wsq, rows.flags))
            want = KR.level_rows(SR.widen(z), table)
            where = (levels, per_image)
            assert np.array_equal(rows.signs.cpu().numpy(), want["signs"]), where
            assert np.array_equal(rows.planes.cpu().numpy(), want["planes"]), where
            assert rows.wsum.cpu().tolist() == want["wsum"].tolist() and rows.wsq.cpu().tolist() == want["wsq"].tolist(), where
            assert rows.flags.cpu().tolist() == want["flags"].tolist(), where
            signs, flags = codec.sign_pack(zd)
            assert torch.equal(rows.signs, signs) and torch.equal(rows.flags, flags), where
            if n >= plant.numel():
                assert want["flags"][1] == 3 and int(want["levels"][1].max()) == levels and int(want["levels"][0, 0::3].max()) == 0


def test_level_pack_wrapper_refuses_bad_operands(G):
    codec, T = G
    z, thr = torch.zeros(2, 16).cuda(), torch.zeros(3).cuda()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.level_pack(z.cpu(), thr)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.level_pack(z, thr.cpu())
    with pytest.raises(ValueError, match="multiple of 8"):
        codec.level_pack(torch.zeros(2, 12).cuda(), thr)
    with pytest.raises(ValueError, match="unsupported dtype"):
        codec.level_pack(z.int(), thr)
    with pytest.raises(ValueError, match="thresholds"):
        codec.level_pack(z, thr.double())
    with pytest.raises(ValueError, match="thresholds"):
        codec.level_pack(z, torch.zeros(3, 3).cuda())                          # three tables, two images
    with pytest.raises(ValueError, match="levels"):
        codec.level_pack(z, torch.zeros(16).cuda())


# ------------------------------------------------------------------------------------------------------------ the search
def _random_rows(rng, B, n, levels, cw, U):
    """sign rows and levels made on the host (the search alone, not level_pack): image 0 all level 0, the last image all top level, image 1
    (B > 2) the codeword of record U // 2 with one bit flipped at an element of level `levels`"""
    signs = rng.integers(0, 256, (B, n // 8), dtype=np.uint8)
    lv = rng.integers(0, levels + 1, (B, n), dtype=np.int64)
    lv[0] = 0
    if B > 1:
        lv[-1] = levels
    if B > 2:
        j = int(rng.integers(0, n))
        signs[1] = cw[U // 2]
        signs[1, j >> 3] ^= 0x80 >> (j & 7)
        lv[1, j] = levels
    planes = np.stack([np.packbits(((lv >> p) & 1).astype(np.uint8), axis=1) for p in range(levels.bit_length())], axis=1)
    return signs, planes, lv.sum(axis=1).astype(np.int32)


def _device_rows(codec, signs, planes, wsum):
    B = signs.shape[0]
    zero = torch.zeros(B, dtype=torch.int32, device="cuda")
    return codec.LevelRows(torch.from_numpy(signs).cuda(), torch.from_numpy(planes).cuda(), torch.from_numpy(wsum).cuda(), zero, zero)


# U x n x msg_bytes x B x k x levels
CASES = [(1, 8, 1, 1, 1, 1), (2, 256, 32, 3, 4, 3), (63, 520, 5, 64, 8, 15), (64, 16384, 32, 130, 1, 15), (65, 36864, 128, 1, 4, 7), (4097, 256, 8, 64, 1, 2),
         (1000, 65536, 256, 3, 8, 15), (2 ** 17 + 3, 520, 5, 3, 4, 8), (5, 196608, 32, 2, 4, 15), (5, 524288, 32, 2, 4, 1)]
# every plane count (levels 1, 3, 7, 15) x tile (B = 1, 2, 5, 17) of csrc/gswm_search_plan.h at the smallest lattice, the message form alternating (dwords at
# 512 bits of 4-byte messages, byte by byte at 504 bits of 3-byte ones); 9 records: one wave takes a second record; 5 with k = 8: an empty tail
CASES += [(9 if (i + j) % 2 else 5, 512 if (i + j) % 2 else 504, 4 if (i + j) % 2 else 3, B, 3 if (i + j) % 2 else 8, levels)
          for i, levels in enumerate((1, 3, 7, 15)) for j, B in enumerate((1, 2, 5, 17))]


@pytest.mark.parametrize("U,n,msg_bytes,B,k,levels", CASES)
def test_soft_search_matches_the_restatement_on_oracle_codewords(G, U, n, msg_bytes, B, k, levels):
    codec, T = G
    rng = np.random.default_rng(U * 7 + n + msg_bytes + B + levels)
    recs, cw = _records_and_codewords(rng, U, n, msg_bytes)
    signs, planes, wsum = _random_rows(rng, B, n, levels, cw, U)
    rows = _rows(T, recs, msg_bytes).to_device()
    idx, score = codec.trace_keyed_soft_topk(_device_rows(codec, signs, planes, wsum), n, rows, msg_bytes, k=k)
    want_idx, want_score = T.keyed_soft_topk_host(signs, planes, wsum, cw, k)
    got_idx, got_score = idx.cpu().numpy(), score.cpu().numpy()
    assert got_idx.dtype == np.int32 and got_score.dtype == np.int32 and got_idx.shape == (B, k)
    assert np.array_equal(got_score, want_score), (np.argwhere(got_score != want_score)[:5], got_score[:2], want_score[:2])
    assert np.array_equal(got_idx, want_idx), (np.argwhere(got_idx != want_idx)[:5], got_idx[:2], want_idx[:2])
    assert (got_score[0][got_idx[0] >= 0] == 0).all()                          # image 0 carries no weight
    if B > 2:
        assert got_idx[1, 0] == U // 2 and got_score[1, 0] == int(wsum[1]) - 2 * levels


def test_one_step_past_the_domain_raises(G):
    codec, T = G
    rec = torch.zeros(4, 80, dtype=torch.uint8).cuda()
    for P, n in ((1, 524288), (2, 349440), (3, 262144), (4, 209664)):          # the largest multiples of 256 with n (1 + P) <= 2^20
        big = n + 256
        zero = torch.zeros(1, dtype=torch.int32).cuda()
        rows = codec.LevelRows(torch.zeros(1, big // 8, dtype=torch.uint8).cuda(), torch.zeros(1, P, big // 8, dtype=torch.uint8).cuda(), zero, zero, zero)
        with pytest.raises(ValueError, match="domain"):
            codec.trace_keyed_soft_topk(rows, big, rec, 32)


def test_soft_search_wrapper_refuses_bad_operands(G):
    codec, T = G
    zero = torch.zeros(2, dtype=torch.int32).cuda()
    rows = codec.LevelRows(torch.zeros(2, 32, dtype=torch.uint8).cuda(), torch.zeros(2, 2, 32, dtype=torch.uint8).cuda(), zero, zero, zero)
    r = torch.zeros(10, 80, dtype=torch.uint8).cuda()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        codec.trace_keyed_soft_topk(rows._replace(planes=rows.planes.cpu()), 256, r, 32)
    with pytest.raises(ValueError, match="n_bits"):
        codec.trace_keyed_soft_topk(rows, 512, r, 32)
    with pytest.raises(ValueError, match="planes"):
        codec.trace_keyed_soft_topk(rows._replace(planes=rows.planes[:, :, :16].contiguous()), 256, r, 32)
    with pytest.raises(ValueError, match="planes"):
        codec.trace_keyed_soft_topk(rows._replace(planes=torch.zeros(2, 5, 32, dtype=torch.uint8).cuda()), 256, r, 32)
    with pytest.raises(ValueError, match="wsum"):
        codec.trace_keyed_soft_topk(rows._replace(wsum=zero.long()), 256, r, 32)
    with pytest.raises(ValueError, match="record rows"):
        codec.trace_keyed_soft_topk(rows, 256, r[:, :64].contiguous(), 32)
    with pytest.raises(ValueError, match="msg_bytes"):
        codec.trace_keyed_soft_topk(rows, 256, r, 0)
    with pytest.raises(ValueError):
        codec.trace_keyed_soft_topk(rows, 256, r, 32, k=9)
    with pytest.raises(IndexError):
        codec.trace_keyed_soft_topk(rows, 256, r, 24)                          # 256 bits are not a multiple of 192


# ------------------------------------------------------------------------------------------------------------ identities on the device
def _random_records(rng, U, mb):
    rows = np.zeros((U, (48 + mb + 15) // 16 * 16), dtype=np.uint8)
    rows[:, :48 + mb] = rng.integers(0, 256, (U, 48 + mb), dtype=np.uint8)
    return torch.from_numpy(rows).cuda()


def test_one_level_at_threshold_zero_is_the_sign_search(G):
    codec, T = G
    rng = np.random.default_rng(41)
    for n, mb, B, U, k, dtype in ((4096, 16, 20, 3000, 8, torch.float16), (520, 5, 3, 700, 4, torch.float32), (16384, 32, 64, 257, 1, torch.bfloat16)):
        z = torch.randn(B, n, generator=torch.Generator().manual_seed(n)).to(dtype).cuda()
        z[0, ::2] = 0.0
        z[0, 1::4] = -0.0
        rec = _random_records(rng, U, mb)
        rows = codec.level_pack(z, torch.zeros(1).cuda())
        assert rows.wsum.tolist() == [n] * B and rows.wsq.tolist() == [n] * B
        idx, score = codec.trace_keyed_soft_topk(rows, n, rec, mb, k=k)
        want_idx, want_score = codec.trace_keyed_topk(codec.sign_pack(z)[0], n, rec, mb, k=k)
        assert torch.equal(idx, want_idx) and torch.equal(score, want_score)


def test_single_shared_key_equals_the_reliability_search(G):
    """records that share one key: the candidates are those of trace_latents(..., reliability=T), field by field"""
    codec, T = G
    rng = np.random.default_rng(12)
    for shape, M, U, B, k, levels, dtype in (((4, 64, 64), 256, 500, 9, 4, 15, torch.float16), ((4, 16, 16), 64, 300, 5, 8, 3, torch.float32)):
        mb = M // 8
        msgs = rng.integers(0, 256, (U, mb), dtype=np.uint8)
        single, keyed = T.Registry(mb), T.KeyedRegistry(mb)
        for u in range(U):
            single.add(f"u{u}", msgs[u].tobytes())
            keyed.add(f"u{u}", KEY, NONCE, msgs[u].tobytes())
        z = torch.cat([codec.embed_batch(KEY, NONCE, msgs[(37 * b) % U].tobytes(), 1, shape, seed=3, image_index0=b) for b in range(B)])
        # noise of sigma 2, brought back to unit variance as inverted latents are (no element then reaches 8.2924, the reference's ValueError)
        z = ((z + 2.0 * torch.randn(z.shape, generator=torch.Generator().manual_seed(7)).cuda()) / 5.0 ** 0.5).to(dtype).contiguous()
        want = T.trace_latents(z, KEY, NONCE, single, k=k, reliability=levels)
        got = T.trace_latents_keyed_soft(z, keyed, levels=levels, k=k)
        assert len(got) == len(want) == B
        for b in range(B):
            assert got[b].attributed == want[b].attributed
            assert [(c.user_id, c.index, c.score, c.agree, c.log10_p_any) for c in got[b].candidates] == \
                   [(c.user_id, c.index, c.score, c.agree, c.log10_p_any) for c in want[b].candidates], b
        assert [r.candidates[0].index for r in got] == [(37 * b) % U for b in range(B)]


def test_two_halves_merged_on_the_host_equal_one_call(G):
    codec, T = G
    rng = np.random.default_rng(31)
    U, n, mb, B, k, levels = 7001, 2048, 32, 40, 8, 15
    rec = _random_records(rng, U, mb)
    z = torch.randn(B, n, generator=torch.Generator().manual_seed(3)).half().cuda()
    rows = codec.level_pack(z, torch.linspace(0.1, 2.4, levels).cuda())
    whole = [t.cpu().numpy() for t in codec.trace_keyed_soft_topk(rows, n, rec, mb, k=k)]
    h = 3333
    lo = [t.cpu().numpy() for t in codec.trace_keyed_soft_topk(rows, n, rec[:h], mb, k=k)]
    hi = [t.cpu().numpy() for t in codec.trace_keyed_soft_topk(rows, n, rec[h:], mb, k=k)]
    for b in range(B):
        both = sorted([(-int(s), int(i)) for i, s in zip(lo[0][b], lo[1][b])] + [(-int(s), int(i) + h) for i, s in zip(hi[0][b], hi[1][b])])[:k]
        assert [i for _, i in both] == whole[0][b].tolist() and [-s for s, _ in both] == whole[1][b].tolist()


@pytest.mark.parametrize("levels", [1, 15])
def test_batch_size_decides_who_computes_never_what(G, levels):
    """B = 1, 2, 5, 17, 130 of the same images: every tile T in {1, 4, 16, 64} (2048 bits with 4 planes still fit T = 64), the same rows per image"""
    codec, T = G
    rng = np.random.default_rng(51)
    U, n, mb, k = 1500, 2048, 32, 8
    rec = _random_records(rng, U, mb)
    z = torch.randn(130, n, generator=torch.Generator().manual_seed(5)).half().cuda()
    thr = torch.linspace(0.0, 2.4, levels).cuda()
    full = codec.trace_keyed_soft_topk(codec.level_pack(z, thr), n, rec, mb, k=k)
    for B in (1, 2, 5, 17):
        part = codec.trace_keyed_soft_topk(codec.level_pack(z[:B].contiguous(), thr), n, rec, mb, k=k)
        assert torch.equal(part[0], full[0][:B]) and torch.equal(part[1], full[1][:B]), B


def test_wider_record_stride_and_side_stream(G):
    """rows padded beyond the minimum stride; the same call twice and on a side stream"""
    codec, T = G
    rng = np.random.default_rng(8)
    U, n, mb, B, levels = 3000, 4096, 16, 20, 7
    recs, cw = _records_and_codewords(rng, U, n, mb)
    rows = _rows(T, recs, mb).packed()
    wide = np.full((U, 128), 0xA5, dtype=np.uint8)
    wide[:, :48 + mb] = rows[:, :48 + mb]
    signs, planes, wsum = _random_rows(rng, B, n, levels, cw, U)
    s, r, w = _device_rows(codec, signs, planes, wsum), torch.from_numpy(rows).cuda(), torch.from_numpy(wide).cuda()
    a = codec.trace_keyed_soft_topk(s, n, r, mb, k=8)
    b = codec.trace_keyed_soft_topk(s, n, w, mb, k=8)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = codec.trace_keyed_soft_topk(s, n, r, mb, k=8)
    side.synchronize()
    want = T.keyed_soft_topk_host(signs, planes, wsum, cw, 8)
    for x in (a, b, c):
        assert np.array_equal(x[0].cpu().numpy(), want[0]) and np.array_equal(x[1].cpu().numpy(), want[1])


# ------------------------------------------------------------------------------------------------------------ poisoned buffers
def test_poisoned_guard_banded_buffers(G):
    """level_pack and the search with every output in a poisoned, guard-banded buffer and every operand wrapped (tests/poison.py): bands intact,
    every multi-byte output element written, the same bits under both patterns and in the clean run; then the restatement.  A ragged last
    block, rows that are not whole dwords, a message that is not whole dwords, and the shipped lattice with one table per image."""
    import types
    from gswm_amd import _native, pf
    from test_gpu_poisoned import Out, three_ways
    codec, T = G
    GG = types.SimpleNamespace(pf=pf, codec=codec, N=_native)
    for U, n, mb, B, k, levels, dtype in ((63, 520, 5, 64, 8, 15, torch.float16), (300, 16384, 32, 5, 4, 3, torch.float32)):
        rng = np.random.default_rng(U + n)
        recs, cw = _records_and_codewords(rng, U, n, mb)
        z = (torch.randn(B, n, generator=torch.Generator().manual_seed(n), dtype=torch.float64) * 1.2).to(dtype)
        table = _tables(rng, B, levels)
        inp = dict(z=z.cuda(), thr=torch.from_numpy(table).cuda(), rec=_rows(T, recs, mb).to_device())

        def case(i, L):
            rows = codec.level_pack(i["z"], i["thr"])
            idx, score = codec.trace_keyed_soft_topk(rows, n, i["rec"], mb, k=k)
            return Out(written=dict(signs=rows.signs, planes=rows.planes, wsum=rows.wsum, wsq=rows.wsq, flags=rows.flags, idx=idx, score=score))

        c = three_ways(GG, case, inp)
        want = KR.level_rows(SR.widen(z), table)
        for name in ("signs", "planes", "wsum", "wsq", "flags"):
            assert np.array_equal(c.written[name].cpu().numpy().astype(np.int64), want[name].astype(np.int64)), name
        want_idx, want_score = T.keyed_soft_topk_host(want["signs"], want["planes"], want["wsum"], cw, k)
        assert np.array_equal(c.written["score"].cpu().numpy(), want_score) and np.array_equal(c.written["idx"].cpu().numpy(), want_idx)


# ------------------------------------------------------------------------------------------------------------ what it buys
def test_what_it_buys(G):
    """40 images issued under 40 distinct keys inside a registry of 1000 records, fp16, noise of sigma 12 on the latent (a fixed seed, added on
    the device), fpr 1e-6: every integer the device returns equals the restatement on the same noisy latents, and the 15-level statistic
    attributes strictly more images to their true record than the sign statistic, neither a wrong one.  The seed was checked on the CPU first
    (test_trace_keyed_soft_host.py::test_the_chosen_seed_separates_the_two_statistics_on_the_cpu).  Measured on the MI355X with seed 2024: the
    sign statistic attributes 31 of the 40 images, the 15-level statistic 39, neither a wrong one (the NumPy simulation gave 31 against 39 as well)."""
    from gswm_amd import soft as S
    codec, T = G
    recs, owners, cw, noise = KR.buys_setup()
    Y = KR.BUYS
    B, U, mb, n = Y["B"], Y["U"], Y["msg_bytes"], cw.shape[1] * 8
    reg = _rows(T, recs, mb)
    z = codec.embed_records(reg.to_device()[torch.from_numpy(owners).cuda()].contiguous(), mb, Y["shape"], seed=Y["seed"], dtype=torch.float16)
    # brought back to unit variance, as inverted latents are: signs and RMS-scaled levels do not depend on the scale, and no element then reaches 8.2924,
    # for which both functions report the reference's ValueError instead of a result
    zn = ((z.float() + Y["sigma"] * noise.view(z.shape).cuda()) / (1.0 + Y["sigma"] ** 2) ** 0.5).half().contiguous()
    sign = T.trace_latents_keyed(zn, reg, fpr=Y["fpr"])
    soft = T.trace_latents_keyed_soft(zn, reg, levels=Y["levels"], clip=Y["clip"], fpr=Y["fpr"])
    # the restatement on the same noisy latents
    thr = S.uniform_thresholds(zn, Y["levels"], Y["clip"])
    want = KR.level_rows(SR.widen(zn), thr.cpu().numpy())
    rows = codec.level_pack(zn, thr)
    for name in ("signs", "planes", "wsum", "wsq", "flags"):
        assert np.array_equal(getattr(rows, name).cpu().numpy().astype(np.int64), want[name].astype(np.int64)), name
    wi, ws = T.keyed_soft_topk_host(want["signs"], want["planes"], want["wsum"], cw, 1)
    si, ss = T.keyed_topk_host(want["signs"], cw, 1)
    assert [(r.candidates[0].index, r.candidates[0].score) for r in soft] == list(zip(wi[:, 0].tolist(), ws[:, 0].tolist()))
    assert [(r.candidates[0].index, r.candidates[0].score) for r in sign] == list(zip(si[:, 0].tolist(), ss[:, 0].tolist()))
    assert [r.candidates[0].log10_p_any for r in soft] == [T.log10_p_any(S.log10_p(int(ws[b, 0]), int(want["wsq"][b])), U) for b in range(B)]
    ids = [f"u{u}" for u in owners]
    right = {name: sum(1 for r, u in zip(res, ids) if r.attributed == u) for name, res in (("sign", sign), ("soft", soft))}
    wrong = {name: sum(1 for r, u in zip(res, ids) if r.attributed not in (None, u)) for name, res in (("sign", sign), ("soft", soft))}
    print("attributed to the true record:", right, " to a wrong one:", wrong)
    assert right["soft"] > right["sign"] and wrong == {"sign": 0, "soft": 0}


# ------------------------------------------------------------------------------------------------------------ end to end
def test_trace_latents_keyed_soft_on_an_issue_log(G, tmp_path):
    from gswm_amd import issue
    codec, T = G
    log = tmp_path / "info_data.txt"
    users = ["alice", "bob", "carol", "dave", "erin"]
    z, _ = issue.issue_latents([issue.Request(u, f"{u}@example") for u in users], log_path=str(log), seed=9, dtype=torch.float16)
    reg = T.KeyedRegistry.from_info_data(log)
    assert reg.user_ids == [f"info:{i}" for i in range(1, 6)] and reg.n_keys == 5
    M, limit = 256, np.log10(1e-6)
    res = T.trace_latents_keyed_soft(z, reg, k=3)
    rows = codec.level_pack(z, __import__("gswm_amd").soft.uniform_thresholds(z, 15, 2.5))
    for b, r in enumerate(res):
        top = r.candidates[0]
        assert r.attributed == f"info:{b + 1}" == top.user_id and top.index == b and top.agree == M
        assert top.score == int(rows.wsum[b]) and top.log10_p_any <= limit     # a noiseless image agrees everywhere: the score is the whole weight
        assert len(r.candidates) == 3 and all(c.log10_p_any > limit for c in r.candidates[1:])
    noisy = ((z.float() + 4.0 * torch.randn(z.shape, generator=torch.Generator().manual_seed(9)).cuda()) / 17.0 ** 0.5).half()
    assert [r.attributed for r in T.trace_latents_keyed_soft(noisy, reg, tamper_tile=8)] == [f"info:{i}" for i in range(1, 6)]
    noise = torch.randn(8, 4, 64, 64, generator=torch.Generator().manual_seed(5)).cuda()
    out = T.trace_latents_keyed_soft(noise, reg, tamper_tile=8)
    assert all(r.attributed is None and r.tamper is None for r in out)
    assert all(T.format_line(f"{b}.png", r, M).startswith(f"{b}.png, user: none, agreement, ") for b, r in enumerate(out))
    bad = z.float().clone()
    bad[1, 0, 0, 0] = 9.0
    bad[2, 1, 2, 3] = float("nan")
    out = T.trace_latents_keyed_soft(bad, reg)
    assert out[0].attributed == "info:1" and out[3].attributed == "info:4"
    assert isinstance(out[1], ValueError) and "invalid literal for int() with base 2" in str(out[1])
    assert isinstance(out[2], ValueError) and "NaN" in str(out[2])
    with pytest.raises(IndexError):
        T.trace_latents_keyed_soft(torch.zeros(1, 4, 10, 10).cuda(), reg)      # 400 lattice bits, 256-bit messages
    with pytest.raises(ValueError, match="domain"):
        T.trace_latents_keyed_soft(torch.zeros(1, 4, 256, 256).cuda(), reg)    # 262144 bits with 4 planes


def test_cli_keyed_reliability(G, tmp_path, monkeypatch, capsys):
    """The front end with --keyed_reliability 15 on a gs_insert log, through the replaced inversion of test_cli_per_record_keys: two issued
    latents and seeded noise; registry, level_pack, search, statistics, trace.txt and the tamper maps are the real run."""
    from PIL import Image
    from gswm_amd import extract as X
    codec, T = G
    log, z = _issue_log(tmp_path, ["first user", "second user", "third user"])
    d = tmp_path / "imgs"
    d.mkdir()
    rng = np.random.RandomState(4)
    for i in range(3):
        Image.fromarray(rng.randint(0, 256, (80, 96, 3), dtype=np.uint8)).save(str(d / f"img{i}.png"))
    latents = torch.cat([z[2:3].float(), z[0:1].float(), torch.randn(1, 4, 64, 64, generator=torch.Generator().manual_seed(5)).cuda()])
    calls = []

    def fake_inversion(arrs, args, **kw):
        calls.append(len(arrs))
        return latents[:len(arrs)].clone()

    monkeypatch.setattr(X, "invert_decoded_images", fake_inversion)
    maps = tmp_path / "maps"
    T.main(["--images_directory_path", str(d), "--per_record_keys", "--keyed_reliability", "15", "--registry", str(log), "--allow_synthetic_weights",
            "--num_inference_steps", "3", "--width", "128", "--height", "128", "--strict_kernels", "0", "--top", "2", "--fpr", "1e-6",
            "--tamper_map", str(maps), "--tile", "8"])
    out = capsys.readouterr().out
    assert calls == [3]
    lines = (d / "trace.txt").read_text().splitlines()
    start = lines.index("=" * 40 + "Batch Start" + "=" * 40)
    info = dict(l.split(",", 1) for l in lines[1:start])
    assert info["statistic"] == "soft, 15 reliability levels" and info["keys"] == "3" and info["users"] == "3" and info["key_hex"] == "per record"
    body = lines[start + 2:-1]
    files = X._DirJob(str(d)).files
    assert len(body) == len(files) == 3
    reg = T.KeyedRegistry.from_info_data(log)
    want = T.trace_latents_keyed_soft(latents, reg, levels=15, k=2, tamper_tile=8)
    for f, line, w, user in zip(files, body, want, ["info:3", "info:1", "none"]):
        assert line == T.format_line(os.path.basename(f), w, 256) and line in out
        assert line.startswith(f"{os.path.basename(f)}, user: {user}, agreement, ")
    assert "intact tiles" in body[0] and "intact tiles" not in body[2]
    stems = [os.path.splitext(os.path.basename(f))[0] for f in files[:2]]       # the two attributed images, in the order the run took them
    assert sorted(os.listdir(maps)) == sorted(f"{s}.tamper.{ext}" for s in stems for ext in ("npy", "png"))
    for extra, name in ((["--hard"], "--hard"), (["--l", "2"], "--l 2"), (["--reliability", "3"], "--reliability")):
        with pytest.raises(SystemExit):
            T.main(["--images_directory_path", str(d), "--per_record_keys", "--keyed_reliability", "15", "--registry", str(log)] + extra)
        assert name in capsys.readouterr().err
