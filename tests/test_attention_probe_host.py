"""CPU (no GPU): the claims tests/attention_reference.py makes about its own operands, checked in fp64 at the shapes of the `cover/` rows of
tests/golden/attn_plan_cases.tsv (the shapes tests/test_gpu_attention_probe.py runs), two heads of one image each:
  * the operands are exact in fp16 and bf16: the scores recomputed from the ROUNDED tensors are the integers -2048 hamming - rho (tiles to the last), below 2^24;
  * one-hot: the target's fp64 softmax weight is >= 1 - 2^-100 and every other key is >= 160 below it in the base-2 exponent (so 0 in fp32), padded keys apart,
    which score +2048 and must be masked;
  * every schedule makes every key of its range a target within the launch cap, and a 32-query block of the "stride" schedule aims at as many different key
    tiles as there are;
  * two-hot: the two keys lie in different tiles (different splits on key-split rows), weigh exactly 1/2 each, and rounding the fp32 sum equals rounding the exact one;
  * the tolerance cases are what they say (maxima that rise / fall by about 3 nats per tile, a subnormal tail, a +2000 offset), and the rounding model of the kernel
    stays within 5 u max|v| of the fp64 softmax for them."""
import math

import pytest
import torch

import attention_reference as R
from test_attn_plan_host import form_of, load_table

COVER = [r for r in load_table() if r["tag"].startswith("cover/")]
DTYPES = [torch.float16, torch.bfloat16]


def shape_of(r):
    return int(r["head_dim"]), int(r["Sq"]), int(r["Sk"]), int(r["Sk_valid"])


def valid_counts(r):
    """the numbers of valid keys the probes run a row with"""
    d, Sq, Sk, Skv = shape_of(r)
    out = {Skv}
    if form_of(r) != "ksplit":
        out |= {v for v in (1, 64, 63, 65, Sk - 1, Sk - 64, Sk - 65, Sk - 63, 77, Sk - 128, Sk - 129) if 1 <= v <= Sk}
    return sorted(out)


@pytest.mark.parametrize("r", COVER, ids=[r["tag"] for r in COVER])
def test_one_hot_operands_are_exact_and_one_hot(r):
    d, Sq, Sk, _ = shape_of(r)
    Sq = min(Sq, 512)
    B, H = 1, 2
    n = R.code_bits(Sk)
    assert n <= 14 and n + 2 <= 40 and n * R.A <= 448
    for dtype in DTYPES:
        for Skv in valid_counts(r):
            k = R.probe_keys(B, H, d, Sk, Skv, dtype)
            for kind in R.SCHEDULES:
                tg, rho = R.schedule(kind, 1, B, H, Sq, Sk, Skv)
                assert tg.shape == (B, H, Sq) and int(tg.min()) >= 0 and int(tg.max()) < Skv
                q = R.probe_queries(tg, rho, d, Sk, dtype)
                raw = R.scores_fp64(q, k, H, 1.0)
                j = torch.arange(Sk).view(1, 1, 1, Sk)
                ham = torch.zeros(B, H, Sq, Sk, dtype=torch.int64)
                for c in range(n):
                    ham += ((j >> c) & 1) != ((tg.unsqueeze(-1) >> c) & 1)
                want = (-R.GAP * ham - rho.to(torch.int64).unsqueeze(-1) * ((Skv - 1) // 64 - j // 64)).to(torch.float64)
                assert torch.equal(raw[..., :Skv], want[..., :Skv]) and float(raw.abs().max()) < 2 ** 24
                assert Skv == Sk or bool((raw[..., Skv:] == R.GAP).all())
                at = raw.gather(-1, tg.unsqueeze(-1))
                assert bool((at == 0).all())
                others = raw[..., :Skv].scatter(-1, tg.unsqueeze(-1), -math.inf)
                gap = (-others.max(dim=-1).values * d ** -0.5 * math.log2(math.e)).min().item() if Skv > 1 else math.inf
                assert gap >= 160, (kind, Skv, gap)
                p = torch.softmax(R.scores_fp64(q, k, H, d ** -0.5, Skv), dim=-1).gather(-1, tg.unsqueeze(-1))
                assert float(p.min()) >= 1 - 2.0 ** -100
                if kind == "last" and Skv > 64:          # the running maximum rises at EVERY tile, by 2048 raw or more
                    best = torch.stack([raw[..., t * 64:min(Skv, t * 64 + 64)].max(dim=-1).values for t in range((Skv + 63) // 64)], dim=-1)
                    assert float((best[..., 1:] - best[..., :-1]).min()) >= R.GAP


@pytest.mark.parametrize("r", COVER, ids=[r["tag"] for r in COVER])
def test_schedules_cover_their_keys_within_the_launch_cap(r):
    d, Sq, Sk, _ = shape_of(r)
    B, H = 2, 3
    for Skv in valid_counts(r):
        cap = R.launch_cap(Sq, Skv)
        lo = 64 * ((Skv - 1) // 64)
        for kind, rng in (("stride", (0, Skv)), ("last", (lo, Skv)), ("first", (0, min(64, Skv)))):
            L = R.launches(kind, Sq, Skv)
            assert 1 <= L <= cap
            seen = torch.zeros(B, H, Sk, dtype=torch.bool)
            for ln in range(L):
                tg, _ = R.schedule(kind, ln, B, H, Sq, Sk, Skv)
                seen.scatter_(-1, tg, True)
            assert bool(seen[..., rng[0]:rng[1]].all()) and not bool(seen[..., :rng[0]].any()) and not bool(seen[..., rng[1]:].any()), (kind, Skv)
        tg, rho = R.schedule("mixed", 0, B, H, Sq, Sk, Skv)
        last = rho > 0
        assert bool((tg[last] >= lo).all()) and bool((tg[~last] < 64).all()) and bool((rho[last] == R.ramp_weight(Sk)).all())
        for q0 in range(0, Sq - 31, 32):          # both kinds in every 16 queries of a wave, and queries i and i + 16 (one lane of the 16-row tail) of different kinds somewhere
            w = last[0, 0, q0:q0 + 32]
            assert 0 < int(w[:16].sum()) < 16 and 0 < int(w[16:].sum()) < 16 and bool((w[:16] != w[16:]).any()) and bool((w[0::2] != w[1::2]).any())
        # a 32-query block of the stride schedule aims at different key tiles: the stride is a tile and a slot (65 or a little more), so between two wraps
        # around Sk_valid every query's target lies one or two tiles past its neighbour's, and a block holds a whole such run or is one
        tg, _ = R.schedule("stride", 0, B, H, Sq, Sk, Skv)
        run = Skv // R.stride_of(Skv)
        for q0 in range(0, Sq, 32):
            blk = tg[..., q0:q0 + 32]
            up = blk[..., 1:] > blk[..., :-1]
            step = blk[..., 1:] // 64 - blk[..., :-1] // 64
            assert Skv < 128 or bool(((step >= 1) & (step <= 2))[up].all()), (Skv, q0)          # (from two whole tiles up: below, the stride is taken modulo a tile)
            for b in range(B):
                for h in range(H):
                    assert len(set((blk[b, h] // 64).tolist())) >= min(blk.shape[-1], run), (Skv, q0)


TWO_HOT = [r for r in COVER if int(r["Sk"]) >= 128]


@pytest.mark.parametrize("r", TWO_HOT, ids=[r["tag"] for r in TWO_HOT])
def test_two_hot_pairs_and_their_expected_rows(r):
    d, Sq, Sk, Skv = shape_of(r)
    Sq = min(Sq, 256)
    B, H = 1, 2
    nt, ks = Sk // 64, int(r["ksplit"])
    for dtype in DTYPES:
        k = R.probe_keys(B, H, d, Sk, Skv, dtype)
        v = R.probe_values(B, H, d, Sk, Skv, dtype, 5)
        for ln in range(3):
            j1, j2 = R.two_hot_pairs(Sk, Skv, ln)
            assert j1.numel() >= 4 and len(set(j1.tolist()) | set(j2.tolist())) == 2 * j1.numel() and int(j2.max()) < Skv
            assert bool((j1 // 64 != j2 // 64).all())
            if ks > 1:          # the split s of the kernel walks tiles [s nt / ks, (s + 1) nt / ks)
                split = lambda t: max(s for s in range(ks) if s * nt // ks <= t)
                assert all(split(a // 64) != split(b // 64) for a, b in zip(j1.tolist(), j2.tolist()))
            k2, tg, exp = R.two_hot(k, v, H, Sq, j1, j2)
            q = R.probe_queries(tg, torch.zeros(B, H, Sq), d, Sk, dtype)
            p = torch.softmax(R.scores_fp64(q, k2, H, d ** -0.5, Skv), dim=-1)
            assert bool((p.gather(-1, tg.unsqueeze(-1)) == 0.5).all()) and bool(((p == 0.5).sum(dim=-1) == 2).all()) and bool(((p <= 2.0 ** -160) | (p == 0.5)).all())
            ref = R.softmax_fp64(q, k2, v, H, d ** -0.5, Skv)
            assert torch.equal(ref.to(dtype), exp)
    # one rounding decides: the fp32 sum of two T values, halved and rounded to T, is the exact sum halved and rounded to T -- on every pair of exponents
    for dtype in DTYPES:
        g = torch.Generator().manual_seed(11)
        a = (torch.randn(1 << 20, generator=g) * torch.exp2(torch.randint(-20, 8, (1 << 20,), generator=g).float())).to(dtype)
        b = (torch.randn(1 << 20, generator=g) * torch.exp2(torch.randint(-20, 8, (1 << 20,), generator=g).float())).to(dtype)
        assert torch.equal(((a.float() + b.float()) * 0.5).to(dtype), ((a.double() + b.double()) * 0.5).to(dtype))


TOL = [(1, 2, 64, 128, 1088), (1, 2, 40, 128, 1088), (1, 2, 64, 128, 2112), (1, 2, 40, 129, 136), (1, 1, 160, 200, 72), (1, 1, 80, 256, 192)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,d,Sq,Sk", TOL)
def test_tolerance_cases_and_the_rounding_model(dtype, B, H, d, Sq, Sk):
    u = R.U[dtype]
    scale = d ** -0.5
    nt = (Sk + 63) // 64
    worst = {}
    for name, (q, k, v) in (("rescale", R.rescale_operands(B, H, d, Sq, Sk, dtype, 3)), ("dominant", R.dominant_operands(B, H, d, Sq, Sk, Sk, dtype, 4)),
                            ("offset", R.offset_operands(B, H, d, Sq, Sk, dtype, 5))):
        s = R.scores_fp64(q, k, H, scale)
        if name == "rescale" and nt >= 3:
            best = torch.stack([s[..., t * 64:min(Sk, t * 64 + 64)].max(dim=-1).values for t in range(nt if Sk % 64 == 0 else nt - 1)], dim=-1)
            step = best[..., 1:] - best[..., :-1]
            assert 1.5 <= float(step[:, :, 0::2].min()) and float(step[:, :, 0::2].max()) <= 4.5          # about 3 nats up per tile for the even queries
            assert -4.5 <= float(step[:, :, 1::2].min()) and float(step[:, :, 1::2].max()) <= -1.5       # ... and down for the odd ones
        if name == "dominant":
            p = torch.softmax(s, dim=-1)
            top = p.max(dim=-1).values
            assert float(top.min()) >= 0.9 and bool(((p < 2.0 ** -14).sum(dim=-1) == Sk - 1).all()) and float(p.min()) > 2.0 ** -24
            assert 11.5 <= float((s.max(dim=-1).values - s.min(dim=-1).values).min()) <= 12.5
        if name == "offset":
            assert float((s / scale).min()) >= 1900 and float((s.max(dim=-1).values - s.min(dim=-1).values).max()) <= 25
        ref = R.softmax_fp64(q, k, v, H, scale)
        vmax = v.double().abs().view(B, Sk, H, d).amax(dim=(1, 3))          # per image and head
        err = ((R.rounded_model(q, k, v, H, scale).double() - ref).abs().view(B, Sq, H, d).amax(dim=(1, 3)) / (u * vmax)).max().item()
        worst[name] = round(err, 3)
        assert err <= 5.0, (name, err)
    print(worst)
