"""GPU: the soft-decision vote -- `codec.extract_soft` (gsw_extract_soft), `soft.uniform_thresholds` / `soft.extract_soft`, `trace.trace_latents(reliability=)`.

All six outputs are exact integers: they are compared bit for bit with the NumPy restatement (tests/soft_reference.py), which shares no code with the device
path; the keystream of the restatement is the oracle's ChaCha20."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import gs_oracle as O  # noqa: E402
import soft_reference as R  # noqa: E402
from poison import FINITE, NAN, Ledger, poisoned  # noqa: E402
from record_rows import counter_carry_rows, make_records  # noqa: E402

pytestmark = pytest.mark.gpu

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
DTYPES = [F32, F16, BF16, F64]
DTYPE_IDS = ["f32", "f16", "bf16", "f64"]
SAT = 8.3125            # >= 8.2924 (the quantiser saturates from 8.292361075813597) and representable in fp16 and bf16
OUTPUTS = ("bits", "flags", "matches", "score", "wsum", "wsq")

# (elements per image, msg_bytes, B): 256 elements with an 8-bit message; 4 x 24 x 40 with a 15-byte message (M = 120, 32 copies: neither a power of two
# nor word-sized, 255 of the 256 threads walk the image); 4 x 64 x 64 with 256 bits; one image at the cap of 1 048 576 elements with M = 2048;
# 2048 elements (four ChaCha blocks) under records whose block counter carries inside the row (CARRY)
CARRY = (2048, 2, 3)
GEOMETRIES = [(256, 1, 3), (256, 1, 70), (3840, 15, 1), (3840, 15, 70), (16384, 32, 3), (16384, 32, 70), (1048576, 256, 1), CARRY]
GEOMETRY_IDS = [f"n{n}-mb{mb}-B{B}" for n, mb, B in GEOMETRIES]


@pytest.fixture(scope="module")
def P():
    import gswm_amd  # noqa: F401
    from gswm_amd import _native, codec, soft, trace
    return types.SimpleNamespace(codec=codec, soft=soft, trace=trace, N=_native, lib=_native.lib())


_CASES = {}


def case(n, mb, B):
    """one set of latents (float64 on the host), records and threshold tables per geometry, shared by every dtype and left unchanged"""
    c = _CASES.get((n, mb, B))
    if c is None:
        rs = np.random.RandomState(n + 131 * mb + B)
        rows, recs = make_records(B, mb, 7 * n + B)
        if (n, mb, B) == CARRY:                 # the 32-bit counter of image 0 carries at block 1, the 64-bit counter of image 1 wraps at block 2
            recs = counter_carry_rows(rows, mb)
        z = rs.standard_normal((B, n)) * rs.uniform(0.5, 3.0, (B, 1))
        tables = {}
        for levels in (1, 2, 15):
            shared = np.abs(rs.standard_normal(levels) * 1.5).astype(np.float32)               # in no order: the level is a count, not a search
            own = np.sort(np.abs(rs.standard_normal((B, levels)) * 2.0), axis=1).astype(np.float32)
            tables[levels] = (shared, own)
        c = _CASES[(n, mb, B)] = types.SimpleNamespace(z=z, rows=rows, recs=recs, tables=tables)
    return c


_INT = {F16: torch.int16, BF16: torch.int16, F32: torch.int32, F64: torch.int64}


def nudge(v, dtype, k):
    """the value k representable steps away from v (away from zero for k > 0) in `dtype`, as a Python float"""
    t = torch.tensor([v], dtype=F64).to(dtype)
    t.view(_INT[dtype]).add_(k)
    return float(t.double())


def device_outputs(res):
    return {k: getattr(res, k).cpu().numpy() for k in OUTPUTS}


def assert_same(got, want, what=""):
    for k in OUTPUTS:
        g, w = np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)
        assert g.shape == w.shape and np.array_equal(g, w), f"{what}: {k} differs at {np.argwhere(g != w)[:4].tolist()}"


# ------------------------------------------------------------------------------------------------ exact parity
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n,mb,B", GEOMETRIES, ids=GEOMETRY_IDS)
def test_all_outputs_equal_the_restatement(P, n, mb, B, dtype):
    c = case(n, mb, B)
    z = torch.from_numpy(c.z).to(dtype).cuda()
    zw = R.widen(z)
    rows = torch.from_numpy(c.rows).cuda()
    for levels in (1, 2, 15):
        for per_image, thr in enumerate(c.tables[levels]):
            res = P.codec.extract_soft(z, rows, mb, torch.from_numpy(thr).cuda())
            assert res.score.dtype == torch.int32 and tuple(res.score.shape) == (B, 8 * mb) and tuple(res.bits.shape) == (B, mb)
            assert_same(device_outputs(res), R.soft_vote_batch(zw, c.recs, thr, mb), f"levels {levels}, {'per-image' if per_image else 'shared'} table")


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_one_level_at_zero_is_the_keyed_extract(P, dtype):
    """levels = 1, thr = {0} on NaN-free input: the bits are `extract_records`' bits and score = 2 counts - copies"""
    for n, mb, B in ((3840, 15, 3), (16384, 32, 5)):
        c = case(n, mb, 70)
        z = torch.from_numpy(c.z[:B]).to(dtype).cuda()
        rows = torch.from_numpy(c.rows[:B]).cuda()
        res = P.codec.extract_soft(z, rows, mb, torch.zeros(1, dtype=torch.float32, device="cuda"))
        bits, flags, matches, counts = P.codec.extract_records(z, rows, mb, return_counts=True)
        copies = n // (8 * mb)
        assert torch.equal(res.bits, bits) and torch.equal(res.flags, flags) and torch.equal(res.matches, matches)
        assert torch.equal(res.score, 2 * counts - copies)
        assert torch.equal(res.wsum, torch.full_like(res.wsum, copies)) and res.wsq.tolist() == [n] * B


# ------------------------------------------------------------------------------------------------ special values
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_special_values(P, dtype):
    """+-0, +-inf, NaN, elements exactly on a threshold (and one step either side of it), a saturated element: levels as defined, flags as `extract_records`"""
    n, mb, B = 256, 2, 4
    thr = np.array([0.0, 0.5, 1.25, 3.0], dtype=np.float32)                   # representable in fp16 and bf16
    rs = np.random.RandomState(3)
    z = torch.from_numpy(rs.standard_normal((B, n))).to(dtype)
    inf = float("inf")
    z[0, :12] = torch.tensor([0.0, -0.0, inf, -inf, 0.5, -0.5, 1.25, -1.25, 3.0, -3.0, nudge(0.5, dtype, -1), nudge(1.25, dtype, -1)], dtype=F64).to(dtype)
    z[1, :4] = torch.tensor([float("nan"), -float("nan"), nudge(0.5, dtype, 1), -nudge(1.25, dtype, 1)], dtype=F64).to(dtype)
    assert float(z[0, 10]) < 0.5 and float(z[0, 11]) < 1.25 and float(z[1, 2]) > 0.5 and float(z[1, 3]) < -1.25
    z[1, 9] = float("nan")
    z[2, 17] = SAT                                                            # saturated: flagged, and still votes with the top level
    z[2, 18] = -SAT
    z[3, 5], z[3, 6] = inf, float("nan")
    zw = R.widen(z)
    lv = R.levels_of(zw[0], thr)
    assert lv[:12].tolist() == [1, 1, 4, 4, 2, 2, 3, 3, 4, 4, 1, 2]
    lv = R.levels_of(zw[1], thr)
    assert lv[:4].tolist() == [0, 0, 2, 3] and lv[9] == 0
    assert R.levels_of(zw[2], thr)[17:19].tolist() == [4, 4]
    rows_h, recs = make_records(B, mb, 11)
    rows, zd = torch.from_numpy(rows_h).cuda(), z.cuda()
    res = P.codec.extract_soft(zd, rows, mb, torch.from_numpy(thr).cuda())
    want = R.soft_vote_batch(zw, recs, thr, mb)
    assert_same(device_outputs(res), want)
    sat, nan = P.N.GSW_FLAG_SATURATED, P.N.GSW_FLAG_NAN                       # (+inf is beyond 8.2924 as well)
    assert res.flags.tolist() == [sat, nan, sat, sat | nan] == want["flags"].tolist()
    assert torch.equal(res.flags, P.codec.extract_records(zd, rows, mb)[1])
    # the level is a count: a table in no order, with repeated, negative, zero, infinite and NaN entries (a NaN threshold counts nothing)
    odd = np.array([3.0, np.nan, 0.5, 0.5, -0.0, -1.0, np.inf, 1.25, np.nan, 0.0], dtype=np.float32)
    assert R.levels_of(zw[0], odd)[:12].tolist() == [3, 3, 8, 8, 5, 5, 6, 6, 7, 7, 3, 5] and R.levels_of(zw[1], odd)[:2].tolist() == [0, 0]
    for table in (odd, odd[:7], odd[:3], odd[1:2]):
        res = P.codec.extract_soft(zd, rows, mb, torch.from_numpy(np.ascontiguousarray(table)).cuda())
        assert_same(device_outputs(res), R.soft_vote_batch(zw, recs, table, mb), f"table {table.tolist()}")
    # fp64 is compared in fp64: a value that rounds onto the threshold in fp32 stays below it
    if dtype == F64:
        z2 = torch.full((1, n), 0.25, dtype=F64)
        z2[0, 0], z2[0, 1] = 0.5 - 2.0 ** -40, 0.5
        r2 = P.codec.extract_soft(z2.cuda(), rows[:1], mb, torch.from_numpy(thr).cuda())
        assert_same(device_outputs(r2), R.soft_vote_batch(R.widen(z2), recs[:1], thr, mb))
        assert R.levels_of(R.widen(z2)[0], thr)[:2].tolist() == [1, 2]


# ------------------------------------------------------------------------------------------------ poisoned, guard-banded outputs
@pytest.mark.parametrize("pattern", [NAN, FINITE], ids=["nan", "finite"])
def test_every_output_element_is_written_and_nothing_else(P, pattern):
    for (n, mb, B), dtype in (((3840, 15, 70), F16), ((256, 1, 3), F64), ((16384, 32, 3), BF16)):
        c = case(n, mb, B)
        ledger = Ledger(pattern)
        z = ledger.wrap(torch.from_numpy(c.z).to(dtype).cuda())
        rows = ledger.wrap(torch.from_numpy(c.rows).cuda())
        thr_h = c.tables[15][1]
        thr = ledger.wrap(torch.from_numpy(thr_h).cuda())
        with poisoned(ledger):
            res = P.codec.extract_soft(z, rows, mb, thr)
        torch.cuda.synchronize()
        want = R.soft_vote_batch(R.widen(z), c.recs, thr_h, mb)
        # an output that equals the pattern by value is told apart by the restatement: only elements that are wrong AND still hold the pattern are unwritten
        for k in OUTPUTS:
            t = getattr(res, k)
            same = torch.from_numpy(np.asarray(want[k]).astype(np.int64)).cuda() == t.to(torch.int64)
            assert bool(same.all()), f"{k}: {ledger.untouched(t)} elements still hold the pattern; {ledger.where(t)}"
        ledger.check()
        # the optional outputs passed as NULL: the rest is written as before, nothing outside
        M = 8 * mb
        bits, flags = ledger.empty((B, mb), torch.uint8, "cuda"), ledger.empty((B,), torch.int32, "cuda")
        score = ledger.empty((B, M), torch.int32, "cuda")
        wide = ledger.wrap(torch.from_numpy(np.pad(thr_h, ((0, 0), (0, 5)), constant_values=np.nan)).cuda())       # thr_stride 20 > levels
        st = torch.cuda.current_stream().cuda_stream
        args = (z.data_ptr(), P.codec._dt(dtype), rows.data_ptr(), rows.shape[1], mb, wide.data_ptr(), 20, 15)
        assert P.lib.gsw_extract_soft(*args, bits.data_ptr(), None, None, None, flags.data_ptr(), None, B, n, st) == 0
        torch.cuda.synchronize()
        assert torch.equal(bits, res.bits) and torch.equal(flags, res.flags)
        assert P.lib.gsw_extract_soft(*args, bits.data_ptr(), score.data_ptr(), None, None, flags.data_ptr(), None, B, n, st) == 0
        torch.cuda.synchronize()
        assert torch.equal(score, res.score) and torch.equal(bits, res.bits)
        ledger.check()
        ledger.release()


# ------------------------------------------------------------------------------------------------ streams, wrapper refusals
def test_runs_on_a_non_default_stream(P):
    n, mb, B = 16384, 32, 70
    c = case(n, mb, B)
    z, rows = torch.from_numpy(c.z).to(F16).cuda(), torch.from_numpy(c.rows).cuda()
    thr = torch.from_numpy(c.tables[15][1]).cuda()
    want = P.codec.extract_soft(z, rows, mb, thr)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        assert torch.cuda.current_stream().cuda_stream == s.cuda_stream != torch.cuda.default_stream().cuda_stream
        got = P.codec.extract_soft(z, rows, mb, thr)
    s.synchronize()
    for k in OUTPUTS:
        assert torch.equal(getattr(got, k), getattr(want, k)), k


def test_wrapper_refuses_bad_operands(P):
    n, mb, B = 256, 1, 3
    c = case(n, mb, B)
    z, rows = torch.from_numpy(c.z).to(F32).cuda(), torch.from_numpy(c.rows).cuda()
    thr = torch.from_numpy(c.tables[2][1]).cuda()
    P.codec.extract_soft(z, rows, mb, thr)
    with pytest.raises(ValueError, match="z must be contiguous"):
        P.codec.extract_soft(torch.from_numpy(c.z).to(F32).cuda().t().contiguous().t(), rows, mb, thr)
    with pytest.raises(ValueError, match="thresholds must be contiguous"):
        P.codec.extract_soft(z, rows, mb, thr.t().contiguous().t())
    with pytest.raises(RuntimeError, match="z must live on a HIP device"):
        P.codec.extract_soft(z.cpu(), rows, mb, thr)
    with pytest.raises(RuntimeError, match="thresholds must live on a HIP device"):
        P.codec.extract_soft(z, rows, mb, thr.cpu())
    with pytest.raises(RuntimeError, match="records must live on a HIP device"):
        P.codec.extract_soft(z, rows.cpu(), mb, thr)
    with pytest.raises(ValueError, match="thresholds must be float32"):
        P.codec.extract_soft(z, rows, mb, thr.double())
    with pytest.raises(ValueError, match="thresholds must be float32"):
        P.codec.extract_soft(z, rows, mb, thr[:2].contiguous())
    with pytest.raises(ValueError, match="levels"):
        P.codec.extract_soft(z, rows, mb, torch.zeros(16, device="cuda"))
    with pytest.raises(ValueError, match="unsupported dtype"):
        P.codec.extract_soft(z.to(torch.int32), rows, mb, thr)
    with pytest.raises(ValueError, match="images"):
        P.codec.extract_soft(z[:2].contiguous(), rows, mb, thr)
    with pytest.raises(IndexError):
        P.codec.extract_soft(z[:, :248].contiguous(), rows, 2, thr)          # 248 elements, 16-bit message
    with pytest.raises(ValueError, match="whole bytes"):
        P.codec.extract_soft(z[:, :252].contiguous(), rows, mb, thr)


# ------------------------------------------------------------------------------------------------ behaviour on the device
def test_level_vote_beats_the_sign_vote_on_noisy_embedded_images(P):
    """32 images under 32 keys (`embed_records`), CPU-generated seeded noise at sigma = 3, fp16: the level vote with `uniform_thresholds` recovers at least
    120 bits more than `extract_records`, and both numbers are the restatement's for the same arrays"""
    B, mb, shape = 32, 32, (4, 64, 64)
    rows_h, recs = make_records(B, mb, 99)
    rows = torch.from_numpy(rows_h).cuda()
    clean = P.codec.embed_records(rows, mb, shape, seed=5, dtype=F32)
    noise = torch.randn((B, *shape), generator=torch.Generator().manual_seed(17)) * 3.0
    z = (clean + noise.cuda()).to(F16)
    thr = P.soft.uniform_thresholds(z, 15)
    assert thr.is_cuda and thr.dtype == torch.float32 and tuple(thr.shape) == (B, 15)
    soft = P.codec.extract_soft(z, rows, mb, thr)
    hard = P.codec.extract_records(z, rows, mb)
    s, h = int(soft.matches.sum()), int(hard[2].sum())
    print(f"sigma 3 on the device: level vote {s} / 8192 bits, sign vote {h} / 8192")
    assert s - h >= 120
    zw = R.widen(z)
    want_soft = R.soft_vote_batch(zw, recs, thr.cpu().numpy(), mb)
    want_hard = R.soft_vote_batch(zw, recs, R.sign_thresholds(), mb)
    assert_same(device_outputs(soft), want_soft)
    assert s == int(want_soft["matches"].sum()) and h == int(want_hard["matches"].sum())
    assert np.array_equal(hard[0].cpu().numpy(), want_hard["bits"])
    # the thresholds are the definition's, from the image's own RMS
    rms = np.sqrt((zw.astype(np.float64) ** 2).mean(axis=1))
    np.testing.assert_allclose(thr.cpu().numpy(), rms[:, None] * ((np.arange(1, 16) - 0.5) * 2.5 / 15)[None, :], rtol=1e-5)
    # the shared-key convenience: the same launch with one record for all images and no message to compare with
    key, nonce, _ = recs[0]
    one = P.soft.extract_soft(z, key, nonce, 8 * mb, thresholds=thr)
    assert one.matches is None and torch.equal(one.score[0], soft.score[0]) and torch.equal(one.bits[0], soft.bits[0])
    assert torch.equal(P.soft.extract_soft(z, key, nonce, 8 * mb).score, one.score)


def test_trace_with_reliability_levels(P):
    """a 1000-message registry under one key, sigma = 4: indices and (halved) scores are the restatement's top-k, the true user comes first, and its bound is
    below the Hoeffding-form value of the margin statistic for the same image (both computed from the restatement)"""
    trace = P.trace
    rs = np.random.RandomState(2024)
    key, nonce = rs.bytes(32), rs.bytes(16)
    reg = trace.Registry(32)
    msgs = [rs.bytes(32) for _ in range(1000)]
    for i, m in enumerate(msgs):
        reg.add(f"user{i}", m)
    users, shape, M, T, k = [17, 640, 999], (4, 64, 64), 256, 15, 4
    n = int(np.prod(shape))
    V = n // M
    clean = torch.cat([P.codec.embed_batch(key, nonce, msgs[u], 1, shape, seed=u, image_index0=u, dtype=F32) for u in users])
    noise = torch.randn((len(users), *shape), generator=torch.Generator().manual_seed(4)) * 4.0
    # brought back to unit variance, as inverted latents are: the votes and the RMS-scaled levels do not depend on the scale, and no element then reaches
    # 8.2924, for which `trace_latents` reports the reference's ValueError instead of a result
    z = ((clean + noise.cuda()) / (1.0 + 4.0 ** 2) ** 0.5).to(F16)
    out = trace.trace_latents(z, key, nonce, reg, k=k, reliability=T)
    # the restatement
    thr = P.soft.uniform_thresholds(z, T).cpu().numpy()
    zw = R.widen(z)
    shared = [(key, nonce, bytes(32))] * len(users)
    lev = R.soft_vote_batch(zw, shared, thr, 32)
    sign = R.soft_vote_batch(zw, shared, R.sign_thresholds(), 32)
    pm = 2 * np.unpackbits(reg.packed(M), axis=1).astype(np.int64) - 1
    totals, margins = lev["score"] @ pm.T, sign["score"] @ pm.T
    order = np.argsort(-totals, axis=1, kind="stable")[:, :k]
    for b, u in enumerate(users):
        r = out[b]
        assert isinstance(r, trace.TraceResult) and len(r.candidates) == k
        assert [c.index for c in r.candidates] == order[b].tolist()
        assert [c.score for c in r.candidates] == totals[b, order[b]].tolist()
        best = r.candidates[0]
        assert best.index == u and best.user_id == f"user{u}" and r.attributed == f"user{u}"
        assert best.agree == M - int(np.unpackbits(lev["bits"][b] ^ np.frombuffer(msgs[u], dtype=np.uint8)).sum())
        level_bound = trace.log10_p_any(P.soft.log10_p(int(totals[b, u]), int(lev["wsq"][b])), 1000)
        margin_bound = trace.log10_p_any(P.soft.log10_p(int(margins[b, u]), M * V), 1000)
        print(f"user {u}: level-weighted log10 p {level_bound:.1f}, margins in Hoeffding form {margin_bound:.1f}")
        assert best.log10_p_any == pytest.approx(level_bound, rel=1e-12)
        assert best.log10_p_any < margin_bound
    # the default statistic is unchanged by the new argument
    plain, again = trace.trace_latents(z, key, nonce, reg, k=k), trace.trace_latents(z, key, nonce, reg, k=k, reliability=None)
    assert [[(c.index, c.score, c.log10_p_any) for c in r.candidates] for r in plain] == [[(c.index, c.score, c.log10_p_any) for c in r.candidates] for r in again]
    assert [c.score for c in plain[0].candidates] == np.sort(margins[0])[::-1][:k].tolist()
