"""GPU: the soft-decision vote for multi-bit windows (l = 2, 4) -- `codec.extract_soft_l` (gsw_extract_soft_l),
`codec.level_pack_l` (gsw_level_pack_l), `soft.window_thresholds` / `soft.extract_soft_l`, `trace.trace_latents_keyed_soft_l`,
`detect.detect_latents_soft_l`.

Every output is an exact integer: all are compared bit for bit with the NumPy restatement (tests/soft_l_reference.py), which shares no code with the
device path; its keystream is the oracle's ChaCha20."""
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

import soft_l_reference as RL  # noqa: E402
from poison import FINITE, NAN, Ledger, poisoned  # noqa: E402
from record_rows import make_records  # noqa: E402

pytestmark = pytest.mark.gpu

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
DTYPES = [F32, F16, BF16, F64]
DTYPE_IDS = ["f32", "f16", "bf16", "f64"]
SAT = 8.3125            # >= 8.2924 (the quantiser saturates from 8.292361075813597) and representable in fp16 and bf16
OUTPUTS = ("bits", "flags", "matches", "score", "wsum", "wsq")
ROW_OUTPUTS = ("signs", "planes", "wsum", "wsq", "flags")

# (elements per image, [msg_bytes], B, [levels], windows).  4x6x8: msg_bytes 3 (l divides it at neither window: a thread's message bytes wrap) and 1;
# 4x8x8: M = 8, 16 and 256 (one and two copies); 4x16x16: M = 2048, one copy at l = 2; 4x32x32: 512 groups, a thread's second trip; 4x64x64 with 256
# bits, the production lattice; 4x128x128 at l = 4: 262 144 bits, 32 KiB of keystream next to the static LDS.  Levels 1, 3, 5, 8 and 15 select every
# bisection depth (1, 2, 3, 4, 4 steps).
GEOMETRIES = [(192, (3, 1), 3, (1, 3, 5, 8, 15), (2, 4)), (256, (1, 2, 32), 3, (1, 3, 8, 15), (2, 4)), (1024, (256,), 2, (3, 15), (2, 4)),
              (4096, (32,), 3, (1, 3, 8, 15), (2, 4)), (16384, (32,), 2, (3, 15), (2, 4)), (65536, (32,), 1, (15,), (4,))]
CASES = [(n, mbs, B, lvs, l) for n, mbs, B, lvs, ls in GEOMETRIES for l in ls]
CASE_IDS = [f"n{n}-l{l}" for n, _, _, _, l in CASES]


@pytest.fixture(scope="module")
def P():
    import gswm_amd  # noqa: F401
    from gswm_amd import _native, codec, detect, soft, trace
    return types.SimpleNamespace(codec=codec, soft=soft, trace=trace, detect=detect, N=_native, lib=_native.lib())


_LATENTS = {}


def latents(n, B):
    """one set of latents (float64 on the host) per geometry, shared by every dtype, window and table, and left unchanged"""
    z = _LATENTS.get((n, B))
    if z is None:
        rs = np.random.RandomState(n + B)
        z = _LATENTS[(n, B)] = rs.standard_normal((B, n)) * rs.uniform(0.5, 3.0, (B, 1))
    return z


def tables(B, l, levels, seed):
    """(one table for all images, in no order; one ascending table per image): the level is a count, not a search"""
    rs = np.random.RandomState(seed)
    shared = np.abs(rs.standard_normal((l, levels)) * 0.5).astype(np.float32)
    own = np.sort(np.abs(rs.standard_normal((B, l, levels)) * 0.3), axis=2).astype(np.float32)
    return shared, own


_INT = {F16: torch.int16, BF16: torch.int16, F32: torch.int32, F64: torch.int64}


def nudge(v, dtype, k):
    """the value k representable steps above v (below for k < 0) in `dtype`, as a Python float; v is rounded into dtype first"""
    t = torch.tensor([v], dtype=F64).to(dtype)
    if k:
        f = float(t.double())
        step = k if f > 0 else -k
        if f == 0.0:
            t = torch.tensor([0.0 if k > 0 else -0.0], dtype=F64).to(dtype)
            step = abs(k)
        t.view(_INT[dtype]).add_(step)
    return float(t.double())


def device_outputs(res):
    return {k: getattr(res, k).cpu().numpy() for k in OUTPUTS}


def assert_same(got, want, names=OUTPUTS, what=""):
    for k in names:
        g, w = np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)
        assert g.shape == w.shape and np.array_equal(g, w), f"{what}: {k} differs at {np.argwhere(g != w)[:4].tolist()}"


# ------------------------------------------------------------------------------------------------ exact parity
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("n,mbs,B,lvs,l", CASES, ids=CASE_IDS)
def test_all_outputs_equal_the_restatement(P, n, mbs, B, lvs, l, dtype):
    z = torch.from_numpy(latents(n, B)).to(dtype).cuda()
    Z = RL.widen64(z)
    for mb in mbs:
        rows_h, recs = make_records(B, mb, 7 * n + mb)
        rows = torch.from_numpy(rows_h).cuda()
        for levels in lvs:
            for per_image, thr in enumerate(tables(B, l, levels, n + levels)):
                what = f"msg_bytes {mb}, levels {levels}, {'per-image' if per_image else 'shared'} table"
                res = P.codec.extract_soft_l(z, rows, mb, torch.from_numpy(thr).cuda(), l)
                assert res.score.dtype == torch.int32 and tuple(res.score.shape) == (B, 8 * mb) and tuple(res.bits.shape) == (B, mb)
                assert_same(device_outputs(res), RL.soft_vote_batch(Z, recs, thr, mb, l), what=what)
                if mb == mbs[0]:
                    packed = P.codec.level_pack_l(z, torch.from_numpy(thr).cuda(), l)
                    assert tuple(packed.planes.shape) == (B, int(levels).bit_length(), n * l // 8)
                    assert_same({k: getattr(packed, k).cpu().numpy() for k in ROW_OUTPUTS}, RL.level_rows(Z, thr, l), ROW_OUTPUTS, what)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("l", [2, 4])
def test_one_level_at_zero_is_the_keyed_extract(P, l, dtype):
    """levels = 1, thr = 0 on NaN-free input: the bits are `extract_records(l=l)`'s bits and score = 2 counts - copies"""
    for n, mb, B in ((192, 3, 3), (4096, 32, 3)):
        z = torch.from_numpy(latents(n, B)).to(dtype).cuda()
        rows = torch.from_numpy(make_records(B, mb, 5)[0]).cuda()
        res = P.codec.extract_soft_l(z, rows, mb, torch.zeros((l, 1), dtype=torch.float32, device="cuda"), l)
        bits, flags, matches, counts = P.codec.extract_records(z, rows, mb, l=l, return_counts=True)
        copies = n * l // (8 * mb)
        assert torch.equal(res.bits, bits) and torch.equal(res.flags, flags) and torch.equal(res.matches, matches)
        assert torch.equal(res.score, 2 * counts - copies)
        assert torch.equal(res.wsum, torch.full_like(res.wsum, copies)) and res.wsq.tolist() == [n * l] * B


def test_l1_through_the_shared_key_form_is_extract_soft(P):
    z = torch.from_numpy(latents(4096, 3)).to(F16).cuda()
    key, nonce = bytes(range(32)), bytes(range(16))
    a, b = P.soft.extract_soft_l(z, key, nonce, 256, 1, levels=7, clip=2.0), P.soft.extract_soft(z, key, nonce, 256, levels=7, clip=2.0)
    assert a.matches is None and b.matches is None
    for k in ("bits", "flags", "score", "wsum", "wsq"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    # and at l = 2 it is codec.extract_soft_l under shared records with window_thresholds
    c = P.soft.extract_soft_l(z, key, nonce, 256, 2, levels=7, clip=2.0)
    d = P.codec.extract_soft_l(z, P.soft.shared_records(key, nonce, 32, 3, z.device), 32, P.soft.window_thresholds(z, 2, 7, 2.0), 2)
    assert c.matches is None
    for k in ("bits", "flags", "score", "wsum", "wsq"):
        assert torch.equal(getattr(c, k), getattr(d, k)), k


# ------------------------------------------------------------------------------------------------ special values
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("l", [2, 4])
def test_special_values(P, l, dtype):
    """every quantiser boundary as the dtype holds it and its two neighbours, every edge T_a + t_i and T_c - t_i and its two neighbours, +-0, +-inf, NaN,
    saturated elements: levels as defined, flags as `extract_records`; then a table in no order with a repeated, a negative and a NaN entry"""
    T = RL.boundaries(l)
    full = 1 << l
    thr = np.array([[0.0, 0.0625, 0.125, 0.25]] + [[0.0, 0.0625, 0.125, 0.046875]] * (l - 1), dtype=np.float32)      # representable in fp16 and bf16
    odd = np.array([[0.125, np.nan, 0.0625, 0.0625, -0.5, 0.0]] * l, dtype=np.float32)
    odd[l - 1] = [np.nan, 0.03125, -0.0, 0.25, 0.03125, 0.125]
    planted = []
    for j in range(1, full):
        planted += [nudge(T[j], dtype, k) for k in (-1, 0, 1)]
        for t in sorted({float(x) for x in thr.ravel()} | {float(x) for x in odd.ravel() if x == x}):
            for edge in (T[j] + t, T[j] - t):
                planted += [nudge(edge, dtype, k) for k in (-1, 0, 1)]
    planted += [0.0, -0.0, float("inf"), -float("inf"), SAT, -SAT, nudge(SAT, dtype, 1)]
    n, mb = (len(planted) + 8 + 63) // 64 * 64, 2
    assert (n * l) % (8 * mb) == 0
    rs = np.random.RandomState(3 + l)
    z = torch.from_numpy(rs.standard_normal((3, n))).to(dtype)
    z[0, :len(planted)] = torch.tensor(planted, dtype=F64).to(dtype)
    z[1, :len(planted)] = torch.tensor(planted[::-1], dtype=F64).to(dtype)            # the same values on other message bits and window phases
    z[1, n - 3], z[1, n - 2] = float("nan"), -float("nan")
    z[2, 5] = float("nan")
    z[2, 6] = float("inf")
    Z = RL.widen64(z)
    if dtype == F64:                                                                  # the planted values are the boundaries and the edges themselves
        assert all(T[j] in Z[0] and float(T[j] + 0.0625) in Z[0] and float(T[j] - 0.046875) in Z[0] for j in range(1, full))
    rows_h, recs = make_records(3, mb, 11)
    rows, zd = torch.from_numpy(rows_h).cuda(), z.cuda()
    sat, nan = P.N.GSW_FLAG_SATURATED, P.N.GSW_FLAG_NAN
    for table in (thr, odd, odd[:, :3].copy(), odd[:, 1:2].copy()):
        res = P.codec.extract_soft_l(zd, rows, mb, torch.from_numpy(table).cuda(), l)
        want = RL.soft_vote_batch(Z, recs, table, mb, l)
        assert_same(device_outputs(res), want, what=f"table {table.tolist()}")
        assert res.flags.tolist() == [sat, sat | nan, sat | nan]
        assert torch.equal(res.flags, P.codec.extract_records(zd, rows, mb, l=l)[1])
        packed = P.codec.level_pack_l(zd, torch.from_numpy(table).cuda(), l)
        assert_same({k: getattr(packed, k).cpu().numpy() for k in ROW_OUTPUTS}, RL.level_rows(Z, table, l), ROW_OUTPUTS, f"table {table.tolist()}")
    # what the definition says about the special elements, on the restatement (which the device equals)
    y, _ = RL.windows(Z[0], l)
    lv = RL.levels_of(Z[0], y, thr, l)
    base = len(planted) - 7
    assert lv[base + 2].tolist() == lv[base + 3].tolist() == [4] + [4] * (l - 1)       # +-inf: every threshold of every bit
    assert lv[base + 4].tolist() == lv[base + 5].tolist() == [4] + [4] * (l - 1)       # saturated: far in the tail, the top level
    assert lv[base][0] == 1 and lv[base + 1][0] == 1                                   # +-0: on the median's upper side by 7e-17, the zero threshold alone
    y2, _ = RL.windows(Z[2], l)
    assert RL.levels_of(Z[2], y2, thr, l)[5].tolist() == [0] * l                       # NaN
    # fp64 is compared in fp64: a value that rounds onto the edge in fp32 stays on its own side
    if dtype == F64:
        edge = float(T[full // 2 + 1] - 0.0625)
        z2 = torch.full((1, 64), 0.01, dtype=F64)
        z2[0, 0], z2[0, 1], z2[0, 2] = edge, edge * (1 + 2.0 ** -40), edge * (1 - 2.0 ** -40)
        t2 = np.full((l, 1), 0.0625, dtype=np.float32)
        r2 = P.codec.extract_soft_l(z2.cuda(), rows[:1], mb, torch.from_numpy(t2).cuda(), l)
        assert_same(device_outputs(r2), RL.soft_vote_batch(RL.widen64(z2), recs[:1], t2, mb, l))
        y3, _ = RL.windows(RL.widen64(z2)[0], l)
        assert RL.levels_of(RL.widen64(z2)[0], y3, t2, l)[:3, l - 1].tolist() == [1, 0, 1]


# ------------------------------------------------------------------------------------------------ the rows feed the unchanged searches
@pytest.mark.parametrize("l", [2, 4])
def test_level_rows_feed_the_two_soft_searches(P, l):
    n, mb, B, U = 4096, 32, 3, 5
    z = torch.from_numpy(latents(n, B)).to(F16).cuda()
    thr = P.soft.window_thresholds(z, l, 15)
    packed = P.codec.level_pack_l(z, thr, l)
    q, qflags = P.codec.quant_pack(z, l)
    assert torch.equal(packed.signs, q) and torch.equal(packed.flags, qflags)
    rows_h, recs = make_records(U, mb, 21)
    rows = torch.from_numpy(rows_h).cuda()
    idx, score = P.codec.trace_keyed_soft_topk(packed, n * l, rows, mb, k=U)
    keys = torch.from_numpy(np.ascontiguousarray(rows_h[:, :48])).cuda()
    kidx, stat = P.codec.key_search_soft_topk(packed, n * l, keys, mb, k=U)
    want_score, want_stat = np.zeros((B, U), dtype=np.int64), np.zeros((B, U), dtype=np.int64)
    for u in range(U):
        vote = P.codec.extract_soft_l(z, rows[u:u + 1].expand(B, -1).contiguous(), mb, thr, l)
        r = torch.from_numpy(np.unpackbits(np.frombuffer(recs[u][2], dtype=np.uint8)).astype(np.int64)).cuda()
        want_score[:, u] = ((2 * r - 1)[None, :] * vote.score.long()).sum(dim=1).cpu().numpy()
        want_stat[:, u] = vote.score.long().abs().sum(dim=1).cpu().numpy()
    for b in range(B):
        got = dict(zip(idx[b].tolist(), score[b].tolist()))
        assert got == {u: int(want_score[b, u]) for u in range(U)}
        got = dict(zip(kidx[b].tolist(), stat[b].tolist()))
        assert got == {u: int(want_stat[b, u]) for u in range(U)}


# ------------------------------------------------------------------------------------------------ poisoned, guard-banded outputs
@pytest.mark.parametrize("pattern", [NAN, FINITE], ids=["nan", "finite"])
def test_every_output_element_is_written_and_nothing_else(P, pattern):
    for (n, mb, B, l), dtype in (((192, 3, 3, 4), F16), ((4096, 32, 3, 2), BF16), ((256, 1, 3, 4), F64)):
        ledger = Ledger(pattern)
        z = ledger.wrap(torch.from_numpy(latents(n, B)).to(dtype).cuda())
        rows_h, recs = make_records(B, mb, 7)
        rows = ledger.wrap(torch.from_numpy(rows_h).cuda())
        thr_h = tables(B, l, 15, 9)[1]
        thr = ledger.wrap(torch.from_numpy(thr_h).cuda())
        with poisoned(ledger):
            res = P.codec.extract_soft_l(z, rows, mb, thr, l)
            packed = P.codec.level_pack_l(z, thr, l)
        torch.cuda.synchronize()
        Z = RL.widen64(z)
        # an output that equals the pattern by value is told apart by the restatement: only elements that are wrong AND still hold the pattern are unwritten
        for out, names, want in ((res, OUTPUTS, RL.soft_vote_batch(Z, recs, thr_h, mb, l)), (packed, ROW_OUTPUTS, RL.level_rows(Z, thr_h, l))):
            for k in names:
                t = getattr(out, k)
                same = torch.from_numpy(np.asarray(want[k]).astype(np.int64)).cuda() == t.to(torch.int64)
                assert bool(same.all()), f"{k}: {ledger.untouched(t)} elements still hold the pattern; {ledger.where(t)}"
        ledger.check()
        # the optional outputs passed as NULL and a table stride wider than l levels: the rest is written as before, nothing outside
        bits, flags = ledger.empty((B, mb), torch.uint8, "cuda"), ledger.empty((B,), torch.int32, "cuda")
        score = ledger.empty((B, 8 * mb), torch.int32, "cuda")
        wide = ledger.wrap(torch.from_numpy(np.pad(thr_h.reshape(B, -1), ((0, 0), (0, 4)), constant_values=np.nan)).cuda())
        st = torch.cuda.current_stream().cuda_stream
        args = (z.data_ptr(), P.codec._dt(dtype), rows.data_ptr(), rows.shape[1], mb, wide.data_ptr(), 15 * l + 4, 15, l)
        assert P.lib.gsw_extract_soft_l(*args, bits.data_ptr(), None, None, None, flags.data_ptr(), None, B, n, st) == 0
        torch.cuda.synchronize()
        assert torch.equal(bits, res.bits) and torch.equal(flags, res.flags)
        assert P.lib.gsw_extract_soft_l(*args, bits.data_ptr(), score.data_ptr(), None, None, flags.data_ptr(), None, B, n, st) == 0
        torch.cuda.synchronize()
        assert torch.equal(score, res.score) and torch.equal(bits, res.bits)
        ledger.check()
        ledger.release()


def test_entry_points_refuse_what_the_header_says(P):
    n, mb, B, l = 256, 1, 3, 2
    z = torch.from_numpy(latents(n, B)).to(F32).cuda()
    rows = torch.from_numpy(make_records(B, mb, 1)[0]).cuda()
    thr = torch.from_numpy(tables(B, l, 3, 1)[1]).cuda()
    P.codec.extract_soft_l(z, rows, mb, thr, l)
    with pytest.raises(ValueError, match="thresholds must be float32"):
        P.codec.extract_soft_l(z, rows, mb, thr[:, :1].contiguous(), l)             # one row for two window bits
    with pytest.raises(ValueError, match="thresholds must be float32"):
        P.codec.level_pack_l(z, thr[:2].contiguous(), l)
    with pytest.raises(ValueError, match="levels"):
        P.codec.level_pack_l(z, torch.zeros((l, 16), device="cuda"), l)
    with pytest.raises(ValueError, match="use `extract_soft`"):
        P.codec.extract_soft_l(z, rows, mb, thr, 1)
    with pytest.raises(IndexError):
        P.codec.extract_soft_l(z[:, :248].contiguous(), rows.new_zeros((B, 64)), 3, thr, l)      # 496 bits, a 24-bit message
    with pytest.raises(ValueError, match="multiple of 8"):
        P.codec.extract_soft_l(z[:, :252].contiguous(), rows, mb, thr, l)
    st = torch.cuda.current_stream().cuda_stream
    out = [torch.empty(4096, dtype=torch.int32, device="cuda") for _ in range(6)]
    N = P.N

    def soft(l_=l, n_=n, mb_=mb, stride=0):
        return P.lib.gsw_extract_soft_l(z.data_ptr(), N.GSW_F32, rows.data_ptr(), rows.shape[1], mb_, thr.data_ptr(), stride, 3, l_, out[0].data_ptr(),
                                        out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), out[4].data_ptr(), out[5].data_ptr(), B, n_, st)

    def pack(l_=l, n_=n, stride=0):
        return P.lib.gsw_level_pack_l(z.data_ptr(), N.GSW_F32, thr.data_ptr(), stride, 3, l_, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                      out[3].data_ptr(), out[4].data_ptr(), B, n_, st)

    assert soft() == 0 and pack() == 0
    for bad in (1, 3, 8, 0):
        assert soft(l_=bad) == N.GSW_ERR_BAD_ARG and pack(l_=bad) == N.GSW_ERR_BAD_ARG
    assert soft(n_=252) == N.GSW_ERR_UNSUPPORTED and pack(n_=252) == N.GSW_ERR_UNSUPPORTED
    assert soft(n_=1048576 // l + 8) == N.GSW_ERR_UNSUPPORTED and pack(n_=1048576 // l + 8) == N.GSW_ERR_UNSUPPORTED
    assert soft(n_=248, mb_=3) == N.GSW_ERR_RAGGED
    assert soft(stride=5) == N.GSW_ERR_BAD_ARG and pack(stride=5) == N.GSW_ERR_BAD_ARG          # neither 0 nor >= l levels
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ behaviour on the device
def noisy_embedded(P, B, seed, sigma, l, shape=(4, 32, 32), mb=32):
    """B images under B keys (`embed_records`, uniforms and noise generated on the CPU from fixed seeds), Gaussian noise `sigma` added to the latent, fp32"""
    n = int(np.prod(shape))
    rows_h, recs = make_records(B, mb, seed)
    u = np.random.RandomState(seed + 1).uniform(0, 1, (B, n))
    rows = torch.from_numpy(rows_h).cuda()
    clean = P.codec.embed_records(rows, mb, shape, u=torch.from_numpy(u).cuda(), dtype=F32, l=l)
    noise = torch.randn((B, n), generator=torch.Generator().manual_seed(seed + 2)) * sigma
    return rows, recs, (clean + noise.reshape(B, *shape).cuda()).contiguous()


@pytest.mark.parametrize("l", [2, 4])
def test_window_vote_beats_the_sign_vote_on_noisy_embedded_images(P, l):
    """40 images of 4x32x32 under 40 keys, 256-bit messages, sigma = 1.0, fp32: the 15-level vote with `window_thresholds` recovers strictly more of the
    10 240 message bits than `extract_records(l=l)`, and both totals are the restatement's for the same arrays.  The restatement on the CPU alone (scipy's
    ndtri for the embed, the same seeds) gives 9930 against 9652 at l = 2 and 9199 against 8649 at l = 4."""
    B, mb = 40, 32
    rows, recs, z = noisy_embedded(P, B, 100 + l, 1.0, l)
    thr = P.soft.window_thresholds(z, l, 15)
    assert thr.is_cuda and thr.dtype == torch.float32 and tuple(thr.shape) == (B, l, 15)
    soft_total = int(P.codec.extract_soft_l(z, rows, mb, thr, l).matches.sum())
    hard_total = int(P.codec.extract_records(z, rows, mb, l=l)[2].sum())
    Z = RL.widen64(z)
    want_soft = int(RL.soft_vote_batch(Z, recs, thr.cpu().numpy(), mb, l)["matches"].sum())
    want_hard = int(RL.soft_vote_batch(Z, recs, np.zeros((l, 1), dtype=np.float32), mb, l)["matches"].sum())     # one level at 0: the sign vote
    print(f"l = {l}: window vote {soft_total} (restatement {want_soft}), sign vote {hard_total} (restatement {want_hard}) of {B * 8 * mb}")
    assert soft_total == want_soft and hard_total == want_hard
    assert soft_total > hard_total


def test_detect_and_trace_name_six_noisy_images(P):
    """Six latents at l = 2, sigma = 1.0 (the restatement on the CPU puts every one of them below 10^-130 under its own key and at 10^0 under every
    other, and unwatermarked noise at 10^-0.15 at the least): a 12-key keyring names all six keys at fpr 1e-6 and reads the soft vote's messages, pure
    noise names none; inside a 200-record keyed registry all six are attributed, none wrongly (restatement: 10^-190 at the most, runners-up at 10^0)."""
    l, mb, shape = 2, 32, (4, 32, 32)
    rows, recs, z = noisy_embedded(P, 6, 300, 1.0, l)
    rs = np.random.RandomState(77)
    ring = P.detect.Keyring()
    for i in range(12):
        key, nonce = bytes(rs.randint(0, 256, 32, dtype=np.uint8)), bytes(rs.randint(0, 256, 16, dtype=np.uint8))
        if i % 2 == 0:
            key, nonce = recs[i // 2][0], recs[i // 2][1]
        ring.add(f"key{i}", key, nonce)
    found = P.detect.detect_latents_soft_l(z, ring, 8 * mb, l, levels=15, fpr=1e-6)
    assert [r.key_id for r in found] == [f"key{2 * b}" for b in range(6)]
    vote = P.codec.extract_soft_l(z, rows, mb, P.soft.window_thresholds(z, l, 15), l)
    assert [r.message for r in found] == [bytes(v) for v in vote.bits.cpu().numpy()]
    assert all(r.candidates[0].log10_p_any < -100 for r in found)
    noise = torch.randn((6, *shape), generator=torch.Generator().manual_seed(5)).cuda()
    none = P.detect.detect_latents_soft_l(noise, ring, 8 * mb, l, levels=15, fpr=1e-6)
    assert [r.key_id for r in none] == [None] * 6 and all(r.message is None for r in none)
    # the same six inside a registry of 200 records that carry their own keys
    _, recs200 = make_records(200, mb, 999)
    pos = [3, 50, 77, 120, 150, 199]
    for b, p in enumerate(pos):
        recs200[p] = recs[b]
    reg = P.trace.KeyedRegistry(mb)
    for i, (key, nonce, msg) in enumerate(recs200):
        reg.add(f"user{i}", key, nonce, msg)
    traced = P.trace.trace_latents_keyed_soft_l(z, reg, l, levels=15, k=2, fpr=1e-6)
    assert [t.attributed for t in traced] == [f"user{p}" for p in pos]
    for t, m in zip(traced, vote.matches.tolist()):
        assert t.candidates[0].agree == m and t.candidates[0].log10_p_any < -100 and t.candidates[1].log10_p_any > -6.0
    assert [t.attributed for t in P.trace.trace_latents_keyed_soft_l(noise, reg, l, levels=15, fpr=1e-6)] == [None] * 6


def test_runs_on_a_non_default_stream(P):
    n, mb, B, l = 4096, 32, 3, 4
    z, rows = torch.from_numpy(latents(n, B)).to(F16).cuda(), torch.from_numpy(make_records(B, mb, 2)[0]).cuda()
    thr = torch.from_numpy(tables(B, l, 15, 2)[1]).cuda()
    want, want_rows = P.codec.extract_soft_l(z, rows, mb, thr, l), P.codec.level_pack_l(z, thr, l)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        assert torch.cuda.current_stream().cuda_stream == s.cuda_stream != torch.cuda.default_stream().cuda_stream
        got, got_rows = P.codec.extract_soft_l(z, rows, mb, thr, l), P.codec.level_pack_l(z, thr, l)
    s.synchronize()
    for k in OUTPUTS:
        assert torch.equal(getattr(got, k), getattr(want, k)), k
    for k in ROW_OUTPUTS:
        assert torch.equal(getattr(got_rows, k), getattr(want_rows, k)), k
