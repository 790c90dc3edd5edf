"""GPU: one record per image -- `codec.embed_records` / `codec.extract_records` (gsw_embed_keyed / gsw_extract_keyed), `issue.issue_latents` and the
pipeline's `embed_records` / `verify_records`.

The identities are exact: row b of either result is compared bit for bit with the shared-key kernels (`embed_batch` / `extract_batch`) called for that one
image with record b's key, nonce and message.  The NumPy oracle checks the planted cipher bits independently of both kernels."""
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
from record_rows import counter_carry_rows, make_records  # noqa: E402

pytestmark = pytest.mark.gpu

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
DTYPES = [F32, F16, BF16, F64]
DTYPE_IDS = ["f32", "f16", "bf16", "f64"]
_INT = {2: torch.int16, 4: torch.int32, 8: torch.int64}
SAT = 8.3125            # >= 8.2924 (the quantiser saturates from 8.292361075813597) and representable in fp16 and bf16, so the cast keeps it there


@pytest.fixture(scope="module")
def P():
    import gswm_amd  # noqa: F401
    from gswm_amd import _native, codec, ddim, issue, pipeline, trace
    return types.SimpleNamespace(codec=codec, ddim=ddim, issue=issue, pipeline=pipeline, trace=trace, N=_native, lib=_native.lib())


def _bits(t):
    return t.contiguous().view(_INT[t.element_size()])


def _n(shape):
    return int(np.prod(shape))


def make_u(B, n, seed):
    u = np.random.RandomState(seed).uniform(0, 1, (B, n))
    q = n // 4
    u[0, :q] = 0.0                              # -inf for a 0 window
    u[0, q:2 * q] = 1.0 - 2.0 ** -53            # the largest double below 1
    return torch.from_numpy(u).cuda()


def reference_embed(P, recs, shape, *, u, seed, i0, dtype, fast, l):
    rows = [P.codec.embed_batch(k, n, m, 1, shape, u=None if u is None else u[b:b + 1], seed=seed, image_index0=i0 + b, dtype=dtype, fast=fast, l=l)
            for b, (k, n, m) in enumerate(recs)]
    return torch.cat(rows)


def assert_same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not torch.equal(g, w):
        bad = (g != w).reshape(g.shape[0], -1)
        rows = bad.any(dim=1).nonzero().flatten().tolist()
        first = bad[rows[0]].nonzero().flatten()[0].item()
        raise AssertionError(f"{what}: {int(bad.sum())} elements differ, images {rows[:8]}, first at element {first} of image {rows[0]}")


# (shape, B, msg_bytes): 256 elements (less than one ChaCha block at l = 1), 1700 (partial last chunk, zero-plaintext tail), the 8- and 18-chunk lattices;
# B crosses every group size (16 / l and its halves); a 256-byte message at 1700 elements never fits once (all-zero plaintext)
EMBED_COMBOS = [((4, 8, 8), 1, 1), ((4, 17, 25), 3, 4), ((4, 64, 64), 17, 32), ((4, 96, 96), 33, 128), ((4, 17, 25), 33, 256), ((4, 8, 8), 17, 32)]


# ------------------------------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("rng", ["philox", "u"])
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("l", [1, 2, 4])
def test_embed_identity(P, l, dtype, fast, rng):
    for j, (shape, B, mb) in enumerate(EMBED_COMBOS):
        n = _n(shape)
        rows, recs = make_records(B, mb, 100 * l + j)
        u = make_u(B, n, j) if rng == "u" else None
        kw = dict(u=u, seed=0xC0FFEE + j, dtype=dtype, fast=fast, l=l)
        got = P.codec.embed_records(torch.from_numpy(rows).cuda(), mb, shape, image_index0=7, **kw)
        assert got.shape == (B, *shape) and got.dtype == dtype
        assert_same_bits(got, reference_embed(P, recs, shape, i0=7, **kw), f"{shape} B={B} msg_bytes={mb}")


def test_embed_identity_large_image_index_wide_stride_and_out(P):
    shape, B, mb = (4, 64, 64), 5, 32
    rows, recs = make_records(B, mb, 5, stride=128)                     # rows wider than key | nonce | message need
    i0 = 2 ** 32 - 2                                                    # the global image index crosses 2^32 inside the batch
    out = torch.empty((B, *shape), dtype=F16, device="cuda")
    got = P.codec.embed_records(torch.from_numpy(rows).cuda(), mb, shape, seed=11, image_index0=i0, fast=True, out=out)
    assert got is out
    assert_same_bits(got, reference_embed(P, recs, shape, u=None, seed=11, i0=i0, dtype=F16, fast=True, l=1), "image_index0 = 2^32 - 2")


@pytest.mark.parametrize("l", [1, 4])
def test_embed_identity_block_counter_carries_inside_the_lattice(P, l):
    # 36864 l bits = 72 l ChaCha blocks: the 32-bit counter of image 0 carries at block 1, of image 1 at block 2, of image 2 at block 256 (l = 4 only)
    shape, B, mb = (4, 96, 96), 3, 32
    rows, _ = make_records(B, mb, 9)
    for b, c in enumerate((0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFF00)):
        rows[b, 32:36] = np.frombuffer(int(c).to_bytes(4, "little"), dtype=np.uint8)
    rows[1, 36:40] = 0xFF                                                # and the carry runs on into the third word's neighbour
    recs = [(bytes(r[:32]), bytes(r[32:48]), bytes(r[48:48 + mb])) for r in rows]
    got = P.codec.embed_records(torch.from_numpy(rows).cuda(), mb, shape, seed=3, l=l)
    assert_same_bits(got, reference_embed(P, recs, shape, u=None, seed=3, i0=0, dtype=F32, fast=False, l=l), "counter carry")
    if l == 1:
        for b, (k, nn, m) in enumerate(recs):
            assert np.array_equal((~torch.signbit(got[b])).cpu().numpy().reshape(-1).astype(np.uint8), O.cipher_bits(m, k, nn, _n(shape)))


# ------------------------------------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("shape,B,mb", [((4, 8, 8), 3, 1), ((4, 17, 25), 17, 4), ((4, 64, 64), 33, 32), ((4, 96, 96), 5, 256)])
def test_sign_bits_are_the_oracles_cipher_bits(P, shape, B, mb):
    n = _n(shape)
    rows, recs = make_records(B, mb, 21)
    z = P.codec.embed_records(torch.from_numpy(rows).cuda(), mb, shape, seed=5, dtype=F32)
    ones = (~torch.signbit(z)).reshape(B, n).cpu().numpy().astype(np.uint8)         # cipher bit 1 <-> the upper half
    for b, (k, nn, m) in enumerate(recs):
        assert np.array_equal(ones[b], O.cipher_bits(m, k, nn, n)), f"image {b}"


# ------------------------------------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("l,fast", [(1, True), (2, False), (4, True)])
def test_split_invariance(P, l, fast):
    shape, B, mb = (4, 64, 64), 17, 32
    rows, _ = make_records(B, mb, 31)
    dev = torch.from_numpy(rows).cuda()
    kw = dict(seed=77, dtype=F16, fast=fast, l=l)
    whole = P.codec.embed_records(dev, mb, shape, image_index0=40, **kw)
    a = P.codec.embed_records(dev[0:5], mb, shape, image_index0=40, **kw)
    b = P.codec.embed_records(dev[5:17], mb, shape, image_index0=45, **kw)
    assert_same_bits(torch.cat([a, b]), whole, "rows [0:5] + [5:17]")


# ------------------------------------------------------------------------------------------------------------------------------------------ 4
CARRY_SHAPE = (4, 16, 32)       # 2048 elements, 4 l ChaCha blocks: the shape whose records count across a carry (record_rows.counter_carry_rows)


def _extract_combos(l):
    out = []
    for shape in ((4, 8, 8), (4, 17, 25), (4, 64, 64), (4, 96, 96)):
        nb = _n(shape) * l
        out += [(shape, mb) for mb in (1, 32, 256) if nb % 8 == 0 and nb % (8 * mb) == 0]
    return out + [(CARRY_SHAPE, 2)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("l", [1, 2, 4])
def test_extract_identity(P, l, dtype):
    B = 5
    combos = _extract_combos(l)
    assert {s for s, _ in combos} >= {(4, 8, 8), (4, 64, 64), (4, 96, 96), CARRY_SHAPE} and {m for _, m in combos} == {1, 2, 32, 256}
    for j, (shape, mb) in enumerate(combos):
        n, M = _n(shape), 8 * mb
        rows, recs = make_records(B, mb, 200 + j)
        if shape == CARRY_SHAPE:
            recs = counter_carry_rows(rows, mb)
        dev = torch.from_numpy(rows).cuda()
        clean = P.codec.embed_records(dev, mb, shape, seed=j, dtype=dtype, l=l)
        g = torch.Generator(device="cuda").manual_seed(j)
        noisy = (clean.double() + torch.randn(clean.shape, generator=g, device="cuda", dtype=F64)).to(dtype)
        planted = noisy.clone()
        planted.view(B, n)[1, n // 3] = float("nan")                    # image 1: NaN
        planted.view(B, n)[2, n - 1] = SAT                              # image 2: saturated; image 3: both
        planted.view(B, n)[3, 0] = float("nan")
        planted.view(B, n)[3, n // 2] = 9.5
        for name, z in (("noiseless", clean), ("noisy", noisy), ("planted", planted)):
            bits, flags, matches, counts = P.codec.extract_records(z, dev, mb, l=l, return_counts=True)
            assert bits.shape == (B, mb) and counts.shape == (B, M) and flags.shape == (B,) and matches.shape == (B,)
            b3, f3, m3 = P.codec.extract_records(z, dev, mb, l=l)
            assert torch.equal(b3, bits) and torch.equal(f3, flags) and torch.equal(m3, matches)
            for b, (k, nn, m) in enumerate(recs):
                rb, rf, rc = P.codec.extract_batch(z[b:b + 1].clone(), k, nn, M, return_counts=True, l=l)       # (a row of 1700 halves is not 16-byte aligned)
                what = f"{name} {shape} msg_bytes={mb} image {b}"
                assert torch.equal(bits[b:b + 1], rb), what
                assert torch.equal(counts[b:b + 1], rc), what
                assert torch.equal(flags[b:b + 1], rf), what
            want = M - np.unpackbits(bits.cpu().numpy() ^ rows[:, 48:48 + mb], axis=1).sum(axis=1)
            assert matches.cpu().tolist() == want.tolist(), f"{name} {shape} msg_bytes={mb}"
            fl = flags.cpu().tolist()
            if name == "noiseless":
                assert matches.cpu().tolist() == [M] * B and fl == [0] * B
            if name == "planted":
                assert fl[0] == 0 and fl[4] == 0 and fl[1] == P.N.GSW_FLAG_NAN and fl[2] == P.N.GSW_FLAG_SATURATED
                assert fl[3] == P.N.GSW_FLAG_NAN | P.N.GSW_FLAG_SATURATED


def test_extract_ragged_raises_index_error(P):
    rows, _ = make_records(2, 3, 1)
    z = torch.zeros((2, 4, 64, 64), device="cuda")
    with pytest.raises(IndexError):                                     # 16384 bits are no multiple of 24
        P.codec.extract_records(z, torch.from_numpy(rows).cuda(), 3)
    with pytest.raises(IndexError):
        P.codec.extract_batch(z, bytes(rows[0, :32]), bytes(rows[0, 32:48]), 24)


# ------------------------------------------------------------------------------------------------------------------------------------------ 5
def test_the_loop_closes(P):
    rs = np.random.RandomState(4)
    reg = P.trace.KeyedRegistry(32)
    for i in range(200):
        reg.add(f"user{i:03d}", bytes(rs.randint(0, 256, 32, dtype=np.uint8)), bytes(rs.randint(0, 256, 16, dtype=np.uint8)),
                bytes(rs.randint(0, 256, 32, dtype=np.uint8)))
    own = [(i * 37) % 200 for i in range(33)]
    records = torch.from_numpy(reg.packed()[own]).cuda()
    shape = (4, 64, 64)
    z = P.codec.embed_records(records, 32, shape, seed=9).half()
    results = P.trace.trace_latents_keyed(z, reg)
    assert [r.candidates[0].user_id for r in results] == [reg.user_at(i) for i in own]
    assert [r.attributed for r in results] == [reg.user_at(i) for i in own]
    bits, flags, matches = P.codec.extract_records(z, records, 32)
    assert matches.cpu().tolist() == [256] * 33 and int(flags.abs().sum()) == 0
    assert bits.cpu().numpy().tobytes() == b"".join(reg.record_at(i)[2] for i in own)
    packed, _ = P.codec.sign_pack(z)
    agree = P.codec.tile_agreement(packed, records[:, :48].contiguous(), records[:, 48:80].contiguous(), 256, shape, 1, 8)
    assert agree.shape == (33, 8, 8) and bool((agree == 4 * 8 * 8).all())


def test_issue_latents_matches_the_reference_call_sequence_and_fills_the_registry(P, tmp_path):
    reqs = [P.issue.Request("alice", "alice@example"), P.issue.Request("bob", b"\x01" * 32, key="11" * 32, nonce="22" * 16),
            P.issue.Request("carol", "carol", key="33" * 32)]
    reg = P.trace.KeyedRegistry(32)
    log = tmp_path / "info_data.txt"
    np.random.seed(123)
    z, records = P.issue.issue_latents(reqs, registry=reg, log_path=log, dtype=F64)
    assert z.shape == (3, 4, 64, 64) and reg.user_ids == ["alice", "bob", "carol"]
    assert np.array_equal(records.cpu().numpy(), reg.packed())
    assert reg.record("carol")[1] == bytes.fromhex("33" * 16)           # gs_insert.py:33-36: the nonce from the key's bytes 8..23
    u = np.random.RandomState(123).uniform(0, 1, (3, 16384))            # what three reference calls in a row draw
    for b, uid in enumerate(reg.user_ids):
        k, nn, m = reg.record(uid)
        want = P.codec.embed_batch(k, nn, m, 1, (4, 64, 64), u=torch.from_numpy(u[b:b + 1]).cuda(), dtype=F64)
        assert_same_bits(z[b:b + 1], want, uid)
    back = P.trace.KeyedRegistry.from_info_data(log)
    assert [back.record_at(i) for i in range(3)] == [reg.record_at(i) for i in range(3)]
    z2, _ = P.issue.issue_latents(reqs, registry=reg, seed=5, image_index0=2, fast=True, dtype=F16)     # the same users again: nothing new to register
    assert len(reg) == 3
    assert_same_bits(z2, P.codec.embed_records(records, 32, (4, 64, 64), seed=5, image_index0=2, fast=True, dtype=F16), "philox")
    with pytest.raises(ValueError, match="already bound"):
        P.issue.issue_latents([P.issue.Request("alice", "someone else")], registry=reg)


# ------------------------------------------------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("shape,l", [((4, 17, 25), 2), ((4, 64, 64), 1)], ids=["1700xl2", "16384xl1"])
def test_poisoned_guard_banded_buffers(P, shape, l):
    from test_gpu_poisoned import Out, three_ways
    B, mb, n = 17, 1 if shape == (4, 17, 25) else 32, _n(shape)
    rows, recs = make_records(B, mb, 61)
    zin = P.codec.embed_records(torch.from_numpy(rows).cuda(), mb, shape, seed=1, dtype=F16, l=l)
    zin = (zin.float() + 0.7 * torch.randn(zin.shape, generator=torch.Generator(device="cuda").manual_seed(2), device="cuda")).half()
    inputs = {"records": torch.from_numpy(rows).cuda(), "u": make_u(B, n, 3), "z": zin}

    def case(i, L):
        o = Out()
        o.written["exact_u"] = P.codec.embed_records(i["records"], mb, shape, u=i["u"], dtype=F32, l=l)
        o.written["fast_philox"] = P.codec.embed_records(i["records"], mb, shape, seed=8, image_index0=3, dtype=F16, fast=True, l=l)
        o.written["exact_philox_f64"] = P.codec.embed_records(i["records"], mb, shape, seed=8, dtype=F64, l=l)
        bits, flags, matches, counts = P.codec.extract_records(i["z"], i["records"], mb, l=l, return_counts=True)
        o.written.update(bits=bits, flags=flags, matches=matches, counts=counts)
        return o

    clean = three_ways(types.SimpleNamespace(pf=None), case, inputs)
    ref = reference_embed(P, recs, shape, u=inputs["u"], seed=0, i0=0, dtype=F32, fast=False, l=l)
    assert_same_bits(clean.written["exact_u"], ref, "exact_u")
    assert not bool(torch.isnan(clean.written["fast_philox"].float()).any())


# ------------------------------------------------------------------------------------------------------------------------------------------ 7
def test_status_codes(P):
    N, lib = P.N, P.lib
    B, mb, n = 2, 32, 16384
    rows, _ = make_records(B, mb, 1)
    wide = torch.zeros(B * 80 + 64, dtype=torch.uint8, device="cuda")
    wide[:B * 80] = torch.from_numpy(rows).cuda().flatten()
    z = torch.zeros((B, n), dtype=F32, device="cuda")
    bits = torch.zeros((B, mb), dtype=torch.uint8, device="cuda")
    flags = torch.zeros(B, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    rp, zp = wide.data_ptr(), z.data_ptr()

    def embed(records=rp, stride=80, msg_bytes=mb, batch=B, n_elems=n, l=1, out=zp, dtype=N.GSW_F32):
        return lib.gsw_embed_keyed(records, stride, msg_bytes, None, 0, 0, out, dtype, batch, n_elems, 0, l, st)

    def extract(records=rp, stride=80, msg_bytes=mb, batch=B, n_elems=n, l=1, zz=zp, dtype=N.GSW_F32, b=bits.data_ptr(), f=flags.data_ptr()):
        return lib.gsw_extract_keyed(zz, dtype, records, stride, msg_bytes, b, None, f, None, batch, n_elems, l, st)

    assert embed() == N.GSW_OK and extract() == N.GSW_OK
    for call in (embed, extract):
        assert call(stride=72) == N.GSW_ERR_BAD_ARG                    # not a multiple of 16
        assert call(stride=64) == N.GSW_ERR_BAD_ARG                    # too short for key | nonce | 32 bytes
        assert call(records=rp + 4) == N.GSW_ERR_BAD_ARG               # not 16-byte aligned
        assert call(records=None) == N.GSW_ERR_BAD_ARG
        assert call(msg_bytes=0) == N.GSW_ERR_BAD_ARG
        assert call(msg_bytes=257, stride=320) == N.GSW_ERR_BAD_ARG
        assert call(batch=0) == N.GSW_ERR_BAD_ARG
        assert call(dtype=7) == N.GSW_ERR_BAD_ARG
        assert call(l=3) == N.GSW_ERR_UNSUPPORTED
    assert embed(out=None) == N.GSW_ERR_BAD_ARG and embed(n_elems=16382) == N.GSW_ERR_BAD_ARG
    assert extract(zz=None) == N.GSW_ERR_BAD_ARG and extract(b=None) == N.GSW_ERR_BAD_ARG and extract(f=None) == N.GSW_ERR_BAD_ARG
    big = torch.zeros((1, 1048576 + 256), dtype=F16, device="cuda")
    assert extract(zz=big.data_ptr(), dtype=N.GSW_F16, batch=1, n_elems=1048576 + 256) == N.GSW_ERR_UNSUPPORTED        # Nb > 1 048 576
    assert extract(zz=big.data_ptr(), dtype=N.GSW_F16, batch=1, n_elems=524288 + 128, l=4) == N.GSW_ERR_UNSUPPORTED
    assert extract(n_elems=16380) == N.GSW_ERR_UNSUPPORTED             # Nb % 8 != 0
    assert extract(msg_bytes=3) == N.GSW_ERR_RAGGED
    assert extract(zz=big.data_ptr(), dtype=N.GSW_F16, batch=1, n_elems=1048576) == N.GSW_OK                           # the largest row: 128 KiB of LDS
    torch.cuda.synchronize()


def test_wrapper_errors(P):
    codec = P.codec
    rows, _ = make_records(2, 32, 1)
    dev = torch.from_numpy(rows).cuda()
    shape = (4, 64, 64)
    z = torch.zeros((2, *shape), device="cuda")
    with pytest.raises(RuntimeError):
        codec.embed_records(torch.from_numpy(rows), 32, shape)                                  # records on the host
    with pytest.raises(RuntimeError):
        codec.extract_records(z.cpu(), dev, 32)
    for bad in (dev.int(), dev[0], dev[:, :72].contiguous(), dev[:0]):
        with pytest.raises(ValueError):
            codec.embed_records(bad, 32, shape)
        with pytest.raises(ValueError):
            codec.extract_records(z, bad, 32)
    for mb in (0, 257, 33, True):                                                               # 33: the 80-byte rows cannot hold it
        with pytest.raises(ValueError):
            codec.embed_records(dev, mb, shape)
    with pytest.raises(ValueError):
        codec.embed_records(dev, 32, shape, l=3)
    with pytest.raises(ValueError):
        codec.embed_records(dev, 32, (3, 5, 5))                         # 75 elements: not a multiple of 4
    with pytest.raises(ValueError):
        codec.embed_records(dev, 32, shape, u=torch.zeros((2, 16384), device="cuda"))           # u must be float64
    with pytest.raises(ValueError):
        codec.embed_records(dev, 32, shape, out=torch.empty((3, *shape), device="cuda"))
    with pytest.raises(ValueError):
        codec.extract_records(z[:1], dev, 32)                                                   # one image, two records
    with pytest.raises(ValueError):
        codec.extract_records(z.int(), dev, 32)
    with pytest.raises(ValueError):
        codec.extract_records(torch.zeros((2, 4, 17, 25), device="cuda"), dev, 32)              # 1700 bits: no whole bytes
    with pytest.raises(ValueError):
        codec.extract_records(torch.zeros((2, 1048576 + 256), device="cuda", dtype=F16), dev, 32)


# ------------------------------------------------------------------------------------------------------------------------------------------ 8
def analytic_eps(x, t, ctx):
    xf = x.float()
    return (0.3 * torch.tanh(xf) + 0.05 * torch.sin(xf * 3.0 + t.float() * 0.01)).to(x.dtype)


def zero_eps(x, t, ctx):
    return torch.zeros_like(x)


def test_pipeline_records(P, keys):
    key, nonce = keys
    msg = O.pad_message("lthero", 32)
    B = 5
    rows, recs = make_records(B, 32, 71)
    records = torch.from_numpy(rows).cuda()
    ctx = torch.zeros(1, 1, 1, device="cuda", dtype=F16)
    pipe = P.pipeline.GaussianShadingPipeline(analytic_eps, key, nonce, msg, num_inference_steps=10, ctx_uncond=ctx)
    before_z = pipe.embed(B, seed=2)
    before = pipe.invert_and_extract(before_z)

    z = pipe.embed_records(records, 32, seed=2, image_index0=4)
    assert_same_bits(z, P.codec.embed_records(records, 32, (4, 64, 64), seed=2, image_index0=4, dtype=F16, fast=True), "pipe.embed_records")
    x0 = pipe.generate(z, ctx.expand(B, -1, -1), guidance_scale=1.0)
    bits, flags, matches, zi = pipe.verify_records(x0, records, 32, return_latents=True)
    assert torch.equal(zi, pipe.invert(x0))
    eb, ef, em = P.codec.extract_records(zi, records, 32)
    assert torch.equal(bits, eb) and torch.equal(flags, ef) and torch.equal(matches, em)
    assert matches.cpu().tolist() == [256] * B and bits.cpu().numpy().tobytes() == b"".join(m for _, _, m in recs)

    ident = P.pipeline.GaussianShadingPipeline(zero_eps, key, nonce, msg, num_inference_steps=10, ctx_uncond=ctx)     # inversion only rescales: signs survive
    bits, flags, matches = ident.verify_records(z, records, 32)
    assert matches.cpu().tolist() == [256] * B and int(flags.abs().sum()) == 0
    assert bits.cpu().numpy().tobytes() == b"".join(m for _, _, m in recs)

    after_z = pipe.embed(B, seed=2)                                     # the shared-key methods of the same object are what they were
    after = pipe.invert_and_extract(after_z)
    assert_same_bits(after_z, before_z, "pipe.embed")
    assert_same_bits(after_z, P.codec.embed_batch(key, nonce, msg, B, (4, 64, 64), seed=2, dtype=F16, fast=True), "pipe.embed vs embed_batch")
    assert all(torch.equal(a, b) for a, b in zip(before, after))
