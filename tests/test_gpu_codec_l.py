"""GPU: the codec with multi-bit windows (l = 2, 4) -- gsw_embed_l, gsw_extract_l, gsw_quant_pack through the package's wrappers against
a restatement that lives in this file, built from the oracle's ChaCha20 and scipy's ndtr / ndtri.

Semantics restated ("Multi-bit windows"): Nb = n l cipher bits = keystream XOR the message repeated floor(Nb / |k|) times then
zeros, MSB first; element i takes bits [i l, i l + l), first bit = MSB of y_i; z_i = ndtri((u_i + y_i) / 2^l), stored as the representable
value nearest to z_i that quantises to y_i; quantise y = int(ndtr(float64(z)) 2^l), saturation (ndtr == 1) packs as all ones, NaN as zeros;
extract = l bits per element, XOR keystream, strict majority over Nb / M copies.

Tolerances: bytes, bits, counts, flags and every quantised y are exact.  fp64 latents: 1e-12 absolute against scipy (the project's l = 1
gate).  fp16 / bf16 / fp32 latents: at most one ulp of that dtype from the restated bin-safe rounding (the kernel rounds fp64 -> fp32 ->
dtype, the restatement fp64 -> dtype).  Fast mode: |dz| <= 1e-5 in fp32 against exact mode, the project's l = 1 gate."""
import functools
import json
import os
import types

import numpy as np
import pytest
import torch
from scipy.special import ndtr, ndtri

import gs_oracle as O
from conftest import GOLDEN, README_KEY, README_NONCE

pytestmark = pytest.mark.gpu

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
DTYPES = [F16, BF16, F32, F64]
DT_IDS = ["f16", "bf16", "f32", "f64"]
WINDOWS = [2, 4]
SAT = 8.292361075813597                       # the smallest double with ndtr(z) == 1.0
LATTICES = [(4, 1, 2), (4, 3, 3), (4, 17, 25), (4, 64, 64)]
BATCHES = [1, 3, 65]
MSG_BYTES = {8: 1, 36: 3, 1700: 32, 16384: 32}          # 4x17x25: 3400 l / 256 is not whole, the tail of the lattice carries zeros

with open(os.path.join(GOLDEN, "chacha20_keystreams.json")) as _f:
    _CH = json.load(_f)["cases"]
KEYS = {"readme": (bytes.fromhex(README_KEY), bytes.fromhex(README_NONCE)),
        "carry": (bytes.fromhex(_CH["carry"]["key_hex"]), bytes.fromhex(_CH["carry"]["nonce_hex"])),        # counter 0xfffffffe: carries after 2 blocks
        "carry2": (bytes.fromhex(_CH["carry2"]["key_hex"]), bytes.fromhex(_CH["carry2"]["nonce_hex"]))}     # counter 0xffffffff: after 1 block
KEY_OF_BATCH = {1: "readme", 3: "carry", 65: "carry2"}


@pytest.fixture(scope="module")
def G():
    import gswm_amd
    from gswm_amd import codec, pf, pipeline, trace, unet
    assert torch.cuda.is_available()
    gswm_amd._native.lib()
    return types.SimpleNamespace(codec=codec, pf=pf, pipeline=pipeline, trace=trace, unet=unet, N=gswm_amd._native)


# ---------------------------------------------------------------------------------------------------------------- the restatement
def cipher_bits(key, nonce, k, n, l):
    """the Nb = n l bits the embed plants, uint8 [Nb]"""
    nb = n * l
    ks = np.unpackbits(np.frombuffer(O.chacha20_keystream(key, nonce, nb // 8), np.uint8))
    kb = np.unpackbits(np.frombuffer(k, np.uint8))
    reps = nb // kb.size
    plain = np.concatenate([np.tile(kb, reps), np.zeros(nb - reps * kb.size, np.uint8)])
    return ks ^ plain


def windows(bits, l):
    """bits [..., n l] -> y [..., n], first bit = MSB"""
    w = bits.reshape(*bits.shape[:-1], -1, l).astype(np.int64)
    return (w << np.arange(l - 1, -1, -1)).sum(-1)


def window_bits(y, l):
    """y [..., n] -> bits [..., n l]"""
    return ((y[..., None] >> np.arange(l - 1, -1, -1)) & 1).astype(np.uint8).reshape(*y.shape[:-1], -1)


def quantise(z64, l):
    """(y as packed: saturation -> 2^l - 1, NaN -> 0; saturated mask; NaN mask)"""
    z64 = np.asarray(z64, np.float64)
    nan = np.isnan(z64)
    c = ndtr(np.where(nan, 0.0, z64))
    sat = c >= 1.0
    y = np.minimum((c * 2.0 ** l).astype(np.int64), 2 ** l - 1)
    return np.where(nan, 0, y), sat & ~nan, nan


def flags_of(z64, l, N):
    _, sat, nan = quantise(z64, l)
    return (sat.any(axis=1) * N.GSW_FLAG_SATURATED + nan.any(axis=1) * N.GSW_FLAG_NAN).astype(np.int32)


_INT = {F16: torch.int16, BF16: torch.int16, F32: torch.int32, F64: torch.int64}


def ordinal(t):
    """a float tensor -> int64 numpy array in the same order, adjacent values one apart (-0.0 and +0.0 coincide)"""
    b = t.contiguous().view(_INT[t.dtype]).numpy().astype(np.int64)
    mag = b & ((1 << (8 * t.element_size() - 1)) - 1)
    return np.where(b < 0, -mag, b)


def from_ordinal(o, dtype):
    b = np.where(o < 0, -o + np.int64(-(1 << (8 * dtype.itemsize - 1))), o)       # sign bit set: magnitude + INT_MIN of the storage integer
    return torch.from_numpy(b.astype({2: np.int16, 4: np.int32, 8: np.int64}[dtype.itemsize])).view(dtype)


@functools.lru_cache(maxsize=None)
def bin_ordinals(l, dtype):
    """per window value y: (ordinal of the smallest, ordinal of the largest) value of `dtype` that quantises to y -- bisection on scipy's
    ndtr over the ordered values of the dtype, -inf .. +inf (quantise is monotone; saturation belongs to the top window)"""
    inf = torch.tensor([float("inf")], dtype=F64).to(dtype)
    top = int(ordinal(inf)[0])
    lo = [-top]
    for y in range(1, 2 ** l):
        a, b = -top, top                                   # quantise(a) < y <= quantise(b)
        while b - a > 1:
            m = (a + b) // 2
            if quantise(from_ordinal(np.array([m]), dtype).to(F64).numpy(), l)[0][0] >= y:
                b = m
            else:
                a = m
        lo.append(b)
    hi = [x - 1 for x in lo[1:]] + [top]
    return np.array(lo), np.array(hi)


def binsafe(z64, y, l, dtype):
    """ordinal of the value of `dtype` nearest to z64 that quantises to y: round to nearest, then into the window's range of values"""
    lo, hi = bin_ordinals(l, dtype)
    return np.clip(ordinal(torch.from_numpy(np.array(z64)).to(dtype)), lo[y], hi[y])


def special_u(rs, B, n):
    """uniforms in [0, 1) with 0, 2^-53 and 1 - 2^-53 planted where they meet every window value"""
    u = rs.uniform(0, 1, (B, n))
    spec = np.array([0.0, 2.0 ** -53, 1.0 - 2.0 ** -53])
    pos = rs.permutation(n)[:min(n, 192)]
    for b in range(B):
        u[b, pos] = spec[(np.arange(pos.size) + b) % 3]
    return u


@functools.lru_cache(maxsize=None)
def embed_case(shape, B, l):
    """shared by the dtypes: inputs and the fp64 reference of one (lattice, batch, l); never modified"""
    n = int(np.prod(shape))
    key, nonce = KEYS[KEY_OF_BATCH[B]]
    rs = np.random.RandomState(1000 * l + 10 * B + n % 7)
    k = bytes(rs.randint(0, 256, MSG_BYTES[n], dtype=np.uint8))
    u = special_u(rs, B, n)
    y = windows(cipher_bits(key, nonce, k, n, l), l)                      # [n], shared by the batch
    with np.errstate(divide="ignore"):
        z = ndtri((u + y[None]) / 2.0 ** l)
    for a in (u, y, z):
        a.setflags(write=False)
    return key, nonce, k, u, y, z


def check_embed(got, shape, B, l, dtype):
    key, nonce, k, u, y, z = embed_case(shape, B, l)
    g = got.cpu().reshape(B, -1)
    yb = np.broadcast_to(y[None], z.shape)
    q, _, nan = quantise(g.to(F64).numpy(), l)
    assert not nan.any()
    assert np.array_equal(q, yb), f"{int((q != yb).sum())} of {q.size} elements quantise to another window"
    if dtype == F64:
        gz = g.numpy()
        inf = np.isinf(z)
        assert np.array_equal(gz[inf], z[inf])
        assert np.abs(gz[~inf] - z[~inf]).max(initial=0.0) <= 1e-12
    else:
        d = np.abs(ordinal(g) - binsafe(z, yb, l, dtype))
        assert d.max() <= 1, f"{int((d > 1).sum())} elements are more than one ulp from the bin-safe rounding (max {int(d.max())})"


def run_embeds(codec, l, dtype, cases):
    out = {}
    for shape, B in cases:
        key, nonce, k, u, y, z = embed_case(shape, B, l)
        out[(shape, B)] = codec.embed_batch(key, nonce, k, B, shape, u=torch.from_numpy(u).cuda(), dtype=dtype, l=l)
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. embed
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("l", WINDOWS)
def test_embed_parity_with_supplied_u(G, l, dtype):
    cases = [(s, B) for s in LATTICES for B in BATCHES]
    for (shape, B), z in run_embeds(G.codec, l, dtype, cases).items():
        assert z.shape == (B, *shape) and z.dtype == dtype
        check_embed(z, shape, B, l, dtype)


def test_embed_refuses_what_the_header_says(G):
    key, nonce = KEYS["readme"]
    with pytest.raises(ValueError):
        G.codec.embed_batch(key, nonce, b"\x01", 1, (2, 1, 1), l=4)          # n % 4, as l = 1
    with pytest.raises(ValueError, match="l must be one of"):
        G.codec.embed_batch(key, nonce, b"\x01", 1, (4, 1, 2), l=3)
    assert G.N.lib().gsw_version() == 500


# ---------------------------------------------------------------------------------------------------------------- 2. fast mode
@pytest.mark.parametrize("l", WINDOWS)
def test_fast_mode_against_exact_mode(G, l):
    codec = G.codec
    key, nonce = KEYS["readme"]
    k = O.pad_message("lthero", 32)
    B, shape, n, seed, i0 = 3, (4, 64, 64), 16384, 0xC0FFEE12345, 7
    u = codec.philox_uniform(seed, i0, B, n)
    exact = codec.embed_batch(key, nonce, k, B, shape, seed=seed, image_index0=i0, dtype=F32, l=l)
    fast = codec.embed_batch(key, nonce, k, B, shape, seed=seed, image_index0=i0, dtype=F32, fast=True, l=l)
    assert torch.equal(exact, codec.embed_batch(key, nonce, k, B, shape, u=u, dtype=F32, l=l))      # the in-kernel stream is gsw_philox_uniform's
    assert torch.equal(fast, codec.embed_batch(key, nonce, k, B, shape, u=u, dtype=F32, fast=True, l=l))
    e, f = exact.cpu().reshape(B, -1).numpy(), fast.cpu().reshape(B, -1).numpy()
    assert np.abs(e.astype(np.float64) - f).max() <= 1e-5
    y = windows(cipher_bits(key, nonce, k, n, l), l)
    assert np.array_equal(quantise(e, l)[0], np.broadcast_to(y, e.shape))
    assert np.array_equal(quantise(f, l)[0], np.broadcast_to(y, f.shape))
    # against scipy on the same u (exact mode, fp32 store: one rounding and the clamp away from fp64)
    z = ndtri((u.cpu().numpy() + y[None]) / 2.0 ** l)
    assert np.abs(e - z).max() <= 1e-5 / 8
    # the deep tail (u = 0, 2^-53, 1 - 2^-53 under every window value): the fp32 core hands over to the exact one
    key2, nonce2, k2, u2, y2, z2 = embed_case((4, 17, 25), 3, l)
    ft = codec.embed_batch(key2, nonce2, k2, 3, (4, 17, 25), u=torch.from_numpy(u2).cuda(), dtype=F32, fast=True, l=l).cpu().reshape(3, -1).numpy()
    inf = np.isinf(z2)
    assert np.array_equal(ft[inf], z2[inf].astype(np.float32))
    assert np.abs(ft[~inf] - z2[~inf]).max() <= 1e-5
    assert np.array_equal(quantise(ft, l)[0], np.broadcast_to(y2, ft.shape))


# ---------------------------------------------------------------------------------------------------------------- 3. quantise edges
def edge_values(l, dtype, thresholds):
    """float64 candidates around every threshold: itself, its fp64 neighbours and the values of `dtype` either side, plus the fixed points"""
    v = []
    for t in thresholds:
        v += [t, np.nextafter(t, -np.inf), np.nextafter(t, np.inf)]
        o = ordinal(torch.tensor([t], dtype=F64).to(dtype))
        v += from_ordinal(np.concatenate([o - 2, o - 1, o, o + 1, o + 2]), dtype).to(F64).tolist()
    v += [0.0, -0.0, -np.inf, -SAT, 1.0, -1.0]
    return np.array(v, np.float64)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("l", WINDOWS)
def test_quantise_edges(G, l, dtype):
    codec = G.codec
    thr = codec.quant_thresholds(l)
    base = edge_values(l, dtype, thr)
    # the saturation boundary as `dtype` sees it: the smallest value of the dtype that is >= SAT (SAT itself in fp64, the float above it in
    # fp32, where SAT and its fp64 predecessor round to one float) and the value of the dtype just below it
    o = ordinal(torch.tensor([SAT], dtype=F64).to(dtype))
    o = o + (from_ordinal(o, dtype).to(F64).numpy() < SAT)
    sat_d, pre_d = (float(from_ordinal(o - d, dtype).to(F64)[0]) for d in (0, 1))
    assert pre_d < SAT <= sat_d and ndtr(pre_d) < 1.0 == ndtr(sat_d)
    if dtype == F64:
        assert sat_d == SAT and pre_d == np.nextafter(SAT, -np.inf)
    n = (base.size + 2 + 7) // 8 * 8                                        # room for two planted values, whole groups of eight
    rows = np.zeros((6, n))
    rows[:, :base.size] = base
    rows[0, base.size] = pre_d                                              # image 0: the largest value below saturation: top window, NO flag
    rows[1, base.size] = np.nan                                             # image 1: a NaN
    rows[2, base.size] = sat_d                                              # image 2: the saturation point alone, nothing above it
    rows[3, base.size], rows[3, base.size + 1] = np.nan, np.inf             # image 3: a NaN and +inf
    rows[4, base.size] = np.inf                                             # image 4: +inf alone
    rows[5, base.size], rows[5, base.size + 1] = pre_d, -pre_d              # image 5: as image 0 (a flag does not leak from the image before)
    z = torch.from_numpy(rows).to(dtype)
    z64 = z.to(F64).numpy()                                                 # what the kernel is handed, as doubles
    assert np.array_equal(z64[[0, 2], base.size], [pre_d, sat_d])           # (both are values of the dtype: the cast moved neither)
    packed, flags = codec.quant_pack(z.cuda(), l)
    y = quantise(z64, l)[0]
    assert y[0, base.size] == y[2, base.size] == 2 ** l - 1                 # either side of the boundary packs as all ones: only the flag tells
    assert packed.shape == (6, n * l // 8) and packed.dtype == torch.uint8
    assert np.array_equal(packed.cpu().numpy(), np.packbits(window_bits(y, l), axis=1))
    want = flags_of(z64, l, G.N)
    SATF, NANF = G.N.GSW_FLAG_SATURATED, G.N.GSW_FLAG_NAN
    assert want.tolist() == [0, NANF, SATF, NANF | SATF, SATF, 0]
    assert flags.cpu().numpy().tolist() == want.tolist()
    # the same decisions inside the vote: one copy, so the counts are the decrypted bits themselves
    key, nonce = KEYS["carry2"]
    bits, f2, counts = codec.extract_batch(z.cuda(), key, nonce, n * l, return_counts=True, l=l)
    ks = np.unpackbits(np.frombuffer(O.chacha20_keystream(key, nonce, n * l // 8), np.uint8))
    assert np.array_equal(counts.cpu().numpy(), window_bits(y, l) ^ ks[None])
    assert np.array_equal(bits.cpu().numpy(), np.packbits(window_bits(y, l) ^ ks[None], axis=1))
    assert f2.cpu().numpy().tolist() == want.tolist()


def test_quant_pack_with_l_1_is_sign_pack(G):
    z = torch.randn(3, 4, 5, 6, generator=torch.Generator().manual_seed(2)).cuda()
    a, b = G.codec.quant_pack(z, 1), G.codec.sign_pack(z)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError):
        G.codec.quant_pack(torch.zeros(2, 6).cuda(), 2)                     # 12 bits per image


# ---------------------------------------------------------------------------------------------------------------- 4. extract
@functools.lru_cache(maxsize=None)
def latent_case(shape, B, dtype):
    """random latents (not embedded), with a NaN and an infinity in batches that have room; float64 view of what the kernel reads"""
    n = int(np.prod(shape))
    z = torch.from_numpy(np.random.RandomState(n + B).standard_normal((B, n)) * 1.2).to(dtype)
    if B >= 3 and n > 8:
        z[1, 5] = float("nan")
        z[2, 3] = float("inf")
    return z, z.to(F64).numpy()


def restated_extract(z64, key, nonce, M, l, N):
    B, n = z64.shape
    y = quantise(z64, l)[0]
    ks = np.unpackbits(np.frombuffer(O.chacha20_keystream(key, nonce, n * l // 8), np.uint8))
    plain = window_bits(y, l) ^ ks[None]
    copies = n * l // M
    counts = plain.reshape(B, copies, M).sum(1).astype(np.int32)
    bits = np.packbits((2 * counts > copies).astype(np.uint8), axis=1)
    return bits, counts, flags_of(z64, l, N)


def message_lengths(nb):
    return sorted({8, 256, 1024, nb})


def run_extracts(codec, l, dtype, cases):
    out = {}
    for shape, B in cases:
        key, nonce = KEYS[KEY_OF_BATCH[B]]
        z = latent_case(shape, B, dtype)[0].cuda()
        for M in message_lengths(z.shape[1] * l):
            if (z.shape[1] * l) % M == 0:
                out[(shape, B, M)] = codec.extract_batch(z, key, nonce, M, return_counts=True, l=l)
    return out


def check_extract(res, shape, B, M, l, dtype, N):
    key, nonce = KEYS[KEY_OF_BATCH[B]]
    bits, counts, flags = restated_extract(latent_case(shape, B, dtype)[1], key, nonce, M, l, N)
    assert res[2].dtype == torch.int32 and np.array_equal(res[2].cpu().numpy(), counts), (shape, B, M)
    assert np.array_equal(res[0].cpu().numpy(), bits), (shape, B, M)
    assert res[1].cpu().numpy().tolist() == flags.tolist(), (shape, B, M)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("l", WINDOWS)
def test_extract_parity(G, l, dtype):
    cases = [(s, B) for s in LATTICES for B in BATCHES]
    got = run_extracts(G.codec, l, dtype, cases)
    seen = set()
    for (shape, B, M), res in got.items():
        check_extract(res, shape, B, M, l, dtype, G.N)
        seen.add(M)
    assert {8, 256, 1024, 16384 * l} <= seen
    # a ragged message length: the reference's IndexError
    for shape, B in cases:
        key, nonce = KEYS[KEY_OF_BATCH[B]]
        z = latent_case(shape, B, dtype)[0].cuda()
        for M in message_lengths(z.shape[1] * l) + [7, z.shape[1] * l + 8]:
            if (z.shape[1] * l) % M:
                with pytest.raises(IndexError, match="string index out of range"):
                    G.codec.extract_batch(z, key, nonce, M, l=l)
    # without counts the bits and flags are the same
    (shape, B, M), res = next(iter(got.items()))
    key, nonce = KEYS[KEY_OF_BATCH[B]]
    b2, f2 = G.codec.extract_batch(latent_case(shape, B, dtype)[0].cuda(), key, nonce, M, l=l)
    assert torch.equal(b2, res[0]) and torch.equal(f2, res[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("l", WINDOWS)
def test_ties_resolve_to_zero(G, l, dtype):
    """two copies that disagree in every bit: every count is 1 of 2, every voted bit 0"""
    key, nonce = KEYS["carry"]
    n = 1700
    M = n * l // 2
    rs = np.random.RandomState(l)
    p = rs.randint(0, 2, M).astype(np.uint8)
    ks = np.unpackbits(np.frombuffer(O.chacha20_keystream(key, nonce, n * l // 8), np.uint8))
    y = windows(np.concatenate([p, 1 - p]) ^ ks, l)
    z = torch.from_numpy(ndtri((y + 0.5) / 2.0 ** l)[None]).to(dtype)       # the middle of each bin
    assert np.array_equal(quantise(z.to(F64).numpy(), l)[0][0], y)
    bits, flags, counts = G.codec.extract_batch(z.cuda(), key, nonce, M, return_counts=True, l=l)
    assert int(flags.abs().sum()) == 0
    assert bool((counts == 1).all()) and int(bits.sum()) == 0
    # and a strict majority of three against one copy turned round
    M3 = n * l // 4
    p3 = rs.randint(0, 2, M3).astype(np.uint8)
    y3 = windows(np.concatenate([p3, p3, 1 - p3, p3]) ^ ks, l)
    z3 = torch.from_numpy(ndtri((y3 + 0.5) / 2.0 ** l)[None]).to(dtype)
    bits3, _, counts3 = G.codec.extract_batch(z3.cuda(), key, nonce, M3, return_counts=True, l=l)
    assert np.array_equal(counts3.cpu().numpy()[0], np.where(p3 == 1, 3, 1))
    assert np.array_equal(bits3.cpu().numpy()[0], np.packbits(p3))


# ---------------------------------------------------------------------------------------------------------------- 5. round trip
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("l", WINDOWS)
def test_noiseless_round_trip(G, l, dtype):
    codec = G.codec
    key, nonce = KEYS["carry"]
    for shape, mb, B in (((4, 64, 64), 32, 3), ((4, 64, 64), 64 * l, 2), ((4, 3, 3), 3, 5)):
        n = int(np.prod(shape))
        k = bytes(np.random.RandomState(mb + l).randint(0, 256, mb, dtype=np.uint8))
        copies = codec.vote_copies(n, 8 * mb, l)
        for fast in (False, True):
            z = codec.embed_batch(key, nonce, k, B, shape, seed=11 + l, image_index0=3, dtype=dtype, fast=fast, l=l)
            bits, flags, counts = codec.extract_batch(z, key, nonce, 8 * mb, return_counts=True, l=l)
            assert int(flags.abs().sum()) == 0
            want = np.unpackbits(np.frombuffer(k, np.uint8)).astype(np.int32) * copies
            assert np.array_equal(counts.cpu().numpy(), np.broadcast_to(want, (B, 8 * mb))), (shape, mb, fast)
            assert all(bits[b].cpu().numpy().tobytes() == k for b in range(B))
            assert int(codec.bit_matches(bits, 8 * mb, k).min()) == 8 * mb
    assert codec.vote_copies(16384, 256, l) == 64 * l and codec.vote_copies(16384, 512 * l, l) == 32


# ---------------------------------------------------------------------------------------------------------------- 6. trace
def test_trace_topk_on_two_bit_counts(G):
    codec, trace = G.codec, G.trace
    key, nonce = KEYS["readme"]
    l, shape, n, M = 2, (4, 64, 64), 16384, 256
    rs = np.random.RandomState(5)
    reg = rs.randint(0, 256, (200, M // 8), dtype=np.uint8)
    planted = [17, 0, 199]
    z = torch.cat([codec.embed_batch(key, nonce, bytes(reg[u]), 1, shape, seed=u, dtype=F16, l=l) for u in planted])
    strangers = torch.from_numpy(rs.standard_normal((4, n))).half().cuda().view(4, *shape)
    zz = torch.cat([z, strangers])
    copies = codec.vote_copies(n, M, l)
    assert copies == 128
    _, flags, counts = codec.extract_batch(zz, key, nonce, M, return_counts=True, l=l)
    assert int(flags.abs().sum()) == 0
    for soft in (True, False):
        idx, score = codec.trace_topk(counts, copies, torch.from_numpy(reg).cuda(), k=3, soft=soft)
        hi, hs = trace.topk_host(counts.cpu().numpy(), copies, reg, 3, soft=soft)
        assert np.array_equal(idx.cpu().numpy(), hi) and np.array_equal(score.cpu().numpy(), hs)
        assert idx[:3, 0].cpu().tolist() == planted
        assert score[:3, 0].cpu().tolist() == [n * l if soft else M] * 3          # every one of the Nb votes agrees
    # the front end: Registry + trace_latents with l
    r = trace.Registry(M // 8)
    for u in range(reg.shape[0]):
        r.add(f"user{u}", bytes(reg[u]))
    res = trace.trace_latents(zz, key, nonce, r, k=2, l=l)
    assert [x.attributed for x in res] == ["user17", "user0", "user199", None, None, None, None]
    assert res[0].candidates[0].score == n * l and res[0].candidates[0].agree == M


def test_quant_pack_feeds_the_keyed_search(G):
    codec, trace = G.codec, G.trace
    shape, n, mb = (4, 17, 25), 1700, 25                                    # 3400 l bits = 17 l copies of 200 bits
    rs = np.random.RandomState(9)
    U = 33
    recs = [(bytes(rs.randint(0, 256, 32, dtype=np.uint8)) if u % 3 else KEYS["carry"][0],
             bytes(rs.randint(0, 256, 16, dtype=np.uint8)) if u % 5 else KEYS["carry2"][1],
             bytes(rs.randint(0, 256, mb, dtype=np.uint8))) for u in range(U)]
    stride = codec.keyed_record_stride(mb)
    rows = np.zeros((U, stride), np.uint8)
    for u, (key, nonce, msg) in enumerate(recs):
        rows[u, :48 + mb] = np.frombuffer(key + nonce + msg, np.uint8)
    for l in WINDOWS:
        code = np.stack([np.packbits(cipher_bits(key, nonce, msg, n, l)) for key, nonce, msg in recs])
        planted = [32, 3, 15]
        z = torch.cat([codec.embed_batch(*recs[u], 1, shape, seed=u, dtype=BF16, l=l) for u in planted] +
                      [torch.from_numpy(rs.standard_normal((2, n))).to(BF16).cuda().view(2, *shape)])
        packed, flags = codec.quant_pack(z, l)
        assert int(flags.abs().sum()) == 0
        assert np.array_equal(packed[:3].cpu().numpy(), code[planted])          # a noiseless image IS its record's codeword
        idx, score = codec.trace_keyed_topk(packed, n * l, torch.from_numpy(rows).cuda(), mb, k=4)
        hi, hs = trace.keyed_topk_host(packed.cpu().numpy(), code, 4)
        assert np.array_equal(idx.cpu().numpy(), hi) and np.array_equal(score.cpu().numpy(), hs)
        assert idx[:3, 0].cpu().tolist() == planted and score[:3, 0].cpu().tolist() == [n * l] * 3
        # the front end
        kr = trace.KeyedRegistry(mb)
        for u, (key, nonce, msg) in enumerate(recs):
            kr.add(f"user{u}", key, nonce, msg)
        res = trace.trace_latents_keyed(z, kr, k=1, l=l)
        assert [x.attributed for x in res] == ["user32", "user3", "user15", None, None]
        assert res[0].candidates[0].agree == 8 * mb and res[0].candidates[0].score == n * l


# ---------------------------------------------------------------------------------------------------------------- 7. pipeline
@pytest.mark.usefixtures("library_kernels_allowed")
def test_pipeline_votes_with_its_window(G):
    """synthetic weights, a 32 x 32 lattice, 2 steps: the pipeline's extract is the plain inversion followed by the l-bit extract, and its
    embed is the l-bit embed.  (What survives a real model at l > 1 has not been measured; nothing is asserted on accuracy.)"""
    key, nonce = KEYS["readme"]
    k = O.pad_message("lthero", 32)
    m = G.unet.synthetic_init_(G.unet.UNet2DCondition(block_out_channels=(64, 128, 128, 128), cross_attention_dim=64, num_heads=(1, 2, 2, 2), head_dim=64), 0)
    m = m.cuda().half().eval()
    g = torch.Generator().manual_seed(3)
    cu = torch.randn(1, 77, 64, generator=g).cuda().half()
    pipe = G.pipeline.GaussianShadingPipeline(m, key, nonce, k, height=256, width=256, num_inference_steps=2, ctx_uncond=cu, l=2)
    assert pipe.l == 2
    x0 = torch.randn(2, 4, 32, 32, generator=g).cuda().half()
    with torch.no_grad():
        bits, flags, z = pipe.invert_and_extract(x0, return_latents=True)
        zi = pipe.invert(x0)
        b0, f0 = pipe.invert_and_extract(x0)
    assert torch.equal(z, zi)
    b2, f2 = G.codec.extract_batch(zi, key, nonce, 256, l=2)
    assert torch.equal(bits, b2) and torch.equal(flags, f2) and torch.equal(b0, b2) and torch.equal(f0, f2)
    b1, _ = G.codec.extract_batch(zi, key, nonce, 256)
    assert not torch.equal(b1, b2)                                           # (the one-bit vote reads other bits out of the same latent)
    zT = pipe.embed(2, seed=4, image_index0=1)
    assert torch.equal(zT, G.codec.embed_batch(key, nonce, k, 2, (4, 32, 32), seed=4, image_index0=1, dtype=F16, fast=True, l=2))
    assert int(G.codec.bit_matches(G.codec.extract_batch(zT, key, nonce, 256, l=2)[0], 256, k).min()) == 256


# ---------------------------------------------------------------------------------------------------------------- 8. poisoned buffers
POISON_CASES = [((4, 3, 3), 3), ((4, 17, 25), 3), ((4, 64, 64), 1)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("l", WINDOWS)
def test_embed_and_extract_on_poisoned_buffers(G, l, dtype):
    """tests 1 and 4 once more on guard-banded, pattern-filled buffers: every output element is written, nothing outside is, and no result depends
    on what lies around the operands"""
    from test_gpu_poisoned import Out, three_ways
    codec = G.codec
    inp = {}
    for j, (shape, B) in enumerate(POISON_CASES):
        inp[f"u{j}"] = torch.from_numpy(embed_case(shape, B, l)[3]).cuda()
        inp[f"z{j}"] = latent_case(shape, B, dtype)[0].cuda()

    def case(i, L):
        o = Out()
        for j, (shape, B) in enumerate(POISON_CASES):
            key, nonce, k = embed_case(shape, B, l)[:3]
            o.written[f"embed{j}"] = codec.embed_batch(key, nonce, k, B, shape, u=i[f"u{j}"], dtype=dtype, l=l)
            o.written[f"philox{j}"] = codec.embed_batch(key, nonce, k, B, shape, seed=j, dtype=dtype, fast=True, l=l)
            kk, nn = KEYS[KEY_OF_BATCH[B]]
            for M in message_lengths(i[f"z{j}"].shape[1] * l):
                if (i[f"z{j}"].shape[1] * l) % M == 0:
                    bits, flags, counts = codec.extract_batch(i[f"z{j}"], kk, nn, M, return_counts=True, l=l)
                    o.written.update({f"bits{j}.{M}": bits, f"flags{j}.{M}": flags, f"counts{j}.{M}": counts})
            packed, pf = codec.quant_pack(i[f"z{j}"], l)
            o.written.update({f"packed{j}": packed, f"pflags{j}": pf})
        return o

    c = three_ways(G, case, inp)
    for j, (shape, B) in enumerate(POISON_CASES):
        check_embed(c.written[f"embed{j}"], shape, B, l, dtype)
        z64 = latent_case(shape, B, dtype)[1]
        for M in message_lengths(z64.shape[1] * l):
            if (z64.shape[1] * l) % M == 0:
                check_extract((c.written[f"bits{j}.{M}"], c.written[f"flags{j}.{M}"], c.written[f"counts{j}.{M}"]), shape, B, M, l, dtype, G.N)
        assert np.array_equal(c.written[f"packed{j}"].cpu().numpy(), np.packbits(window_bits(quantise(z64, l)[0], l), axis=1))
        assert c.written[f"pflags{j}"].cpu().numpy().tolist() == flags_of(z64, l, G.N).tolist()
