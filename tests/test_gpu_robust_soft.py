"""GPU: the robust decode in one launch, tile weights times reliability levels (`codec.decode_robust` / gsw_decode_robust) against the
NumPy restatement of tests/robust_soft_reference.py -- all six outputs bit for bit -- then the identities with the shipped decoders (`tamper.extract_robust`,
`codec.extract_soft[_l]`, the plain vote), determinism, poisoned and guard-banded buffers, every refusal, `tamper.extract_robust_soft` end to end on the damaged
latents of tests/test_robust_soft_host.py, and the front ends.  EXACT equality everywhere, no tolerance."""
import types

import numpy as np
import pytest
import torch

from conftest import README_KEY, README_NONCE

import gs_oracle as O
import robust_soft_reference as R
import tamper_reference as TR
from poison import FINITE, NAN, Ledger, poisoned

pytestmark = pytest.mark.gpu

KEY, NONCE = bytes.fromhex(README_KEY), bytes.fromhex(README_NONCE)
OUTS = ("bits", "score", "wsum", "excess", "wsq", "weights")


@pytest.fixture(scope="module")
def G():
    import gswm_amd
    from gswm_amd import codec, soft, tamper
    return codec, soft, tamper


def _operands(seed, B, shape, l, tile, M, P, kind):
    """rows and planes built as bits.  kind "random": uniformly random rows (no watermark: most weights fall to 0); "planted": the codeword of the image's
    message with each bit flipped with probability 0.25 and some tiles overwritten with random bits.  The levels are uniform over 0 .. 2^P - 1.  A key,
    nonce and message per image; image 1 (image 0 when B == 1) starts at block counter 0xFFFFFFFF so that the 32-bit counter carries inside the row."""
    rng = np.random.default_rng(seed)
    C, h, w = shape
    nb = C * h * w * l
    tau = R.tile_index(shape, l, tile)
    n_tiles = (h // tile) * (w // tile)
    packed, planes, recs, levs = [], [], [], []
    for b in range(B):
        key, nonce = bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8))
        if b == min(1, B - 1):
            nonce = b"\xff\xff\xff\xff" + nonce[4:]
        msg = bytes(rng.integers(0, 256, M // 8, dtype=np.uint8))
        q = rng.integers(0, 2, nb, dtype=np.uint8)
        if kind == "planted":
            lost = rng.random(n_tiles) < 0.3                                   # these tiles keep their random bits
            cw = np.asarray(O.cipher_bits(msg, key, nonce, nb)).astype(np.uint8) ^ (rng.random(nb) < 0.25).astype(np.uint8)
            q = np.where(lost[tau], q, cw).astype(np.uint8)
        lev = rng.integers(0, 1 << P, nb) if P else None
        if P and nb >= 64 << P:
            assert set(np.unique(lev)) == set(range(1 << P))                   # all levels 0 .. 2^P - 1 occur
        recs.append((key, nonce, msg))
        packed.append(np.packbits(q))
        levs.append(lev)
        if P:
            planes.append(R.planes_from_levels(lev, P))
    return np.stack(packed), (np.stack(planes) if P else None), recs, levs


def _dev(tamper, packed, planes, recs):
    keys = tamper.keys_tensor([(k, n) for k, n, _ in recs], "cuda")
    return torch.from_numpy(packed).cuda(), (torch.from_numpy(planes).cuda() if planes is not None else None), keys


def _same(got, want, b, what=""):
    """the six outputs of image b of a `RobustVote` against the restatement's dict"""
    for name in OUTS:
        g = getattr(got, name)[b].cpu().numpy()
        w = np.packbits(want["bits"]) if name == "bits" else want[name]
        assert g.shape == w.shape and np.array_equal(g.astype(np.int64), w.astype(np.int64)), (name, b, what)


# shape, tile, M (None: M = Nb, one copy) and per case the (l, P, iters, sign_rounds, kind) it runs with: every value of every axis occurs
CASES = [
    ((4, 8, 8), 8, 32, [(1, 4, 2, 0, "planted"), (2, 0, 1, 0, "random"), (4, 2, 3, 1, "planted")]),                  # one tile
    ((3, 8, 8), 8, 24, [(1, 1, 2, 1, "planted"), (2, 4, 0, 0, "random"), (4, 2, 1, 0, "planted")]),                  # 24-byte row, partial block, 3 message bytes
    ((4, 16, 24), 8, 64, [(1, 2, 3, 0, "planted"), (2, 4, 2, 1, "random"), (4, 0, 2, 0, "planted")]),                # not square
    ((1, 32, 32), 32, 128, [(1, 4, 1, 1, "planted"), (2, 1, 2, 0, "planted"), (4, 4, 0, 1, "random")]),
    ((4, 32, 32), 8, 8, [(1, 4, 2, 0, "planted"), (4, 4, 2, 0, "planted")]),                                         # eight lanes per message bit
    ((4, 32, 32), 16, 8, [(2, 2, 3, 1, "random"), (4, 4, 1, 1, "planted")]),                                         # (l = 4: 2048 x 225 x 4096, next to the int32 bound)
    ((4, 32, 32), 8, None, [(1, 2, 2, 0, "planted"), (2, 4, 1, 1, "random")]),                                       # one copy
    ((4, 32, 32), 16, None, [(1, 0, 2, 0, "random"), (4, 1, 3, 0, "planted")]),
    ((4, 64, 64), 8, 256, [(1, 4, 2, 0, "planted"), (1, 4, 2, 1, "random"), (1, 0, 2, 0, "planted"), (2, 2, 3, 0, "planted"), (4, 1, 0, 0, "planted")]),
    ((4, 96, 96), 32, 1024, [(1, 4, 2, 1, "planted"), (2, 2, 1, 0, "random"), (4, 4, 3, 0, "planted")]),             # blocks straddle rows and tiles
]
GRID = [(shape, tile, M, *combo) for shape, tile, M, combos in CASES for combo in combos]


def test_the_grid_covers_every_axis():
    for axis, want in ((3, {1, 2, 4}), (4, {0, 1, 2, 4}), (5, {0, 1, 2, 3}), (6, {0, 1}), (7, {"random", "planted"})):
        assert {g[axis] for g in GRID} == want


@pytest.mark.parametrize("shape,tile,M,l,P,iters,W,kind", GRID)
def test_all_six_outputs_match_the_restatement(G, shape, tile, M, l, P, iters, W, kind):
    codec, soft, tamper = G
    B = 3
    M = int(np.prod(shape)) * l if M is None else M
    packed, planes, recs, levs = _operands(7 * tile + 31 * l + 101 * P + 3 * iters + W + shape[1], B, shape, l, tile, M, P, kind)
    want = [R.decode(np.unpackbits(packed[b]), recs[b][0], recs[b][1], levs[b], M, shape, l, tile, iters, W) for b in range(B)]
    th, tw = shape[1] // tile, shape[2] // tile
    for Bn in (3, 1):                      # B == 1: image 0 alone (the image whose counter carries is image 1; alone, in the test below)
        s, p, k = _dev(tamper, packed[:Bn], planes[:Bn] if P else None, recs[:Bn])
        got = codec.decode_robust(s, p, k, M, shape, l, tile, iters, W)
        assert got.bits.dtype == torch.uint8 and got.bits.shape == (Bn, M // 8)
        assert all(getattr(got, n).dtype == torch.int32 for n in OUTS[1:]) and got.score.shape == got.wsum.shape == (Bn, M)
        assert got.excess.shape == got.wsq.shape == got.weights.shape == (Bn, th, tw)
        for b in range(Bn):
            _same(got, want[b], b, (Bn, kind))
    if iters == 0:
        assert bool((got.weights == 1).all())


def test_single_image_under_a_carrying_counter(G):
    codec, soft, tamper = G
    shape, l, tile, M, P = (4, 16, 24), 2, 8, 64, 4
    packed, planes, recs, levs = _operands(5, 1, shape, l, tile, M, P, "planted")
    assert recs[0][1][:4] == b"\xff\xff\xff\xff"
    got = codec.decode_robust(*_dev(tamper, packed, planes, recs), M, shape, l, tile, 2, 0)
    _same(got, R.decode(np.unpackbits(packed[0]), recs[0][0], recs[0][1], levs[0], M, shape, l, tile, 2, 0), 0)


@pytest.mark.parametrize("P,W", [(0, 0), (2, 1), (4, 0)])
def test_a_round_without_any_weight_decodes_zeros(G, P, W):
    """p_j = parity of the copy j // M at 4 x 64 x 64, M = 256: every message bit ties (bits 0), every 8 x 8 tile holds as many ones as zeros, so with equal
    levels every excess is 0, every weight falls to 0 and the rounds after the first vote with no weight at all"""
    codec, soft, tamper = G
    shape, l, tile, M = (4, 64, 64), 1, 8, 256
    nb = 16384
    p = ((np.arange(nb) // M) & 1).astype(np.uint8)
    ks = np.asarray(O.keystream_bits(KEY, NONCE, nb)).astype(np.uint8)
    packed = np.packbits(p ^ ks)[None]
    lev = np.full(nb, (1 << P) - 1) if P else None
    planes = R.planes_from_levels(lev, P)[None] if P else None
    want = R.decode_p(p, lev, M, shape, l, tile, 2, W)
    assert not want["weights"].any() and not want["score"].any() and not want["wsum"].any() and not want["bits"].any() and not want["excess"].any()
    got = codec.decode_robust(*_dev(tamper, packed, planes, [(KEY, NONCE, b"")]), M, shape, l, tile, 2, W)
    _same(got, want, 0)


# ===================================================================================================================== identities against the shipped kernels
def _real_latents(codec, l, dtype, B=3, seed=3):
    msg = codec.pad_message("lthero", 32)
    z = codec.embed_batch(KEY, NONCE, msg, B, (4, 64, 64), seed=seed, l=l)
    g = torch.Generator().manual_seed(10 + l)
    z = z + 1.1 * torch.randn(z.shape, generator=g).cuda()
    z[:, :, :24, :] = torch.randn((B, 4, 24, 64), generator=g).cuda()            # the top rows pasted over
    return msg, z.to(dtype).contiguous()


@pytest.mark.parametrize("l", [1, 2, 4])
def test_without_planes_it_is_extract_robust(G, l):
    codec, soft, tamper = G
    shape, M, tile = (4, 64, 64), 256, 8
    msg, z = _real_latents(codec, l, torch.float32)
    n_t = 4 * tile * tile * l
    for iters in (0, 2):
        bits, flags, score, wsum, agree = tamper.extract_robust(z, KEY, NONCE, M, l=l, tile=tile, iters=iters)
        packed, _ = codec.quant_pack(z, l)
        for W in (0, 1):
            got = codec.decode_robust(packed, None, tamper.keys_tensor([(KEY, NONCE)] * 3, "cuda"), M, shape, l, tile, iters, W)
            assert torch.equal(got.bits, bits) and torch.equal(got.score, score) and torch.equal(got.wsum, wsum)
            assert torch.equal(got.excess + n_t, 2 * agree) and bool((got.wsq == n_t).all())
        two = tamper.extract_robust_soft(z, KEY, NONCE, M, l=l, tile=tile, iters=iters, levels=0)          # the two-launch form of extract_robust
        assert torch.equal(two.bits, bits) and torch.equal(two.score, score) and torch.equal(two.wsum, wsum) and torch.equal(two.flags, flags)
        assert torch.equal(two.weights, got.weights) and torch.equal(tamper.soft_weights(two.excess, two.wsq), tamper.default_weights(agree, n_t).view(torch.int16).to(torch.int32))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("l", [1, 2, 4])
def test_without_iterations_it_is_the_soft_vote_or_the_plain_vote(G, l, dtype):
    codec, soft, tamper = G
    shape, M, tile, B = (4, 64, 64), 256, 8, 3
    msg, z = _real_latents(codec, l, dtype)
    table = soft._default_table(z, l, 15)
    records = soft.shared_records(KEY, NONCE, M // 8, B, "cuda")
    want = codec.extract_soft(z, records, M // 8, table) if l == 1 else codec.extract_soft_l(z, records, M // 8, table, l)
    rows = codec.level_pack(z, table) if l == 1 else codec.level_pack_l(z, table, l)
    keys = tamper.keys_tensor([(KEY, NONCE)] * B, "cuda")
    got = codec.decode_robust(rows.signs, rows.planes, keys, M, shape, l, tile, 0, 0)
    assert torch.equal(got.bits, want.bits) and torch.equal(got.score, want.score) and torch.equal(got.wsum, want.wsum)
    assert torch.equal(got.wsq.sum(dim=(1, 2)).to(torch.int32), want.wsq) and bool((got.weights == 1).all())
    plain = codec.decode_robust(rows.signs, rows.planes, keys, M, shape, l, tile, 0, 1)                    # the only round at unit levels
    bits0, _, counts = codec.extract_batch(z, KEY, NONCE, M, return_counts=True, l=l)
    copies = codec.vote_copies(4 * 64 * 64, M, l)
    assert torch.equal(plain.bits, bits0) and torch.equal(plain.score, 2 * counts.to(torch.int32) - copies) and bool((plain.wsum == copies).all())
    assert bool((plain.wsq == 4 * tile * tile * l).all())


# ===================================================================================================================== determinism, poisoned buffers
def test_two_runs_give_identical_bytes(G):
    codec, soft, tamper = G
    shape, l, tile, M, P = (4, 64, 64), 2, 8, 256, 4
    packed, planes, recs, _ = _operands(3, 3, shape, l, tile, M, P, "planted")
    ops = _dev(tamper, packed, planes, recs)
    a = codec.decode_robust(*ops, M, shape, l, tile, 3, 1)
    b = codec.decode_robust(*ops, M, shape, l, tile, 3, 1)
    for name in OUTS:
        assert getattr(a, name).cpu().numpy().tobytes() == getattr(b, name).cpu().numpy().tobytes(), name


@pytest.mark.parametrize("shape,l,tile,M,P", [((4, 16, 24), 1, 8, 64, 4), ((4, 64, 64), 2, 16, 256, 2), ((4, 64, 64), 1, 8, 256, 0)])
def test_poisoned_guard_banded_buffers(G, shape, l, tile, M, P):
    """every operand inside banded buffers and every output served pattern-filled, under both patterns: the bands stay intact, no output element of more than
    a byte keeps the pattern, and the bits of every output are those of the clean run"""
    codec, soft, tamper = G
    packed, planes, recs, _ = _operands(21, 3, shape, l, tile, M, P, "planted")
    s, p, k = _dev(tamper, packed, planes, recs)

    def run(s_, p_, k_):
        return codec.decode_robust(s_, p_, k_, M, shape, l, tile, 2, 1)

    clean = run(s, p, k)
    torch.cuda.synchronize()
    for pattern in (NAN, FINITE):
        L = Ledger(pattern)
        try:
            with poisoned(L):
                outs = run(L.wrap(s), L.wrap(p) if p is not None else None, L.wrap(k))
            torch.cuda.synchronize()
            L.check()
            for name, o, c in zip(OUTS, outs, clean):
                if o.element_size() > 1:
                    assert L.untouched(o) == 0, f"{name}: {L.where(o)}"
                assert torch.equal(o, c), name
        finally:
            L.release()


# ===================================================================================================================== refusals
def test_every_refusal(G):
    codec, soft, tamper = G
    shape, l, tile, M, B, P = (4, 16, 16), 1, 8, 64, 2, 2
    packed, planes, recs, _ = _operands(2, B, shape, l, tile, M, P, "random")
    s, p, k = _dev(tamper, packed, planes, recs)

    def f(**kw):
        return codec.decode_robust(kw.get("s", s), kw.get("p", p), kw.get("k", k), kw.get("M", M), kw.get("shape", shape), kw.get("l", l), kw.get("tile", tile),
                                   kw.get("iters", 2), kw.get("W", 0))

    f()
    launches = []
    lib = codec.N.lib()
    real = lib.gsw_decode_robust

    class Spy:                                                                   # none of the refusals below reaches the library
        def __getattr__(self, name):
            if name == "gsw_decode_robust":
                launches.append(name)
            return getattr(lib, name)

    orig = codec.N.lib
    codec.N.lib = lambda: Spy()
    try:
        for bad_tile in (4, 12, 64, True):
            with pytest.raises(ValueError, match="tile must be one of"):
                f(tile=bad_tile)
        with pytest.raises(ValueError, match="whole number"):
            f(tile=32)
        for bad_l in (0, 3, 8):
            with pytest.raises(ValueError, match="l must be one of"):
                f(l=bad_l)
        with pytest.raises(ValueError, match="multiple of 8"):
            f(M=60)
        with pytest.raises(ValueError, match="packed rows hold"):
            f(shape=(4, 16, 24))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(s=s.cpu())
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(p=p.cpu())
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(k=k.cpu())
        with pytest.raises(ValueError, match="keys must be uint8"):
            f(k=k[:, :32].contiguous())
        with pytest.raises(ValueError, match="packed must be uint8"):
            f(s=s.view(torch.int8))
        for bad_p in (p.view(torch.int8), p[:1].contiguous(), p[:, :, :64].contiguous(), torch.zeros((B, 5, 128), dtype=torch.uint8).cuda(), p[:, 0].contiguous()):
            with pytest.raises(ValueError, match="planes must be uint8"):
                f(p=bad_p)
        for bad in (-1, 9, 2.0, True):
            with pytest.raises(ValueError, match="iters must be an int in 0..8"):
                f(iters=bad)
        for bad in (-1, 2, 1.0, False):
            with pytest.raises(ValueError, match="sign_rounds must be an int in 0..1"):
                f(W=bad)
        with pytest.raises(IndexError, match="string index out of range"):
            f(M=384)
        # n_bits (1 + P) > 1 048 576: 262 144 bits with four planes
        big = torch.zeros((1, 32768), dtype=torch.uint8).cuda()
        with pytest.raises(ValueError, match=r"n_bits \(1 \+ P\) <= 1048576"):
            codec.decode_robust(big, torch.zeros((1, 4, 32768), dtype=torch.uint8).cuda(), k[:1].contiguous(), 256, (16, 128, 128), 1, 8)
        # the int32 bound, a lattice and message the plan sweep accepts one tile size below: 2048 copies x 15^2 x 16384 bits of the one 32 x 32 tile
        s4, p4 = torch.zeros((1, 2048), dtype=torch.uint8).cuda(), torch.zeros((1, 4, 2048), dtype=torch.uint8).cuda()
        with pytest.raises(ValueError, match=r"copies Lmax\^2 n_t = 2048 x 15\^2 x 16384 = 7549747200 does not fit int32"):
            codec.decode_robust(s4, p4, k[:1].contiguous(), 8, (4, 32, 32), 4, 32)
        # the LDS cap: 128 KiB of row and 64 KiB of tile weights
        s1 = torch.zeros((1, 131072), dtype=torch.uint8).cuda()
        with pytest.raises(ValueError, match="196640 bytes of LDS"):
            codec.decode_robust(s1, None, k[:1].contiguous(), 256, (1, 1024, 1024), 1, 8)
    finally:
        codec.N.lib = orig
    assert not launches
    assert codec.decode_robust(s4, p4, k[:1].contiguous(), 8, (4, 32, 32), 4, 16).score.shape == (1, 8)          # 2048 x 225 x 4096 fits

    # the C ABI's own status codes (include/gswm.h), called directly
    N = codec.N
    o = codec.decode_robust(s, p, k, M, shape, l, tile)
    ptr = {n: getattr(o, n).data_ptr() for n in OUTS}

    def rc(S=s.data_ptr(), Pl=p.data_ptr(), P_=P, B_=B, C=4, h=16, w_=16, l_=1, t=8, K=k.data_ptr(), M_=M, I=2, W=0, **out):
        a = dict(ptr, **out)
        return real(S, Pl, P_, B_, C, h, w_, l_, t, K, M_, I, W, a["bits"], a["score"], a["wsum"], a["excess"], a["wsq"], a["weights"], None)

    assert rc() == N.GSW_OK and rc(Pl=None, P_=0) == N.GSW_OK
    assert rc(S=None) == rc(K=None) == rc(Pl=None) == rc(B_=0) == rc(l_=3) == rc(l_=0) == rc(P_=-1) == rc(P_=5) == rc(I=-1) == rc(I=9) == rc(W=2) == rc(W=-1) == N.GSW_ERR_BAD_ARG
    assert rc(S=s.data_ptr() + 1) == rc(Pl=p.data_ptr() + 2) == rc(K=k.data_ptr() + 1) == N.GSW_ERR_BAD_ARG
    for name in OUTS:
        assert rc(**{name: None}) == N.GSW_ERR_BAD_ARG
    assert rc(t=4) == rc(t=64) == rc(h=12) == rc(w_=20) == rc(M_=60) == N.GSW_ERR_UNSUPPORTED
    assert rc(C=4, h=512, w_=520, P_=0) == N.GSW_ERR_UNSUPPORTED               # 1 064 960 bits > 1 048 576
    assert rc(C=16, h=128, w_=128, M_=256, P_=4) == N.GSW_ERR_UNSUPPORTED      # 262 144 bits x 5
    assert rc(C=4, h=32, w_=32, l_=4, t=32, M_=8, P_=4) == N.GSW_ERR_UNSUPPORTED      # the int32 bound
    assert rc(C=1, h=1024, w_=1024, M_=256, P_=0) == N.GSW_ERR_UNSUPPORTED     # the LDS cap
    assert rc(M_=384) == N.GSW_ERR_RAGGED
    torch.cuda.synchronize()


# ===================================================================================================================== end to end
SETS = {"quiet": (1.5, 56, 1.0), "loud": (1.0, 48, 3.0)}       # sigma, rows replaced, scale of the replaced rows: the two sets of tests/test_robust_soft_host.py
MSG = bytes(np.random.default_rng(5).integers(0, 256, 32, dtype=np.uint8))
MSG_BITS = np.unpackbits(np.frombuffer(MSG, dtype=np.uint8))


def _right(bits):
    return int((np.asarray(bits).reshape(-1, 256) == MSG_BITS[None]).sum())


@pytest.fixture(scope="module")
def damaged():
    """per set and seed: the fp16 latents on the device (20 images), their default table, what the restatement decodes under that table for both sign_rounds,
    and the bits the restated tile-weighted decode and soft vote get right on the same latents"""
    from gswm_amd import soft
    ks = np.asarray(O.keystream_bits(KEY, NONCE, 16384)).astype(np.uint8)
    out = {}
    for name, (sigma, rows, loud) in SETS.items():
        for seed in (0, 1, 2):
            z = TR.synthetic_latents(MSG, KEY, NONCE, (4, 64, 64), sigma, seed, 20, rows).astype(np.float32)
            z[:, :, :rows, :] *= np.float32(loud)
            zd = torch.from_numpy(z).cuda().half().contiguous()
            table = soft.uniform_thresholds(zd, 15, 2.5)
            zh, th = zd.float().cpu().numpy(), table.cpu().numpy()
            p = [R.sign_bits(zh[i]) ^ ks for i in range(20)]
            lev = [R.levels_of(zh[i], th[i]) for i in range(20)]
            want = {W: [R.decode_p(p[i], lev[i], 256, (4, 64, 64), 1, 8, 2, W) for i in range(20)] for W in (0, 1)}
            base = {"robust": _right([R.decode_p(p[i], None, 256, (4, 64, 64), 1, 8, 2, 0)["bits"] for i in range(20)]),
                    "soft": _right([R.decode_p(p[i], lev[i], 256, (4, 64, 64), 1, 8, 0, 0)["bits"] for i in range(20)])}
            out[name, seed] = (zd, table, want, base)
    return out


def test_extract_robust_soft_end_to_end_equals_the_restatement_and_meets_its_margins(G, damaged):
    """uploaded as fp16, with its default table: all outputs equal the restatement fed the same table, on both damaged sets of tests/test_robust_soft_host.py and
    their three seeds, so the margins asserted there hold here as well (and are asserted again, on the device's bits)"""
    codec, soft, tamper = G
    right = {}
    for (name, seed), (zd, table, want, base) in damaged.items():
        for W in (0, 1):
            got = tamper.extract_robust_soft(zd, KEY, NONCE, 256, sign_rounds=W)              # its default table: soft.uniform_thresholds(zd, 15, 2.5)
            # (a paste at 3 x unit scale reaches 8.2924, where the reference's quantiser saturates: the packer's flag says so, the bits are decoded all the same)
            assert got.flags.cpu().tolist() == [int((zd[b].float() >= O.Y2_THRESHOLD).any()) for b in range(20)] and (name == "loud" or not int(got.flags.sum()))
            for b in range(20):
                _same(got, want[W][b], b, (name, seed, W))
            same = tamper.extract_robust_soft(zd, KEY, NONCE, 256, sign_rounds=W, thresholds=table)
            assert all(torch.equal(getattr(got, n), getattr(same, n)) for n in OUTS)
            right[name, seed, W] = _right(np.unpackbits(got.bits.cpu().numpy(), axis=1))
        print(name, seed, right[name, seed, 0], right[name, seed, 1], base)
        if name == "quiet":
            assert right[name, seed, 0] >= base["robust"] + 500 and right[name, seed, 0] >= base["soft"] + 500
    both1, both0 = (sum(right["loud", s, W] for s in (0, 1, 2)) for W in (1, 0))
    assert both1 >= sum(damaged["loud", s][3]["robust"] for s in (0, 1, 2)) and both1 >= both0 + 300
    zd = damaged["quiet", 0][0]
    assert torch.equal(tamper.extract_robust_soft(zd, KEY, NONCE, 256).bits, tamper.extract_robust_soft(zd, KEY, NONCE, 256, sign_rounds=1).bits)   # the default is the conservative mode


def test_the_front_ends_return_those_bits(G, damaged):
    from gswm_amd import extract as X, pipeline
    codec, soft, tamper = G
    zd = damaged["quiet", 0][0][:4].contiguous()
    want = {W: [codec.bits_to_str(r) for r in tamper.extract_robust_soft(zd, KEY, NONCE, 256, sign_rounds=W).bits.cpu().numpy()] for W in (0, 1)}
    args = types.SimpleNamespace(key=KEY, nonce=NONCE, message_length=256, l=1, robust_soft=15)
    assert X.recover_exactracted_message_batch(zd, args) == want[1] and X.recover_exactracted_message(zd[:1], args) == want[1][0]
    args.sign_rounds, args.tile, args.iters = 0, 8, 2
    assert X.recover_exactracted_message_batch(zd, args) == want[0] and X.recover_exactracted_message(zd[1:2].cpu().numpy(), args) == want[0][1]
    args = X.build_parser().parse_args(["--key_hex", README_KEY, "--nonce_hex", README_NONCE, "--original_message_hex", MSG.hex(), "--robust_soft", "15",
                                        "--message_length", "256"])
    args.key, args.nonce = KEY, NONCE
    assert X.recover_exactracted_message_batch(zd, args) == want[1]
    for extra, match in ((dict(soft=1), "--soft 1"), (dict(robust=1), "--robust 1"), (dict(window_soft=7, l=2), "--window_soft"), (dict(align="d4"), "--align")):
        bad = types.SimpleNamespace(**dict(dict(key=KEY, nonce=NONCE, message_length=256, l=1, robust_soft=15), **extra))
        with pytest.raises(ValueError, match="--robust_soft cannot be combined with " + match):
            X.recover_exactracted_message_batch(zd, bad)

    # the pipeline: an eps model of zeros makes the inversion a rescaling; every image under its own record's key (here the same one) and message
    rec = np.zeros((4, 80), dtype=np.uint8)
    rec[:, :48] = np.frombuffer(KEY + NONCE, dtype=np.uint8)
    rec[:, 48:80] = np.frombuffer(MSG, dtype=np.uint8)
    rec[3, 48] ^= 0x81                                                            # image 3 is checked against a message two bits away
    records = torch.from_numpy(rec).cuda()
    pipe = pipeline.GaussianShadingPipeline(lambda x, t, c: torch.zeros_like(x), KEY, NONCE, MSG, num_inference_steps=4, ctx_uncond=torch.zeros(1, 1, 1, device="cuda", dtype=torch.float16))
    res = pipe.verify_records(zd, records, 32, robust_levels=15, return_latents=True)
    zi = res[-1]
    for W in (1, 0):
        v = pipe.verify_records(zd, records, 32, robust_levels=15, sign_rounds=W)
        ref = tamper.extract_robust_soft(zi, KEY, NONCE, 256, sign_rounds=W)
        assert all(torch.equal(getattr(v, n), getattr(ref, n)) for n in OUTS) and torch.equal(v.flags, ref.flags)
        got_bits = np.unpackbits(v.bits.cpu().numpy(), axis=1)
        msgs = np.unpackbits(rec[:, 48:80], axis=1)
        assert v.matches.dtype == torch.int32 and v.matches.cpu().tolist() == (got_bits == msgs).sum(axis=1).tolist()
    assert torch.equal(res[0], pipe.verify_records(zd, records, 32, robust_levels=15).bits)
