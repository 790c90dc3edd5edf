"""NumPy restatement of the robust decode with reliability levels (`codec.decode_robust` / gsw_decode_robust), used by
tests/test_robust_soft_host.py and tests/test_gpu_robust_soft.py.  A plain helper module, like tests/tamper_reference.py: no pytest plugin, no settings.

Everything is written per lattice BIT, on unpacked arrays, from the specification: bit j belongs to element j // l = (c, y, x) in C order, tile
(y // T, x // T); p_j = q_j ^ ks_j with the keystream from the oracle's `keystream_bits`; lev_j is given per bit (None: 1 everywhere).  Round r = 0 .. iters
votes with L_j = 1 when r < sign_rounds, else lev_j, and the tile weights wgt^(r), ones in round 0:

    score[t]    = sum over j = t (mod M) of L_j wgt[tile(j)] (2 p_j - 1)        wsum[t] the same sum without the sign        bit_t = score[t] > 0
    excess[tau] = sum over j in tau of L_j (1 - 2 (p_j ^ bit_(j mod M)))          wsq[tau] = sum over j in tau of L_j^2
    wgt^(r+1)[tau] = max(0, excess[tau] - isqrt(wsq[tau]))

It shares no code with the device path or with gswm_amd.tamper."""
import math

import numpy as np

import gs_oracle as O


def tile_index(shape, l, tile):
    """int64 [Nb]: the flat tile ty * tw + tx of every lattice bit"""
    C, h, w = shape
    assert h % tile == 0 and w % tile == 0
    j = np.arange(C * h * w * l, dtype=np.int64)
    e = j // l
    x = e % w
    y = (e // w) % h
    return (y // tile) * (w // tile) + (x // tile)


def decode_p(p, lev, M, shape, l=1, tile=8, iters=2, sign_rounds=0):
    """the rounds on decrypted bits p [Nb] 0/1 and levels lev [Nb] (or None) -> dict of the six outputs of the last round: bits uint8 [M] 0/1, score and
    wsum int64 [M], excess, wsq and weights int64 [th, tw]"""
    C, h, w = shape
    p = np.asarray(p).astype(np.int64)
    nb = p.size
    assert nb == C * h * w * l and nb % M == 0 and 0 <= iters and sign_rounds in (0, 1)
    tau = tile_index(shape, l, tile)
    n_tiles = (h // tile) * (w // tile)
    lev = np.ones(nb, dtype=np.int64) if lev is None else np.asarray(lev).astype(np.int64)
    assert lev.shape == (nb,) and lev.min() >= 0
    wgt = np.ones(n_tiles, dtype=np.int64)
    out = None
    for r in range(iters + 1):
        L = np.ones(nb, dtype=np.int64) if r < sign_rounds else lev
        vote = L * wgt[tau]
        score = (vote * (2 * p - 1)).reshape(nb // M, M).sum(axis=0)
        wsum = vote.reshape(nb // M, M).sum(axis=0)
        bits = (score > 0).astype(np.int64)
        d = p ^ np.tile(bits, nb // M)
        excess = np.zeros(n_tiles, dtype=np.int64)
        wsq = np.zeros(n_tiles, dtype=np.int64)
        np.add.at(excess, tau, L * (1 - 2 * d))
        np.add.at(wsq, tau, L * L)
        out = {"bits": bits.astype(np.uint8), "score": score, "wsum": wsum, "excess": excess.reshape(h // tile, w // tile),
               "wsq": wsq.reshape(h // tile, w // tile), "weights": wgt.reshape(h // tile, w // tile)}
        wgt = np.maximum(excess - np.array([math.isqrt(int(v)) for v in wsq], dtype=np.int64), 0)
    return out


def decode(qbits, key, nonce, lev, M, shape, l=1, tile=8, iters=2, sign_rounds=0):
    """the same from the quantised bits q [Nb] of an image and its key"""
    qbits = np.asarray(qbits).astype(np.uint8)
    ks = np.asarray(O.keystream_bits(key, nonce, qbits.size)).astype(np.uint8)
    return decode_p(qbits ^ ks, lev, M, shape, l, tile, iters, sign_rounds)


def levels_from_planes(planes):
    """uint8 [P, Nb / 8] packed MSB first, plane k = bit k of the level -> int64 [Nb]"""
    planes = np.asarray(planes, dtype=np.uint8)
    return sum(np.unpackbits(planes[k]).astype(np.int64) << k for k in range(planes.shape[0]))


def planes_from_levels(lev, P):
    """int [Nb] in 0 .. 2^P - 1 -> uint8 [P, Nb / 8]"""
    lev = np.asarray(lev).astype(np.int64)
    return np.stack([np.packbits(((lev >> k) & 1).astype(np.uint8)) for k in range(P)])


def soft_weights(excess, wsq):
    return np.maximum(np.asarray(excess).astype(np.int64) - np.array([math.isqrt(int(v)) for v in np.asarray(wsq).reshape(-1)], dtype=np.int64).reshape(np.shape(wsq)), 0)


def uniform_thresholds32(z, levels=15, clip=2.5):
    """float32 [levels]: t_i = (i - 1/2) clip rms / levels for i = 1 .. levels, rms of one image's finite elements in float32 -- the definition of
    `soft.uniform_thresholds`, restated; the last ulp of rms may differ from the device's sum"""
    z = np.asarray(z, dtype=np.float32).reshape(-1)
    ok = np.isfinite(z)
    rms = np.sqrt(np.float32((z[ok].astype(np.float64) ** 2).sum() / max(int(ok.sum()), 1)), dtype=np.float32)
    steps = ((np.arange(1, levels + 1, dtype=np.float32) - np.float32(0.5)) * np.float32(clip / levels)).astype(np.float32)
    return (rms * steps).astype(np.float32)


def levels_of(z, thr):
    """level_j = #{ i : |z_j| >= thr[i] } in float32; NaN -> 0 (l = 1)"""
    z = np.asarray(z, dtype=np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        return (np.abs(z)[:, None] >= np.asarray(thr, dtype=np.float32)[None, :]).sum(axis=1).astype(np.int64)


def sign_bits(z):
    """the l = 1 quantised bit of every element: z >= the median threshold of the oracle (y >= 1 of int(norm.cdf(z) 2))"""
    with np.errstate(invalid="ignore"):
        return (np.asarray(z, dtype=np.float64).reshape(-1) >= O.Y1_THRESHOLD).astype(np.uint8)
