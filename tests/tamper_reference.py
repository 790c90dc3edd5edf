"""NumPy restatement of the tile agreement map and the tile-weighted vote (tests/test_tamper_host.py, tests/test_gpu_tamper.py).  A plain helper
module, like tests/poison.py and tests/dpm_reference.py: no pytest plugin, no settings.

Everything is written per lattice BIT, on unpacked 0/1 arrays, from the specification: bit j belongs to element
j // l = (c, y, x) in C order, tile (y // T, x // T); the codeword comes from the oracle's `cipher_bits`, the keystream from its `keystream_bits`.
It shares no code with the device path or with gswm_amd.tamper."""
import math

import numpy as np

import gs_oracle as O


def quantise_bits(z, l=1):
    """float latents of one image (any shape) -> the Nb = n l quantised bits, element i at [i l, i l + l), MSB first: y = int(ndtr(z) 2^l)"""
    from scipy.special import ndtr
    y = np.minimum((ndtr(np.asarray(z, dtype=np.float64).reshape(-1)) * (1 << l)).astype(np.int64), (1 << l) - 1)
    return ((y[:, None] >> np.arange(l - 1, -1, -1)[None, :]) & 1).astype(np.uint8).reshape(-1)


def tile_of_bit(shape, l, tile):
    """int64 [Nb]: the flat tile index ty * tw + tx of every lattice bit"""
    C, h, w = shape
    assert h % tile == 0 and w % tile == 0
    e = np.arange(C * h * w * l) // l
    y, x = (e // w) % h, e % w
    return (y // tile) * (w // tile) + x // tile


def codeword(message, key, nonce, nb):
    """the cipher bits the embed plants for (key, nonce, message) over nb lattice bits (nb a multiple of the message's length)"""
    assert nb % (8 * len(message)) == 0
    return O.cipher_bits(message, key, nonce, nb)


def tile_agree(qbits, cw, shape, l, tile):
    """int64 [th, tw]: bits of each tile with q == cw"""
    C, h, w = shape
    t = tile_of_bit(shape, l, tile)
    same = (np.asarray(qbits) == np.asarray(cw)).astype(np.int64)
    return np.bincount(t, weights=same, minlength=(h // tile) * (w // tile)).astype(np.int64).reshape(h // tile, w // tile)


def vote(qbits, ks, weights, M, shape, l, tile):
    """(bits uint8 [M] 0/1, score int64 [M], wsum int64 [M]) of the weighted vote; weights [th, tw] non-negative integers"""
    nb = len(qbits)
    assert nb % M == 0
    p = (np.asarray(qbits) ^ np.asarray(ks)).astype(np.int64)
    wj = np.asarray(weights).astype(np.int64).reshape(-1)[tile_of_bit(shape, l, tile)]
    score = (wj * (2 * p - 1)).reshape(nb // M, M).sum(axis=0)
    wsum = wj.reshape(nb // M, M).sum(axis=0)
    return (score > 0).astype(np.uint8), score, wsum


def default_weights(agree, n_t):
    return np.maximum(2 * np.asarray(agree).astype(np.int64) - n_t - math.isqrt(n_t), 0)


def message_codeword(bits, ks):
    """codeword of a message given as M unpacked bits"""
    return np.asarray(ks) ^ np.tile(np.asarray(bits, dtype=np.uint8), len(ks) // len(bits))


def robust(qbits, key, nonce, M, shape, l=1, tile=8, iters=2):
    """the robust decode of one image -> (bits [M] 0/1, score, wsum, agree [th, tw] against the returned bits)"""
    C, h, w = shape
    ks = O.keystream_bits(key, nonce, len(qbits))
    n_t = C * tile * tile * l
    bits, score, wsum = vote(qbits, ks, np.ones((h // tile, w // tile), np.int64), M, shape, l, tile)
    agree = tile_agree(qbits, message_codeword(bits, ks), shape, l, tile)
    for _ in range(iters):
        bits, score, wsum = vote(qbits, ks, default_weights(agree, n_t), M, shape, l, tile)
        agree = tile_agree(qbits, message_codeword(bits, ks), shape, l, tile)
    return bits, score, wsum, agree


def synthetic_latents(message, key, nonce, shape, sigma, seed, n_images, replaced_rows=0):
    """|g| (2 cw - 1) + sigma noise per element (l = 1), then the top `replaced_rows` lattice rows of every channel replaced by fresh N(0, 1):
    float64 [n_images, C, h, w]; the draws of one call come from one np.random.default_rng(seed), image by image"""
    C, h, w = shape
    n = C * h * w
    cw = codeword(message, key, nonce, n).astype(np.float64)
    rng = np.random.default_rng(seed)
    out = np.empty((n_images, C, h, w))
    for i in range(n_images):
        z = (np.abs(rng.standard_normal(n)) * (2.0 * cw - 1.0) + sigma * rng.standard_normal(n)).reshape(C, h, w)
        if replaced_rows:
            z[:, :replaced_rows, :] = rng.standard_normal((C, replaced_rows, w))
        out[i] = z
    return out
