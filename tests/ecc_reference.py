"""NumPy restatement of the error-corrected payload: the rate-1/2, constraint-length-7 convolutional code (0o171, 0o133) with a zero
tail, CRC-16/CCITT-FALSE and the multiplicative interleaver, and its maximum-correlation Viterbi decoder.  Integer arithmetic throughout: the device
(`codec.viterbi_decode`) and the package's host encoder (`ecc.encode`) must equal it bit for bit.  Written from the definitions, not from the package."""
import math

import numpy as np

G0, G1 = 0o171, 0o133
TAIL = 6


def check_length(M):
    if isinstance(M, bool) or not isinstance(M, (int, np.integer)) or M % 16 or not 64 <= M <= 8192:
        raise ValueError(f"message_length must be a multiple of 16 in 64..8192, got {M!r}")
    return int(M)


def sizes(M):
    """-> (I info bits, T trellis steps, payload bytes)"""
    M = check_length(M)
    T = M // 2
    I = T - TAIL
    return I, T, (I - 16) // 8


def capacity(M):
    return sizes(M)[2]


def interleaver_step(M):
    S = math.isqrt(M) | 1
    while math.gcd(S, M) != 1:
        S += 2
    return S


def positions(M, interleave=True):
    """message position of code bit i"""
    i = np.arange(M, dtype=np.int64)
    return (i * interleaver_step(M)) % M if interleave else i


def crc16(data: bytes) -> int:
    crc = 0xFFFF
    for byte in data:
        crc ^= byte << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    return crc


def info_word(payload: bytes, M) -> np.ndarray:
    """uint8 [I]: payload bits MSB first, CRC-16, zero pad"""
    I, _, pb = sizes(M)
    if len(payload) != pb:
        raise ValueError(f"a payload of {len(payload)} bytes; message_length {M} carries exactly {pb}")
    c = crc16(payload)
    bits = np.unpackbits(np.frombuffer(bytes(payload) + bytes([c >> 8, c & 0xFF]), dtype=np.uint8))
    return np.concatenate([bits, np.zeros(I - bits.size, dtype=np.uint8)])


def conv_encode(u) -> np.ndarray:
    """input bits (tail included) -> 2 len(u) code bits, by the shift register as the issue states it"""
    out, s = [], 0
    for bit in u:
        r = (int(bit) << 6) | s
        out += [bin(r & G0).count("1") & 1, bin(r & G1).count("1") & 1]
        s = r >> 1
    return np.array(out, dtype=np.uint8)


def encode_bits(info, M, interleave=True) -> np.ndarray:
    """uint8 [M] message bits of an info word of I bits"""
    code = conv_encode(np.concatenate([np.asarray(info, dtype=np.uint8), np.zeros(TAIL, dtype=np.uint8)]))
    msg = np.zeros(M, dtype=np.uint8)
    msg[positions(M, interleave)] = code
    return msg


def encode(payload: bytes, M, interleave=True) -> bytes:
    return np.packbits(encode_bits(info_word(payload, M), M, interleave)).tobytes()


def _labels():
    s = np.arange(64)
    r = ((s >> 5) << 6) | (2 * (s & 31))
    par = lambda v: np.array([bin(int(x)).count("1") & 1 for x in v])
    return par(r & G0), par(r & G1)


def decode(score, interleave=True) -> dict:
    """score int [B, M] -> info uint8 [B, M/16], message uint8 [B, M/8], metric, flips, ok int32 [B]"""
    score = np.asarray(score)
    assert score.ndim == 2 and np.issubdtype(score.dtype, np.integer)
    B, M = score.shape
    I, T, pb = sizes(M)
    assert int(np.abs(score.astype(np.int64)).sum(axis=1).max()) < 2 ** 30
    pos = positions(M, interleave)
    x = score.astype(np.int64)[:, pos]                              # x[:, i]: the vote of code bit i
    s = np.arange(64)
    p0, u = 2 * (s & 31), s >> 5
    l0, l1 = _labels()
    sg0, sg1 = 2 * l0 - 1, 2 * l1 - 1
    pm = np.zeros((B, 64), dtype=np.int64)
    reach = np.zeros(64, dtype=bool)
    reach[0] = True
    dec = np.zeros((T, B, 64), dtype=bool)
    for t in range(T):
        bm = sg0[None, :] * x[:, 2 * t, None] + sg1[None, :] * x[:, 2 * t + 1, None]
        c0, c1 = pm[:, p0] + bm, pm[:, p0 + 1] - bm
        r0, r1 = reach[p0], reach[p0 + 1]
        d = r1[None, :] & (~r0[None, :] | (c1 > c0))
        live = (r0 | r1) & ((u == 0) if t >= I else np.ones(64, dtype=bool))
        pm = np.where(live[None, :], np.where(d, c1, c0), 0)
        reach = live
        dec[t] = d
    metric = pm[:, 0].astype(np.int32)
    st = np.zeros(B, dtype=np.int64)
    ub = np.zeros((B, T), dtype=np.uint8)
    rows = np.arange(B)
    for t in range(T - 1, -1, -1):
        ub[:, t] = st >> 5
        st = 2 * (st & 31) + dec[t][rows, st]
    # re-encode: delay k of the input meets bit 6 - k of the generators
    up = np.concatenate([np.zeros((B, TAIL), dtype=np.uint8), ub], axis=1)
    c = np.zeros((B, T, 2), dtype=np.uint8)
    for k in range(TAIL + 1):
        past = up[:, TAIL - k:TAIL - k + T]
        if (G0 >> (6 - k)) & 1:
            c[:, :, 0] ^= past
        if (G1 >> (6 - k)) & 1:
            c[:, :, 1] ^= past
    code = c.reshape(B, M)
    msg = np.zeros((B, M), dtype=np.uint8)
    msg[:, pos] = code
    flips = (msg != (score > 0)).sum(axis=1).astype(np.int32)
    info = np.packbits(ub, axis=1)                                  # T = 8 (M / 16): the tail's zeros fill the last byte
    ok = np.array([crc16(info[b, :pb].tobytes()) == (int(info[b, pb]) << 8 | int(info[b, pb + 1])) and info[b, pb + 2] == 0 for b in range(B)], dtype=np.int32)
    return {"info": info, "message": np.packbits(msg, axis=1), "metric": metric, "flips": flips, "ok": ok}


def payloads(info, M):
    pb = capacity(M)
    return [np.asarray(info)[b, :pb].tobytes() for b in range(len(info))]


# ------------------------------------------------------------------------------------------------ the sigma walk (tools/ecc_sigma_walk.py, the end-to-end tests)
WALK = {"shape": (4, 32, 32), "M": 256, "levels": 15, "clip": 2.5, "images": 20, "seed": 20260429,
        "sigmas": [0.5 + 0.25 * i for i in range(15)],             # 0.5 .. 4.0
        "sigma": 2.5}                                              # the recorded outcome: `chosen_sigma(walk())`, asserted by tests/test_ecc_host.py


def uniform_thresholds32(z, levels=15, clip=2.5):
    """`soft.uniform_thresholds` for one image, restated: float32 [levels], t_i = (i - 1/2) clip rms / levels"""
    z = np.asarray(z, dtype=np.float32).reshape(-1)
    ok = np.isfinite(z)
    rms = np.sqrt(np.float32((z[ok].astype(np.float64) ** 2).sum() / max(int(ok.sum()), 1)), dtype=np.float32)
    steps = ((np.arange(1, levels + 1, dtype=np.float32) - np.float32(0.5)) * np.float32(clip / levels)).astype(np.float32)
    return (rms * steps).astype(np.float32)


def walk_setup():
    """the fixed inputs of the walk: a keyring of 12 (key, nonce) pairs, image b under pair b mod 12; per image a payload, the embed's uniforms and unit noise.
    The uniforms are NumPy's legacy MT19937 stream of the seed, which `issue.issue_latents(seed=None)` draws on the device after np.random.seed(seed): the
    end-to-end tests issue these very images (up to the embed's 1e-5)."""
    rng = np.random.default_rng(WALK["seed"])
    n, B = int(np.prod(WALK["shape"])), WALK["images"]
    pb = capacity(WALK["M"])
    ring = [(rng.bytes(32), rng.bytes(16)) for _ in range(12)]
    return {"ring": ring, "keys": [ring[b % 12][0] for b in range(B)], "nonces": [ring[b % 12][1] for b in range(B)],
            "payloads": [rng.bytes(pb) for _ in range(B)], "u": np.random.RandomState(WALK["seed"]).uniform(0.0, 1.0, (B, n)),
            "noise": rng.standard_normal((B, n)).astype(np.float32), "blank": rng.standard_normal((64, n)).astype(np.float32)}


def uncoded_message(payload: bytes) -> bytes:
    """the alternative without the code: the same bytes and CRC as a 128-bit message (one zero byte of pad), which gets twice the copies"""
    c = crc16(payload)
    return bytes(payload) + bytes([c >> 8, c & 0xFF, 0])


def held(z, noise, sigma):
    """the attacked latents as both sides see them: float32, z + sigma noise brought back to unit variance, as inverted latents are"""
    return ((np.asarray(z, dtype=np.float32) + np.float32(sigma) * noise) / np.float32((1.0 + sigma * sigma) ** 0.5)).astype(np.float32)


def walk_latents(setup, messages):
    """float32 [B, n]: image b carries messages[b] under its own key and nonce, by the oracle's embed"""
    import gs_oracle as O
    return np.stack([O.embed_latent(m, setup["keys"][b], setup["nonces"][b], setup["u"][b], WALK["shape"]).reshape(-1)
                     for b, m in enumerate(messages)]).astype(np.float32)


def walk_scores(setup, z, msg_bits):
    """the soft vote of every image under its own key, 15 uniform levels on its own RMS -> (score int32 [B, msg_bits], thresholds float32 [B, levels])"""
    import gs_oracle as O
    import soft_reference as SR
    thr = np.stack([uniform_thresholds32(row, WALK["levels"], WALK["clip"]) for row in z])
    score = np.stack([SR.soft_vote(z[b], np.frombuffer(O.chacha20_keystream(setup["keys"][b], setup["nonces"][b], z.shape[1] // 8), dtype=np.uint8), thr[b],
                                   msg_bits)["score"] for b in range(len(z))]).astype(np.int32)
    return score, thr


def walk_point(setup, sigma, coded_z, uncoded_z):
    """-> (coded images whose payload reads back exactly with ok, uncoded images whose every bit is right)"""
    M = WALK["M"]
    score, _ = walk_scores(setup, held(coded_z, setup["noise"], sigma), M)
    d = decode(score)
    got = payloads(d["info"], M)
    coded = sum(1 for b, p in enumerate(setup["payloads"]) if got[b] == p and d["ok"][b])
    score_u, _ = walk_scores(setup, held(uncoded_z, setup["noise"], sigma), M // 2)
    want = np.stack([np.unpackbits(np.frombuffer(uncoded_message(p), dtype=np.uint8)) for p in setup["payloads"]])
    uncoded = int(((score_u > 0) == (want > 0)).all(axis=1).sum())
    return coded, uncoded


def walk():
    """[(sigma, coded, uncoded)] over the grid"""
    setup = walk_setup()
    coded_z = walk_latents(setup, [encode(p, WALK["M"]) for p in setup["payloads"]])
    uncoded_z = walk_latents(setup, [uncoded_message(p) for p in setup["payloads"]])
    return [(s,) + walk_point(setup, s, coded_z, uncoded_z) for s in WALK["sigmas"]]


def chosen_sigma(table):
    """the LARGEST grid point at which all coded payloads read back with ok; None when there is none"""
    full = [s for s, c, _ in table if c == WALK["images"]]
    return max(full) if full else None


def score_of(message: bytes, magnitude: int = 1) -> np.ndarray:
    """the noiseless votes of a message: +-magnitude"""
    bits = np.unpackbits(np.frombuffer(message, dtype=np.uint8)).astype(np.int64)
    return ((2 * bits - 1) * magnitude).astype(np.int32)
