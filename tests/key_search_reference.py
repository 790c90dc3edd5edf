"""NumPy restatement of the blind key search (`codec.key_search_topk`): the keystream of every key from the oracle's
ChaCha20, the per-position counts, S = sum_t |2 c_t - V| and a stable top-k.  Shares no code with the device path; a plain module, no
pytest plugin."""
import numpy as np

import gs_oracle as O

INT32_MIN = -2 ** 31


def keystreams(pairs, n_bits: int) -> np.ndarray:
    """pairs: [(key, nonce16)] -> uint8 [K, n_bits / 8], the first n_bits bits of each key's stream"""
    return np.stack([np.frombuffer(O.chacha20_keystream(k, n, n_bits // 8), dtype=np.uint8) for k, n in pairs])


def counts(signs: np.ndarray, ks_row: np.ndarray, msg_bytes: int) -> np.ndarray:
    """signs uint8 [B, n/8] decrypted under ONE keystream row -> int64 [B, M]: the ones among the V copies of every message position"""
    M = 8 * msg_bytes
    d = np.unpackbits(signs ^ ks_row[None, :], axis=1)                     # MSB first: bit j -> byte j >> 3, bit 7 - (j & 7)
    B, n = d.shape
    assert n % M == 0
    return d.reshape(B, n // M, M).astype(np.int64).sum(axis=1)


def stats(signs: np.ndarray, ks: np.ndarray, msg_bytes: int) -> np.ndarray:
    """S[b, u] = sum_t |2 c_t - V|: int64 [B, K]"""
    V = signs.shape[1] * 8 // (8 * msg_bytes)
    out = np.empty((signs.shape[0], ks.shape[0]), dtype=np.int64)
    for u in range(ks.shape[0]):
        out[:, u] = np.abs(2 * counts(signs, ks[u], msg_bytes) - V).sum(axis=1)
    return out


def topk(S: np.ndarray, k: int):
    """the k best per row by (S descending, index ascending), padded with -1 / INT32_MIN"""
    B, K = S.shape
    idx = np.full((B, k), -1, dtype=np.int32)
    out = np.full((B, k), INT32_MIN, dtype=np.int32)
    order = np.argsort(-S, axis=1, kind="stable")[:, :k]
    m = order.shape[1]
    idx[:, :m] = order
    out[:, :m] = np.take_along_axis(S, order, axis=1)
    return idx, out


def voted_message(signs_row: np.ndarray, ks_row: np.ndarray, msg_bytes: int) -> bytes:
    """the strict-majority vote of one image under one key (a tie gives 0), MSB first"""
    c = counts(signs_row[None, :], ks_row, msg_bytes)[0]
    V = signs_row.shape[0] * 8 // (8 * msg_bytes)
    return np.packbits((2 * c > V).astype(np.uint8)).tobytes()


def sign_rows(z: np.ndarray) -> np.ndarray:
    """the oracle's one-bit quantiser, packed: z [B, n] -> uint8 [B, n/8]"""
    return np.packbits((np.asarray(z, dtype=np.float64) >= O.Y1_THRESHOLD).astype(np.uint8), axis=1)


# ---- end to end: six images under rows [0, 3, 50, 50, 117, 199] of a keyring of 200, random unregistered messages, additive Gaussian noise on
# the latent, fp16.  The CPU test (test_detect_host.py) runs the restatement on NumPy-drawn latents, the GPU test runs it on
# codec.embed_records' latents before it asks the device; both add the SAME noise.
E2E = dict(seed=4180, K=200, rows=(0, 3, 50, 50, 117, 199), shape=(4, 64, 64), msg_bytes=32, fpr=1e-6)


def e2e_setup():
    """-> (pairs [(key, nonce)] x K, messages [bytes] x 6, noise float32 torch [6, n] of unit variance, blank float32 torch [2, n]: unwatermarked N(0, 1))"""
    import torch
    rng = np.random.default_rng(E2E["seed"])
    n = int(np.prod(E2E["shape"]))
    pairs = [(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8))) for _ in range(E2E["K"])]
    msgs = [bytes(rng.integers(0, 256, E2E["msg_bytes"], dtype=np.uint8)) for _ in E2E["rows"]]
    g = torch.Generator().manual_seed(E2E["seed"])
    noise = torch.randn(len(E2E["rows"]), n, generator=g)
    blank = torch.randn(2, n, generator=g)
    return pairs, msgs, noise, blank


def e2e_host_latents(pairs, msgs):
    """the six watermarked latents from the oracle's embed with NumPy uniforms: float64 [6, n]"""
    rs = np.random.RandomState(E2E["seed"])
    n = int(np.prod(E2E["shape"]))
    return np.stack([O.embed_latent(m, *pairs[r], rs.uniform(0, 1, n), (n,)) for r, m in zip(E2E["rows"], msgs)])


def detect_host(z16, ks: np.ndarray, msg_bytes: int, log10_p_blind, log10_p_any):
    """The restatement of detect_latents(k=1) on fp16 latents z16 (a torch tensor [B, n]) against the keystreams ks [K, n/8]:
    [(best index, stat, Bonferroni bound, voted message under the best key)].  The two statistics functions are passed in (host code)."""
    signs = sign_rows(z16.double().numpy())
    n_bits = signs.shape[1] * 8
    M = 8 * msg_bytes
    idx, st = topk(stats(signs, ks, msg_bytes), 1)
    out = []
    for b in range(signs.shape[0]):
        i, s = int(idx[b, 0]), int(st[b, 0])
        out.append((i, s, log10_p_any(log10_p_blind(s, M, n_bits // M), ks.shape[0]), voted_message(signs[b], ks[i], msg_bytes)))
    return out
