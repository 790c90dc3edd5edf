"""NumPy restatement of the blind key search ranked by reliability levels (`codec.key_search_soft_topk`, `detect.log10_p_blind_soft`, DESIGN.md section
4.21): the levels from the planes, X_t and S = sum_t |X_t| under every keystream, a stable top-k, and the Chernoff bound of S's null tail given the levels,
restated independently of `detect` (pmfs as pattern counts by one shifted add per element, the minimum over theta by golden section, not by bisection on the
tilted mean).  Shares no code with the device path or with detect.py; a plain module, no pytest plugin."""
import math

import numpy as np

import gs_oracle as O
from key_search_reference import keystreams, sign_rows  # noqa: F401  (the oracle's ChaCha20 keystreams; the oracle's one-bit quantiser)
from soft_reference import levels_of, widen  # noqa: F401

INT32_MIN = -2 ** 31
LN10 = math.log(10.0)


def planes_of_levels(lv: np.ndarray, P: int) -> np.ndarray:
    """levels int [B, n] -> uint8 [B, P, n / 8], plane k = bit k of the levels, packed MSB first"""
    return np.stack([np.packbits(((lv >> p) & 1).astype(np.uint8), axis=1) for p in range(P)], axis=1)


def levels_of_planes(planes: np.ndarray) -> np.ndarray:
    """uint8 [B, P, n / 8] -> int64 [B, n]"""
    B, P, nb = planes.shape
    lv = np.zeros((B, nb * 8), dtype=np.int64)
    for p in range(P):
        lv += np.unpackbits(planes[:, p], axis=1).astype(np.int64) * (1 << p)
    return lv


def margins(signs: np.ndarray, lv: np.ndarray, ks_row: np.ndarray, msg_bytes: int) -> np.ndarray:
    """X[b, t] = sum_{j mod M == t} w_j (2 d_j - 1) under ONE keystream row: int64 [B, M]"""
    M = 8 * msg_bytes
    d = np.unpackbits(signs ^ ks_row[None, :], axis=1).astype(np.int64)    # MSB first: bit j -> byte j >> 3, bit 7 - (j & 7)
    B, n = d.shape
    assert n % M == 0 and lv.shape == d.shape
    return (lv * (2 * d - 1)).reshape(B, n // M, M).sum(axis=1)


def stats(signs: np.ndarray, lv: np.ndarray, ks: np.ndarray, msg_bytes: int) -> np.ndarray:
    """S[b, u] = sum_t |X_t|: int64 [B, K]"""
    out = np.empty((signs.shape[0], ks.shape[0]), dtype=np.int64)
    for u in range(ks.shape[0]):
        out[:, u] = np.abs(margins(signs, lv, ks[u], msg_bytes)).sum(axis=1)
    return out


def topk(S: np.ndarray, k: int):
    """the k best per row by (S descending, index ascending), padded with -1 / INT32_MIN"""
    B, K = S.shape
    idx = np.full((B, k), -1, dtype=np.int32)
    out = np.full((B, k), INT32_MIN, dtype=np.int32)
    for b in range(B):
        best = sorted(range(K), key=lambda u: (-int(S[b, u]), u))[:k]
        idx[b, :len(best)] = best
        out[b, :len(best)] = [S[b, u] for u in best]
    return idx, out


def voted_message(signs_row: np.ndarray, lv_row: np.ndarray, ks_row: np.ndarray, msg_bytes: int) -> bytes:
    """the soft vote of one image under one key: bit t = (X_t > 0), MSB first"""
    x = margins(signs_row[None, :], lv_row[None, :], ks_row, msg_bytes)[0]
    return np.packbits((x > 0).astype(np.uint8)).tobytes()


# ---- the null law, given the levels
def position_laws(lv_row: np.ndarray, M: int):
    """per message position t: (values a of |X_t| ascending, log P[|X_t| = a]), from the number of sign patterns that reach every value of
    Y = sum_j w_j d_j (float64 counts: exact below 2^53, rounded to 1e-16 relative above); X = 2 Y - W"""
    w = np.asarray(lv_row, dtype=np.int64).reshape(-1, M)
    V = w.shape[0]
    assert V <= 1000                                                        # (counts up to 2^V in float64)
    laws = []
    for t in range(M):
        W = int(w[:, t].sum())
        c = np.zeros(W + 1)
        c[0] = 1.0
        for x in w[:, t]:
            if x:
                c[x:] = c[x:] + c[:W + 1 - x]
            else:
                c = 2.0 * c
        a = np.abs(2 * np.arange(W + 1) - W)
        vals = np.unique(a)
        mass = np.array([c[a == v].sum() for v in vals])
        keep = mass > 0
        laws.append((vals[keep].astype(np.float64), np.log(mass[keep]) - V * math.log(2.0)))
    return laws


def _cgf(laws, theta: float) -> float:
    """sum_t log E e^(theta |X_t|)"""
    total = 0.0
    for a, lp in laws:
        x = lp + theta * a
        top = x.max()
        total += top + math.log(np.exp(x - top).sum())
    return total


def log10_bound(stat: int, lv_row: np.ndarray, M: int, laws=None) -> float:
    """min over theta >= 0 of [sum_t log E e^(theta |X_t|) - theta stat] / ln 10; 0.0 at and below E[S]; the exact prod_t P[|X_t| = W_t] at the top"""
    laws = position_laws(lv_row, M) if laws is None else laws
    total = int(sum(a[-1] for a, _ in laws))
    s = int(stat)
    if not 0 <= s <= total:
        raise ValueError(f"stat {s} is outside 0..{total}")
    mean = sum(float((np.exp(lp) * a).sum()) for a, lp in laws)
    if s <= mean:
        return 0.0
    if s == total:
        return sum(float(lp[-1]) for _, lp in laws) / LN10
    f = lambda th: _cgf(laws, th) - th * s                                 # convex in theta, f(0) = 0, f'(0) = E[S] - s < 0
    hi = 1.0
    while f(2.0 * hi) < f(hi):
        hi *= 2.0
    lo, hi = 0.0, 2.0 * hi
    g = (math.sqrt(5.0) - 1.0) / 2.0
    x1, x2 = hi - g * (hi - lo), lo + g * (hi - lo)
    f1, f2 = f(x1), f(x2)
    for _ in range(120):
        if f1 < f2:
            hi, x2, f2 = x2, x1, f1
            x1 = hi - g * (hi - lo)
            f1 = f(x1)
        else:
            lo, x1, f1 = x1, x2, f2
            x2 = lo + g * (hi - lo)
            f2 = f(x2)
    return min(0.0, min(f1, f2) / LN10)


# ---- end to end: six images under six keys of a keyring of 12, random unregistered 64-bit messages, Gaussian noise of sigma 5 on the latent, fp16; four
# unwatermarked images.  The CPU test (test_detect_soft_host.py) runs the restatement on the oracle's latents, the GPU test on codec.embed_records' latents of
# the SAME uniforms, both with the SAME noise.
E2E = dict(seed=2113, K=12, rows=(0, 2, 5, 7, 8, 11), shape=(4, 32, 32), msg_bytes=8, sigma=5.0, fpr=1e-4, levels=15, blanks=4)


def e2e_setup():
    """-> (pairs [(key, nonce)] x K, messages [bytes] x 6, uniforms float64 [6, n], noise float32 torch [6, n] of unit variance, blank float32 torch [4, n])"""
    import torch
    rng = np.random.default_rng(E2E["seed"])
    n = int(np.prod(E2E["shape"]))
    pairs = [(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8))) for _ in range(E2E["K"])]
    msgs = [bytes(rng.integers(0, 256, E2E["msg_bytes"], dtype=np.uint8)) for _ in E2E["rows"]]
    u = np.random.RandomState(E2E["seed"]).uniform(0, 1, (len(E2E["rows"]), n))
    g = torch.Generator().manual_seed(E2E["seed"])
    noise = torch.randn(len(E2E["rows"]), n, generator=g)
    blank = torch.randn(E2E["blanks"], n, generator=g)
    return pairs, msgs, u, noise, blank


def e2e_host_latents(pairs, msgs, u):
    """the six watermarked latents from the oracle's embed: float64 [6, n]"""
    n = u.shape[1]
    return np.stack([O.embed_latent(m, *pairs[r], u[b], (n,)) for b, (r, m) in enumerate(zip(E2E["rows"], msgs))])


def detect_soft_host(z16, thr: np.ndarray, ks: np.ndarray, msg_bytes: int, log10_p_any):
    """The restatement of detect_latents(k=1, reliability=levels) on fp16 latents z16 (a torch tensor [B, n]) with the threshold tables thr float32
    [B, levels] against the keystreams ks [K, n/8]: [(best index, stat, Bonferroni bound, soft-voted message under the best key)]"""
    z = widen(z16)
    signs = sign_rows(z)
    lv = np.stack([levels_of(z[b], thr[b]) for b in range(z.shape[0])])
    M = 8 * msg_bytes
    idx, st = topk(stats(signs, lv, ks, msg_bytes), 1)
    out = []
    for b in range(signs.shape[0]):
        i, s = int(idx[b, 0]), int(st[b, 0])
        out.append((i, s, log10_p_any(log10_bound(s, lv[b], M), ks.shape[0]), voted_message(signs[b], lv[b], ks[i], msg_bytes)))
    return out
