"""NumPy restatement of `codec.level_pack` (gsw_level_pack) on top of tests/soft_reference.py, and the brute-force
definition of the level-weighted keyed score.  Shares no code with the device path; a plain module, no pytest plugin."""
import numpy as np

import gs_oracle as O
from soft_reference import levels_of


def planes_of(levels: int) -> int:
    return int(levels).bit_length()


def level_rows(z: np.ndarray, thr: np.ndarray) -> dict:
    """z: float32 / float64 [B, n] (`soft_reference.widen`), thr: float32 [levels] or [B, levels] -> signs uint8 [B, n/8], planes uint8
    [B, P, n/8], wsum / wsq int64 [B], flags [B], and the levels themselves int64 [B, n]"""
    B, n = z.shape
    T = thr.shape[-1]
    P = planes_of(T)
    lv = np.stack([levels_of(z[b], thr if thr.ndim == 1 else thr[b]) for b in range(B)])
    z64 = z.astype(np.float64)
    with np.errstate(invalid="ignore"):
        q = (z64 >= O.Y1_THRESHOLD).astype(np.uint8)                                            # a NaN packs as 0
        flags = np.where((z64 >= O.Y2_THRESHOLD).any(axis=1), 1, 0) | np.where(np.isnan(z64).any(axis=1), 2, 0)
    signs = np.packbits(q, axis=1)
    planes = np.stack([np.packbits(((lv >> p) & 1).astype(np.uint8), axis=1) for p in range(P)], axis=1)
    return {"signs": signs, "planes": planes, "wsum": lv.sum(axis=1), "wsq": (lv * lv).sum(axis=1), "flags": flags.astype(np.int64), "levels": lv}


def brute_scores(signs: np.ndarray, levels: np.ndarray, codewords: np.ndarray) -> np.ndarray:
    """score[b, u] = sum_j level_j (1 - 2 (h_j ^ e[u]_j)), pair by pair: int64 [B, U]"""
    h = np.unpackbits(signs, axis=1).astype(np.int64)
    e = np.unpackbits(codewords, axis=1).astype(np.int64)
    out = np.empty((h.shape[0], e.shape[0]), dtype=np.int64)
    for b in range(h.shape[0]):
        for u in range(e.shape[0]):
            out[b, u] = int((levels[b] * (1 - 2 * (h[b] ^ e[u]))).sum())
    return out


# ---- "what it buys": 40 images under 40 distinct keys inside a registry of 1000 records, Gaussian noise of sigma 12 on the latent, fpr 1e-6.
# The CPU test (test_trace_keyed_soft_host.py) runs it on NumPy-drawn latents, the GPU test on codec.embed_records' latents; both add the SAME noise.
BUYS = dict(seed=2024, U=1000, B=40, shape=(4, 64, 64), msg_bytes=32, sigma=12.0, fpr=1e-6, levels=15, clip=2.5)


def buys_setup():
    """-> (records [(key, nonce, message)] x U, owners int [B], codewords uint8 [U, n/8], noise float32 torch [B, n] of unit variance)"""
    import torch
    rng = np.random.default_rng(BUYS["seed"])
    U, B, mb, n = BUYS["U"], BUYS["B"], BUYS["msg_bytes"], int(np.prod(BUYS["shape"]))
    recs = [(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8)), bytes(rng.integers(0, 256, mb, dtype=np.uint8)))
            for _ in range(U)]
    owners = rng.choice(U, B, replace=False)
    cw = np.stack([np.packbits(O.cipher_bits(m, k, nn, n)) for k, nn, m in recs])
    noise = torch.randn(B, n, generator=torch.Generator().manual_seed(BUYS["seed"]))
    return recs, owners, cw, noise


def attributions(idx, log10_p_any, owners, fpr):
    """(images attributed to their true record, images attributed to a wrong one) from the best candidate's index and Bonferroni bound per image"""
    limit = np.log10(fpr)
    right = sum(1 for b in range(len(owners)) if log10_p_any[b] <= limit and idx[b] == owners[b])
    wrong = sum(1 for b in range(len(owners)) if log10_p_any[b] <= limit and idx[b] != owners[b])
    return right, wrong


def brute_topk(scores: np.ndarray, k: int):
    """the k best per row by (score descending, index ascending), padded with -1 / INT32_MIN"""
    B, U = scores.shape
    idx = np.full((B, k), -1, dtype=np.int32)
    out = np.full((B, k), -2 ** 31, dtype=np.int32)
    for b in range(B):
        best = sorted(range(U), key=lambda u: (-int(scores[b, u]), u))[:k]
        idx[b, :len(best)] = best
        out[b, :len(best)] = [scores[b, u] for u in best]
    return idx, out
