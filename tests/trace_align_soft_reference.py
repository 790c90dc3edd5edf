"""NumPy restatement of the aligned registry search ranked by reliability levels (`codec.level_counts_align`, `trace.trace_latents_aligned_soft`,
`trace.trace_latents_keyed_aligned_soft`): the sign bits and the levels of an image travel through every alignment as numbers
(`align_soft_reference.aligned`), the level-weighted vote of an aligned image is `key_search_soft_reference.margins`, the shared-key score an einsum with the
registry's +-1 messages, the keyed score a level-weighted correlation with the codewords, the merge `trace_align_reference.merge`.  Shares no code with the
device path or with `trace.py` / `align.py`; the statistics (`soft.log10_p`, `trace.log10_p_any`) and the threshold tables are passed in by the caller.  A
plain module, no pytest plugin."""
import numpy as np

import align_reference as AR
import align_soft_reference as ASR
import key_search_soft_reference as KS
import trace_align_reference as TR

INT32_MIN = TR.INT32_MIN
SATURATES_AT = 8.296875                 # the smallest fp16 at which float64 norm.cdf is 1.0: the reference cannot read such an element


def aligned_rows(signs: np.ndarray, lv: np.ndarray, shape, aligns):
    """signs uint8 [B, n/8], lv int [B, n] -> (uint8 [B, A, n/8], int64 [B, A, n]): the sign row and the levels of every aligned image"""
    s = np.packbits(ASR.aligned(np.unpackbits(signs, axis=1), shape, aligns).astype(np.uint8), axis=2)
    return s, ASR.aligned(lv, shape, aligns).astype(np.int64)


def level_counts_align(signs: np.ndarray, lv: np.ndarray, shape, aligns, ks_row: np.ndarray, M: int):
    """-> (score, wsum) int64 [B, A, M]: score[b, a, t] = sum over p = t (mod M) of level_p (2 d_p - 1) of image b under alignment a, wsum the same sum of
    level_p alone"""
    s, w = aligned_rows(signs, lv, shape, aligns)
    B, A, n = w.shape
    score = np.stack([KS.margins(s[:, a], w[:, a], ks_row, M // 8) for a in range(A)], axis=1)
    return score, w.reshape(B, A, n // M, M).sum(axis=2)


def shared_scores(score: np.ndarray, registry: np.ndarray) -> np.ndarray:
    """score int64 [B, A, M], registry uint8 [U, M / 8] -> S int64 [B, A, U] = sum_t (2 r_t - 1) score[t]"""
    r = 2 * np.unpackbits(registry, axis=1).astype(np.int64) - 1
    return np.einsum("bat,ut->bau", score.astype(np.int64), r)


def keyed_scores(s_al: np.ndarray, w_al: np.ndarray, codewords: np.ndarray) -> np.ndarray:
    """aligned sign rows uint8 [B, A, n/8], aligned levels [B, A, n], codewords uint8 [U, n/8] -> S int64 [B, A, U] = sum_j level_j (1 - 2 (sign_j ^
    codeword_j)).  (Products of integers below 16 with +-1, at most 2^20 terms: exact in float64)"""
    B, A, n = w_al.shape
    h = (w_al * (1 - 2 * np.unpackbits(s_al, axis=2).astype(np.int64))).reshape(B * A, n).astype(np.float64)
    e = 1.0 - 2.0 * np.unpackbits(codewords, axis=1).astype(np.float64)
    return np.rint(h @ e.T).astype(np.int64).reshape(B, A, codewords.shape[0])


merge = TR.merge


def trace_host(S: np.ndarray, wsq, log10_p, log10_p_any):
    """S [B, A, U] of a level-weighted search, wsq [B] the images' sums of squared levels -> [(record, alignment index, score, Bonferroni bound over U A of
    Hoeffding's bound)] of every image's best pair"""
    B, A, U = S.shape
    rec, al, sc = merge(S, 1)
    return [(int(rec[b, 0]), int(al[b, 0]), int(sc[b, 0]), log10_p_any(log10_p(int(sc[b, 0]), int(wsq[b])), U * A)) for b in range(B)]


def hold(z16):
    """fp16 latents held just below the value at which the reference refuses an image: no sign changes, and the thresholds are taken AFTER this"""
    return z16.clamp(max=SATURATES_AT - 2.0 ** -7)


# ---- the shared-key case: `trace_align_reference.setup` with the noise raised from sigma 4 to 5.75, where the sign statistic no longer names all six
SHARED = dict(TR.SHARED, sigma=5.75, levels=15)


def shared_setup(sigma=None):
    """-> `trace_align_reference.setup(sigma)` plus held (torch fp16 [6, C, H, W]) and held_blank"""
    s = TR.setup(SHARED["sigma"] if sigma is None else sigma)
    return dict(s, held=hold(s["z16"]), held_blank=hold(s["blank"]))


# ---- the keyed case: `align_soft_reference.e2e_setup()`'s six latents (each under its own key of a 12-key ring) with noise of sigma 5, their records planted
# at `trace_align_reference.KEYED["rows"]` among 1000 random ones
KEYED = dict(TR.KEYED, sigma=5.0, levels=15, shape=ASR.E2E["shape"], msg_bytes=ASR.E2E["msg_bytes"], fpr=ASR.E2E["fpr"], shift=ASR.E2E["shift"],
             attacks=ASR.E2E["attacks"])


def keyed_setup(sigma=None):
    """-> dict(records [(key, nonce, message)] x U, rows, clean float64 [6, C, H, W], attacked, held torch fp16 [6, C, H, W], held_blank, z16)"""
    import torch
    E = ASR.E2E
    pairs, msgs, u, noise, blank = ASR.e2e_setup()
    clean = ASR.e2e_host_latents(pairs, msgs, u)
    attacked = np.stack([AR.apply_np(clean[b], a) for b, a in enumerate(E["attacks"])])
    z16 = (torch.from_numpy(attacked).double() + (KEYED["sigma"] if sigma is None else sigma) * noise).half()
    rng = np.random.default_rng(KEYED["seed"])
    records = [(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8)), bytes(rng.integers(0, 256, E["msg_bytes"], dtype=np.uint8)))
               for _ in range(KEYED["U"])]
    for row, ring_row, msg in zip(KEYED["rows"], E["rows"], msgs):
        records[row] = (*pairs[ring_row], msg)
    return dict(records=records, rows=KEYED["rows"], clean=clean, attacked=attacked, z16=z16, held=hold(z16), held_blank=hold(blank))


def shared_search(z16, thr: np.ndarray, aligns, ks_row: np.ndarray, registry: np.ndarray):
    """fp16 latents (a torch tensor [B, C, H, W]) and their threshold tables float32 [B, levels] -> (score [B, A, M], S [B, A, U], wsq [B])"""
    signs, lv = ASR.rows_of(z16, thr)
    score, _ = level_counts_align(signs, lv, tuple(z16.shape[1:]), aligns, ks_row, registry.shape[1] * 8)
    return score, shared_scores(score, registry), (lv * lv).sum(axis=1)


def keyed_search(z16, thr: np.ndarray, aligns, records):
    """fp16 latents and their threshold tables -> (S [B, A, U], wsq [B]) of the keyed level-weighted search"""
    signs, lv = ASR.rows_of(z16, thr)
    s, w = aligned_rows(signs, lv, tuple(z16.shape[1:]), aligns)
    return keyed_scores(s, w, TR.codewords(records, signs.shape[1] * 8)), (lv * lv).sum(axis=1)
