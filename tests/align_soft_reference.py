"""NumPy restatement of the alignment search ranked by reliability levels (`codec.level_rows_align`, `align.search_keys_soft`,
`detect.detect_latents_aligned_soft`): the sign bits and the levels of an image are reshaped to (C, H, W), flipped / turned /
rolled with NumPy's own array functions (`align_reference.apply_np`), scored by `key_search_soft_reference.stats` and merged by
`align_reference.merge`; the bound is `key_search_soft_reference.log10_bound` of the levels UNDER the alignment.  Shares no code with the device path or
with `align.py`; a plain module, no pytest plugin."""
import numpy as np

import align_reference as AR
import key_search_soft_reference as KS
from key_search_reference import keystreams, sign_rows  # noqa: F401

INT32_MIN = AR.INT32_MIN


def aligned(bits_or_levels: np.ndarray, shape, aligns) -> np.ndarray:
    """per-element values [B, n] (sign bits, levels) -> [B, A, n]: every alignment of the image's (C, H, W) lattice"""
    C, H, W = shape
    v = np.asarray(bits_or_levels).reshape(-1, C, H, W)
    return np.stack([AR.apply_np(v, a).reshape(v.shape[0], -1) for a in aligns], axis=1)


def level_rows_align(signs: np.ndarray, planes: np.ndarray, shape, aligns):
    """signs uint8 [B, n/8], planes uint8 [B, P, n/8] -> (uint8 [B, A, n/8], uint8 [B, A, P, n/8]): the levels travel as numbers, not as planes"""
    B, P, nb = planes.shape
    s = aligned(np.unpackbits(signs, axis=1), shape, aligns)                                   # [B, A, n]
    lv = aligned(KS.levels_of_planes(planes), shape, aligns)
    A = s.shape[1]
    out_p = np.stack([KS.planes_of_levels(lv[:, a], P) for a in range(A)], axis=1)             # [B, A, P, n/8]
    return np.packbits(s.astype(np.uint8), axis=2), out_p


def search_stats(signs: np.ndarray, lv: np.ndarray, shape, aligns, ks: np.ndarray, msg_bytes: int) -> np.ndarray:
    """S[b, a, u]: the level-weighted blind statistic of image b under alignment a and key u, int64.  signs uint8 [B, n/8], lv int [B, n]"""
    s = np.packbits(aligned(np.unpackbits(signs, axis=1), shape, aligns).astype(np.uint8), axis=2)
    w = aligned(lv, shape, aligns)
    B, A = s.shape[:2]
    return np.stack([KS.stats(s[:, a], w[:, a], ks, msg_bytes) for a in range(A)], axis=1)


def search_keys(signs, lv, shape, aligns, ks, msg_bytes: int, k: int):
    return AR.merge(search_stats(signs, lv, shape, aligns, ks, msg_bytes), k)


def rows_of(z, thr: np.ndarray):
    """latents (a torch tensor [B, ...]) and the float32 threshold tables [B, levels] -> (signs uint8 [B, n/8], levels int64 [B, n])"""
    zw = KS.widen(z)
    return sign_rows(zw), np.stack([KS.levels_of(zw[b], thr[b]) for b in range(zw.shape[0])])


def detect_host(z, thr: np.ndarray, aligns, ks: np.ndarray, msg_bytes: int, log10_p_any):
    """The restatement of detect_latents_aligned_soft(k=1) on latents z (a torch tensor [B, C, H, W]) with the threshold tables thr float32 [B, levels] of
    the UN-aligned latents against the keystreams ks [K, n/8]: [(key index, alignment index, stat, Bonferroni bound over K A of the Chernoff bound given
    the levels under that alignment, soft-voted message under that key on the aligned image)]"""
    shape = tuple(z.shape[1:])
    signs, lv = rows_of(z, thr)
    key, al, st = search_keys(signs, lv, shape, aligns, ks, msg_bytes, 1)
    M = 8 * msg_bytes
    out = []
    for b in range(signs.shape[0]):
        u, a, s = int(key[b, 0]), int(al[b, 0]), int(st[b, 0])
        s_a = np.packbits(aligned(np.unpackbits(signs[b:b + 1], axis=1), shape, [aligns[a]])[0, 0].astype(np.uint8))
        w_a = aligned(lv[b:b + 1], shape, [aligns[a]])[0, 0]
        out.append((u, a, s, log10_p_any(KS.log10_bound(s, w_a, M), ks.shape[0] * len(aligns)), KS.voted_message(s_a, w_a, ks[u], msg_bytes)))
    return out


# ---- end to end: `align_reference.E2E` (seed 4190, six 4 x 32 x 32 latents under rows of a 12-key keyring, 64-bit messages, the six attacks, A = 200) with
# the noise raised from sigma 1 to sigma 4, 15 levels, fpr 1e-6.  The CPU test runs the restatement on the oracle's latents, the GPU test on
# codec.embed_records' latents of the SAME uniforms, both with the SAME noise.
E2E = dict(AR.E2E, sigma=4.0, levels=15)


def e2e_setup():
    """-> (pairs [(key, nonce)] x K, messages [bytes] x 6, uniforms float64 [6, n], noise float64 torch [6, C, H, W] of unit variance,
    blank: torch fp16 [4, C, H, W] unwatermarked N(0, 1)): the draws of `align_reference.e2e_setup`, in its order"""
    import torch
    E = E2E
    rng = np.random.default_rng(E["seed"])
    n = int(np.prod(E["shape"]))
    pairs = [(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8))) for _ in range(E["K"])]
    msgs = [bytes(rng.integers(0, 256, E["msg_bytes"], dtype=np.uint8)) for _ in E["rows"]]
    rs = np.random.RandomState(E["seed"])
    u = np.stack([rs.uniform(0, 1, n) for _ in E["rows"]])
    g = torch.Generator().manual_seed(E["seed"])
    noise = torch.randn(len(msgs), *E["shape"], generator=g, dtype=torch.float64)
    blank = torch.randn(4, *E["shape"], generator=g).half()
    return pairs, msgs, u, noise, blank


def e2e_host_latents(pairs, msgs, u) -> np.ndarray:
    """the six watermarked latents from the oracle's embed: float64 [6, C, H, W], as embedded"""
    import gs_oracle as O
    n = u.shape[1]
    return np.stack([np.asarray(O.embed_latent(m, *pairs[r], u[b], (n,))).reshape(E2E["shape"]) for b, (r, m) in enumerate(zip(E2E["rows"], msgs))])


def e2e_attack(clean, noise):
    """clean [6, C, H, W] (NumPy, any float type) -> torch fp16 [6, C, H, W]: every image through its attack, plus sigma x noise, cast to fp16"""
    import torch
    attacked = np.stack([AR.apply_np(clean[b], a) for b, a in enumerate(E2E["attacks"])])
    return (torch.from_numpy(attacked).double() + E2E["sigma"] * noise).half()
