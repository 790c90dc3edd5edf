"""NumPy restatement of the alignment search (`codec.rows_align`, `align.search_keys`): a packed row is unpacked to its
l-bit groups, flipped / turned / rolled with NumPy's own array functions and packed again; the search is `key_search_reference.stats` on every
aligned row and the merge rule, in plain loops.  Shares no code with the device path or with `align.py`; a plain module, no pytest plugin."""
import numpy as np

import key_search_reference as R

INT32_MIN = -2 ** 31


def apply_np(z: np.ndarray, a) -> np.ndarray:
    """a = (d, dy, dx) on the axes (H, W) = (-2, -1) of z [..., H, W] (any trailing axes must be moved away by the caller)"""
    d, dy, dx = a
    t = np.flip(z, axis=-1) if d & 4 else z
    t = np.rot90(t, d & 3, axes=(-2, -1))
    return np.roll(t, (dy, dx), axis=(-2, -1))


def rows_align(rows: np.ndarray, shape, l: int, aligns) -> np.ndarray:
    """rows uint8 [B, C H W l / 8] -> uint8 [B, A, C H W l / 8]"""
    C, H, W = shape
    B = rows.shape[0]
    bits = np.unpackbits(rows, axis=1).reshape(B, C, H, W, l)          # MSB first: element e owns bits [e l, e l + l)
    out = np.empty((B, len(aligns), rows.shape[1]), dtype=np.uint8)
    for i, a in enumerate(aligns):
        t = apply_np(np.moveaxis(bits, -1, 1), a)                      # [B, l, C, H', W']: the group of an element travels with it
        out[:, i] = np.packbits(np.ascontiguousarray(np.moveaxis(t, 1, -1)).reshape(B, -1), axis=1)
    return out


def search_stats(rows: np.ndarray, shape, l: int, aligns, ks: np.ndarray, msg_bytes: int) -> np.ndarray:
    """S[b, a, u]: the blind statistic of image b's row under alignment a and key u, int64"""
    al = rows_align(rows, shape, l, aligns)
    B, A, rb = al.shape
    return R.stats(al.reshape(B * A, rb), ks, msg_bytes).reshape(B, A, ks.shape[0])


def merge(S: np.ndarray, k: int):
    """S [B, A, K] -> (key, align, stat) int32 [B, k]: every key keeps its best alignment (the lowest index among equals), the keys are ordered by
    (stat descending, key ascending) and the first k kept; -1 / -1 / INT32_MIN past the keyring's end"""
    B, A, K = S.shape
    key = np.full((B, k), -1, dtype=np.int32)
    al = np.full((B, k), -1, dtype=np.int32)
    st = np.full((B, k), INT32_MIN, dtype=np.int32)
    for b in range(B):
        best = []
        for u in range(K):
            a = min(range(A), key=lambda i: (-int(S[b, i, u]), i))
            best.append((-int(S[b, a, u]), u, a))
        for j, (neg, u, a) in enumerate(sorted(best)[:k]):
            key[b, j], al[b, j], st[b, j] = u, a, -neg
    return key, al, st


def search_keys(rows: np.ndarray, shape, l: int, aligns, ks: np.ndarray, msg_bytes: int, k: int):
    return merge(search_stats(rows, shape, l, aligns, ks, msg_bytes), k)


# ---- end to end: six 4 x 32 x 32 latents from the oracle's embed under rows of a 12-key keyring, random 64-bit messages; each is attacked on the host by
# one alignment, gets unit Gaussian noise and is cast to fp16.  The candidates of the search are all eight orientations x shifts in [-2, 2]^2 (A = 200).
E2E = dict(seed=4190, K=12, rows=(0, 3, 5, 5, 7, 11), shape=(4, 32, 32), msg_bytes=8, fpr=1e-6, sigma=1.0, shift=2,
           attacks=((0, 0, 0), (4, 0, 0), (1, 0, 0), (2, 1, -2), (7, -2, 2), (5, 2, 1)))


def e2e_setup():
    """-> (pairs [(key, nonce)] x K, messages [bytes] x 6, clean float64 [6, C, H, W] as embedded, attacked float64 [6, C, H, W] noise-free,
    z16: torch fp16 [6, C, H, W] attacked + noise, blank: torch fp16 [4, C, H, W] unwatermarked N(0, 1))"""
    import torch
    import gs_oracle as O
    E = E2E
    rng = np.random.default_rng(E["seed"])
    n = int(np.prod(E["shape"]))
    pairs = [(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8))) for _ in range(E["K"])]
    msgs = [bytes(rng.integers(0, 256, E["msg_bytes"], dtype=np.uint8)) for _ in E["rows"]]
    rs = np.random.RandomState(E["seed"])
    clean = np.stack([np.asarray(O.embed_latent(m, *pairs[r], rs.uniform(0, 1, n), (n,))).reshape(E["shape"]) for r, m in zip(E["rows"], msgs)])
    attacked = np.stack([apply_np(clean[b], a) for b, a in enumerate(E["attacks"])])
    g = torch.Generator().manual_seed(E["seed"])
    noise = torch.randn(len(msgs), *E["shape"], generator=g, dtype=torch.float64)
    z16 = (torch.from_numpy(attacked) + E["sigma"] * noise).half()
    blank = torch.randn(4, *E["shape"], generator=g).half()
    return pairs, msgs, clean, attacked, z16, blank


def detect_host(z16, aligns, ks: np.ndarray, msg_bytes: int, log10_p_blind, log10_p_any):
    """The restatement of detect_latents(k=1, align=aligns) on fp16 latents z16 (a torch tensor [B, C, H, W]) against the keystreams ks [K, n/8]:
    [(key index, alignment index, stat, Bonferroni bound over K A, message voted under that key on the aligned row)]"""
    B = z16.shape[0]
    shape = tuple(z16.shape[1:])
    rows = R.sign_rows(z16.reshape(B, -1).double().numpy())
    key, al, st = search_keys(rows, shape, 1, aligns, ks, msg_bytes, 1)
    M, n_bits = 8 * msg_bytes, rows.shape[1] * 8
    out = []
    for b in range(B):
        u, a, s = int(key[b, 0]), int(al[b, 0]), int(st[b, 0])
        row = rows_align(rows[b:b + 1], shape, 1, [aligns[a]])[0, 0]
        out.append((u, a, s, log10_p_any(log10_p_blind(s, M, n_bits // M), ks.shape[0] * len(aligns)), R.voted_message(row, ks[u], msg_bytes)))
    return out


def quant_rows(z: np.ndarray, l: int, thresholds) -> np.ndarray:
    """the l-bit quantiser on float64 thresholds, packed: z [B, n] -> uint8 [B, n l / 8]; y = #{thresholds <= z}"""
    y = (np.asarray(z, dtype=np.float64)[..., None] >= np.asarray(thresholds, dtype=np.float64)).sum(axis=-1).astype(np.uint8)
    bits = (y[..., None] >> np.arange(l - 1, -1, -1, dtype=np.uint8)) & 1
    return np.packbits(bits.reshape(z.shape[0], -1).astype(np.uint8), axis=1)
