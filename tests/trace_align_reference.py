"""NumPy restatement of the aligned registry search (`codec.counts_align`, `trace.trace_latents_aligned`, `trace.trace_latents_keyed_aligned`, DESIGN.md
section 4.25): the vote counts of every alignment are `align_reference.rows_align`, an XOR with the keystream, `unpackbits` and a reshape-sum; the search is a
score per (image, alignment, record) and the merge rule in plain loops.  Shares no code with the device path or with `trace.py` / `align.py`; the statistics
(`log10_p_soft`, `log10_p_any`, ...) are passed in by the caller.  A plain module, no pytest plugin."""
import numpy as np

import align_reference as AR
import key_search_reference as R

INT32_MIN = -2 ** 31


def counts_align(rows: np.ndarray, shape, l: int, aligns, ks_row: np.ndarray, M: int) -> np.ndarray:
    """rows uint8 [B, C H W l / 8], ks_row uint8 [C H W l / 8] -> int64 [B, A, M]: the ones among the copies of every message position of every aligned,
    decrypted row"""
    al = AR.rows_align(rows, shape, l, aligns)
    d = np.unpackbits(al ^ ks_row[None, None, :], axis=2)                 # MSB first: bit p -> byte p >> 3, bit 7 - (p & 7)
    B, A, n = d.shape
    return d.reshape(B, A, n // M, M).sum(axis=2).astype(np.int64)


def scores(counts: np.ndarray, V: int, registry: np.ndarray, soft: bool = True) -> np.ndarray:
    """counts int64 [B, A, M], registry uint8 [U, M / 8] -> S int64 [B, A, U]: sum_t (2 r_t - 1) w_t, w = 2 c - V (soft) or the strict majority as +-1"""
    w = 2 * counts - V if soft else np.where(2 * counts > V, 1, -1)
    r = 2 * np.unpackbits(registry, axis=1).astype(np.int64) - 1
    return np.einsum("bat,ut->bau", w.astype(np.int64), r)


def keyed_scores(al_rows: np.ndarray, codewords: np.ndarray) -> np.ndarray:
    """al_rows uint8 [B, A, n / 8], codewords uint8 [U, n / 8] -> S int64 [B, A, U] = n - 2 popcount(row ^ codeword).  (+-1 products of at most 2^24 terms:
    exact in float32)"""
    B, A, rb = al_rows.shape
    assert rb * 8 <= 1 << 24
    h = 2.0 * np.unpackbits(al_rows.reshape(B * A, rb), axis=1).astype(np.float32) - 1.0
    e = 2.0 * np.unpackbits(codewords, axis=1).astype(np.float32) - 1.0
    return np.rint(h @ e.T).astype(np.int64).reshape(B, A, codewords.shape[0])


def codewords(records, n_bits: int) -> np.ndarray:
    """records [(key, nonce, message)] -> uint8 [U, n_bits / 8]: keystream ^ (message repeated), the cipher bits the embed plants"""
    out = np.empty((len(records), n_bits // 8), dtype=np.uint8)
    for u, (key, nonce, msg) in enumerate(records):
        ks = R.keystreams([(key, nonce)], n_bits)[0]
        out[u] = ks ^ np.resize(np.frombuffer(msg, dtype=np.uint8), n_bits // 8)
    return out


def merge(S: np.ndarray, k: int):
    """S [B, A, U] -> (record, alignment, score) int32 [B, k]: every record keeps its best alignment (the lowest index among equals), the records are ordered
    by (score descending, record ascending) and the first k kept; -1 / -1 / INT32_MIN past the registry's end"""
    B, A, U = S.shape
    rec = np.full((B, k), -1, dtype=np.int32)
    al = np.full((B, k), -1, dtype=np.int32)
    sc = np.full((B, k), INT32_MIN, dtype=np.int32)
    for b in range(B):
        best = []
        for u, col in enumerate(S[b].T.tolist()):                         # col: the A scores of record u, as Python integers
            a = 0
            for i in range(1, A):
                if col[i] > col[a]:
                    a = i
            best.append((-col[a], u, a))
        for j, (neg, u, a) in enumerate(sorted(best)[:k]):
            rec[b, j], al[b, j], sc[b, j] = u, a, -neg
    return rec, al, sc


def trace_host(S: np.ndarray, n: int, log10_p, log10_p_any):
    """S [B, A, U] of a soft search over n lattice bits -> [(record, alignment index, score, Bonferroni bound over U A)] of every image's best pair"""
    B, A, U = S.shape
    rec, al, sc = merge(S, 1)
    return [(int(rec[b, 0]), int(al[b, 0]), int(sc[b, 0]), log10_p_any(log10_p(int(sc[b, 0]), n), U * A)) for b in range(B)]


# ---- the shared-key case: 4 x 32 x 32 latents from the oracle's embed under ONE key, 64-bit messages, a registry of 1000 random messages; six images issued to
# six rows (two of them to the same one), attacked by `align_reference.E2E`'s six alignments, Gaussian noise of sigma 4 from a torch CPU generator, fp16.
SHARED = dict(seed=77, U=1000, rows=(3, 100, 500, 500, 731, 999), shape=(4, 32, 32), msg_bytes=8, fpr=1e-6, sigma=4.0, shift=2, attacks=AR.E2E["attacks"])


def setup(sigma=None):
    """-> dict(key, nonce, registry uint8 [U, 8], clean float64 [6, C, H, W], attacked (noise-free), z16 torch fp16 [6, C, H, W], blank torch fp16 [4, C, H, W],
    ks uint8 [n / 8])"""
    import torch
    import gs_oracle as O
    E = SHARED
    rng = np.random.default_rng(E["seed"])
    n = int(np.prod(E["shape"]))
    key, nonce = bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8))
    registry = rng.integers(0, 256, (E["U"], E["msg_bytes"]), dtype=np.uint8)
    assert len({bytes(r) for r in registry}) == E["U"]
    rs = np.random.RandomState(E["seed"])
    clean = np.stack([np.asarray(O.embed_latent(bytes(registry[r]), key, nonce, rs.uniform(0, 1, n), (n,))).reshape(E["shape"]) for r in E["rows"]])
    attacked = np.stack([AR.apply_np(clean[b], a) for b, a in enumerate(E["attacks"])])
    g = torch.Generator().manual_seed(E["seed"])
    noise = torch.randn(len(E["rows"]), *E["shape"], generator=g, dtype=torch.float64)
    z16 = (torch.from_numpy(attacked) + (E["sigma"] if sigma is None else sigma) * noise).half()
    blank = torch.randn(4, *E["shape"], generator=g).half()
    return dict(key=key, nonce=nonce, registry=registry, clean=clean, attacked=attacked, z16=z16, blank=blank, ks=R.keystreams([(key, nonce)], n)[0])


def shared_scores(z16, aligns, ks_row: np.ndarray, registry: np.ndarray, soft: bool = True):
    """fp16 latents (a torch tensor [B, C, H, W]) -> (counts [B, A, M], S [B, A, U]) of the shared-key search at l = 1"""
    B = z16.shape[0]
    shape = tuple(z16.shape[1:])
    rows = R.sign_rows(z16.reshape(B, -1).double().numpy())
    M = registry.shape[1] * 8
    c = counts_align(rows, shape, 1, aligns, ks_row, M)
    return c, scores(c, rows.shape[1] * 8 // M, registry, soft)


def tile_agree(row: np.ndarray, cw_row: np.ndarray, shape, tile: int) -> np.ndarray:
    """one packed sign row (l = 1) against one packed codeword -> int64 [H / tile, W / tile]: the agreeing bits of every tile, over all channels"""
    C, H, W = shape
    eq = (np.unpackbits(row) == np.unpackbits(cw_row)).reshape(C, H // tile, tile, W // tile, tile)
    return eq.sum(axis=(0, 2, 4)).astype(np.int64)


# ---- the keyed case: `align_reference.e2e_setup()`'s six latents (each under its own key of a 12-key ring, sigma 1), their (key, nonce, message) planted at
# six rows of a registry of 1000 records whose other rows carry random keys, nonces and messages
KEYED = dict(seed=78, U=1000, rows=(3, 100, 500, 501, 731, 999))


def keyed_setup():
    """-> dict(records [(key, nonce, message)] x U, rows, clean, attacked, z16, blank): the records of KEYED["rows"] are the six images' own"""
    E = AR.E2E
    pairs, msgs, clean, attacked, z16, blank = AR.e2e_setup()
    rng = np.random.default_rng(KEYED["seed"])
    records = [(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8)), bytes(rng.integers(0, 256, E["msg_bytes"], dtype=np.uint8)))
               for _ in range(KEYED["U"])]
    for row, ring_row, msg in zip(KEYED["rows"], E["rows"], msgs):
        records[row] = (*pairs[ring_row], msg)
    return dict(records=records, rows=KEYED["rows"], clean=clean, attacked=attacked, z16=z16, blank=blank)


def keyed_search(z16, aligns, records):
    """fp16 latents -> S [B, A, U] of the keyed search at l = 1"""
    B = z16.shape[0]
    shape = tuple(z16.shape[1:])
    rows = R.sign_rows(z16.reshape(B, -1).double().numpy())
    return keyed_scores(AR.rows_align(rows, shape, 1, aligns), codewords(records, rows.shape[1] * 8))
