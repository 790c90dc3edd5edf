"""NumPy restatement of pooled evidence across the images of a set: `codec.pool_rows`, `codec.trace_keyed_pooled_topk` and the
statistics of `trace.trace_sets_keyed`.  It unpacks bits, forms S as int64 and scores with plain sums; it shares no code with the device path.  A plain
module, no pytest plugin."""
import math

import numpy as np

import gs_oracle as O

MAX_Q = 10


def levels_of_planes(planes, n_images: int, n: int) -> np.ndarray:
    """planes uint8 [B, P, n / 8] or None (unit levels) -> int64 [B, n]"""
    if planes is None:
        return np.ones((n_images, n), dtype=np.int64)
    bits = np.unpackbits(planes, axis=2).astype(np.int64)
    return sum(bits[:, k] << k for k in range(planes.shape[1]))


def signed_sums(signs, planes, sets) -> np.ndarray:
    """S[g, j] = sum over the images b of set g of lev_bj (1 - 2 h_bj): int64 [G, n]"""
    h = np.unpackbits(signs, axis=1).astype(np.int64)
    lev = levels_of_planes(planes, *h.shape)
    return np.stack([sum(lev[b] * (1 - 2 * h[b]) for b in members) for members in sets])


def planes_needed(P: int, max_set: int) -> int:
    return int(((2 ** P - 1 if P else 1) * max_set)).bit_length()


def pool_rows(signs, planes, sets) -> dict:
    """-> signs uint8 [G, n / 8], planes uint8 [G, Q, n / 8], wsum / wsq int64 [G], S int64 [G, n]; Q from the LARGEST set, as the wrapper chooses it"""
    S = signed_sums(signs, planes, sets)
    Q = planes_needed(0 if planes is None else planes.shape[1], max(len(m) for m in sets))
    mag = np.abs(S)
    assert int(mag.max()) < 2 ** Q
    return {"signs": np.packbits((S < 0).astype(np.uint8), axis=1),
            "planes": np.stack([np.packbits(((mag >> k) & 1).astype(np.uint8), axis=1) for k in range(Q)], axis=1),
            "wsum": mag.sum(axis=1), "wsq": (S * S).sum(axis=1), "S": S, "Q": Q}


def scores(S, codewords) -> np.ndarray:
    """score[g, u] = sum_j S_gj (1 - 2 e[u]_j): int64 [G, U]"""
    e = 1 - 2 * np.unpackbits(codewords, axis=1).astype(np.int64)
    return S @ e.T


def sums_of_rows(signs, planes, wsum) -> np.ndarray:
    """the signed sums a packed pooled row stands for: int64 [G, n] (the search alone, on rows made on the host)"""
    h = np.unpackbits(signs, axis=1).astype(np.int64)
    return levels_of_planes(planes, *h.shape) * (1 - 2 * h)


def topk(sc: np.ndarray, k: int):
    """the k best per row by (score descending, index ascending), padded with -1 / INT32_MIN"""
    G, U = sc.shape
    idx = np.full((G, k), -1, dtype=np.int32)
    out = np.full((G, k), -2 ** 31, dtype=np.int32)
    for g in range(G):
        best = sorted(range(U), key=lambda u: (-int(sc[g, u]), u))[:k]
        idx[g, :len(best)] = best
        out[g, :len(best)] = [sc[g, u] for u in best]
    return idx, out


def bound(score: int, wsq: int, U: int) -> float:
    """Hoeffding's bound of the pooled score in decades, Bonferroni over U records, capped at 0"""
    lp = 0.0 if score <= 0 or wsq <= 0 else -(score * score) / (2.0 * wsq * math.log(10.0))
    return min(0.0, lp + math.log10(U))


def agree(S_row, record, n: int) -> int:
    """message bits of the pooled vote under the record's own key that equal its message"""
    key, nonce, msg = record
    M = 8 * len(msg)
    ks = np.asarray(O.keystream_bits(key, nonce, n)).astype(np.int64)
    # S_j (1 - 2 ks_j) is level_j (1 - 2 d_j) for the decrypted bit d_j; the vote for bit 1 is its negative
    vote = (-(S_row * (1 - 2 * ks))).reshape(-1, M).sum(axis=0)
    want = np.unpackbits(np.frombuffer(msg, dtype=np.uint8)).astype(np.int64)
    return int((((vote > 0).astype(np.int64)) == want).sum())


def trace_sets(signs, planes, flags, sets, records, codewords, k: int, fpr: float):
    """The statistics of `trace.trace_sets_keyed` on packed rows -> per set None (left empty) or a dict: candidates [(index, score, agree, bound)], attributed
    index or None, size, skipped, wsq"""
    n, U, limit = signs.shape[1] * 8, len(records), math.log10(fpr)
    out = []
    for members in sets:
        kept = [b for b in members if not flags[b]]
        if not kept:
            out.append(None)
            continue
        S = signed_sums(signs, planes, [kept])
        wsq = int((S * S).sum())
        idx, sc = topk(scores(S, codewords), k)
        cands = [(int(i), int(s), agree(S[0], records[int(i)], n), bound(int(s), wsq, U)) for i, s in zip(idx[0], sc[0]) if i >= 0]
        out.append({"candidates": cands, "attributed": cands[0][0] if cands and cands[0][3] <= limit else None, "size": len(kept),
                    "skipped": len(members) - len(kept), "wsq": wsq})
    return out


def sign_rows(z) -> np.ndarray:
    """the quantiser at l = 1: uint8 [B, n / 8]"""
    return np.packbits((np.asarray(z, dtype=np.float64).reshape(len(z), -1) >= O.Y1_THRESHOLD).astype(np.uint8), axis=1)


# ---- what pooling buys: 16 images of 4 x 32 x 32 under ONE record among 1000 keyed records, Gaussian noise of sigma 12 on the latent, fpr 1e-6, unit levels.
# Alone no image is attributed (every bound at least a decade above the limit), pooled the set is (at least a decade below).  The CPU test runs it on the oracle's
# latents, the GPU test on codec.embed_records' latents under the same uniforms; both add the SAME noise.  A single image is held to BOTH of its bounds: Hoeffding's
# for a set of one (what `trace_sets_keyed` reports) and the exact binomial tail of `trace_latents_keyed` (what a caller runs today).  With these seeds sigma 12.0
# meets the first (lowest single bound -4.82) but not the second (-5.98, inside the decade above the limit); so do 12.5 (-5.56) and 13.0 (-5.08).  13.5 is the first
# value of the 0.5 grid that meets both: single bounds from -4.69 (exact) / -3.57 (Hoeffding) upwards, the pooled bound -35.65.
E2E = dict(seed=4271, U=1000, B=16, shape=(4, 32, 32), msg_bytes=32, sigma=13.5, fpr=1e-6, owner=137, other=612)


def e2e_setup():
    """-> (records [(key, nonce, message)] x U, codewords uint8 [U, n / 8], uniforms float64 [2 B, n], noise float32 torch [2 B, n] of unit variance)"""
    import torch
    rng = np.random.default_rng(E2E["seed"])
    U, B, mb, n = E2E["U"], E2E["B"], E2E["msg_bytes"], int(np.prod(E2E["shape"]))
    recs = [(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8)), bytes(rng.integers(0, 256, mb, dtype=np.uint8)))
            for _ in range(U)]
    cw = np.stack([np.packbits(O.cipher_bits(m, k, nn, n)) for k, nn, m in recs])
    u = rng.uniform(0.0, 1.0, (2 * B, n))
    noise = torch.randn(2 * B, n, generator=torch.Generator().manual_seed(E2E["seed"]))
    return recs, cw, u, noise


def e2e_oracle_latents(recs, u, owners):
    """float32 [len(owners), n]: image b under record owners[b], by the oracle's embed"""
    return np.stack([O.embed_latent(recs[o][2], recs[o][0], recs[o][1], u[b], E2E["shape"]).reshape(-1) for b, o in enumerate(owners)]).astype(np.float32)


def held(z, noise):
    """the attacked latents as both sides see them: float32 torch, z + sigma noise brought back to unit variance, as inverted latents are (signs and RMS-scaled
    levels do not depend on the scale, and no element then reaches 8.2924, for which the reference raises)"""
    import torch
    return (torch.from_numpy(np.asarray(z, dtype=np.float32)).reshape(len(z), -1) + E2E["sigma"] * noise[:len(z)]) / (1.0 + E2E["sigma"] ** 2) ** 0.5
