"""NumPy restatement of the reliability levels of multi-bit windows (l = 2, 4) through the alignment searches (`codec.level_rows_align_l`,
`codec.level_counts_align_l`, `align.search_keys_soft_l`, `detect.detect_latents_aligned_soft_l`, `trace.trace_latents_aligned_soft_l`,
`trace.trace_latents_keyed_aligned_soft_l`): the n l window bits and the n l levels of an image are reshaped to (C, H, W, l), the window
axis is moved out of the way, the lattice is flipped / turned / rolled with NumPy's own array functions (`align_reference.apply_np`) and the values are laid
out again -- the l values of an element travel with it.  Everything after that is the l = 1 restatement on rows of n l bits
(`key_search_soft_reference`, `trace_align_soft_reference`, `trace_align_reference`).  Shares no code with the device path or with `align.py` / `trace.py` /
`detect.py`; the statistics and the threshold tables are passed in by the caller.  A plain module, no pytest plugin."""
import numpy as np

import align_reference as AR
import key_search_reference as R
import key_search_soft_reference as KS
import soft_l_reference as SL
import trace_align_reference as TR
import trace_align_soft_reference as TS

INT32_MIN = AR.INT32_MIN


def aligned(values: np.ndarray, shape, l: int, aligns) -> np.ndarray:
    """per-cipher-bit values [B, n l] (window bits, levels) -> [B, A, n l]: every alignment of the image's (C, H, W) lattice, l values per element"""
    C, H, W = shape
    v = np.moveaxis(np.asarray(values).reshape(-1, C, H, W, l), -1, 1)             # [B, l, C, H, W]
    out = []
    for a in aligns:
        t = np.moveaxis(AR.apply_np(v, a), 1, -1)                                   # [B, C, H', W', l]
        out.append(np.ascontiguousarray(t).reshape(v.shape[0], -1))
    return np.stack(out, axis=1)


def aligned_rows(signs: np.ndarray, lv: np.ndarray, shape, l: int, aligns):
    """signs uint8 [B, n l / 8], lv int [B, n l] -> (uint8 [B, A, n l / 8], int64 [B, A, n l])"""
    s = np.packbits(aligned(np.unpackbits(signs, axis=1), shape, l, aligns).astype(np.uint8), axis=2)
    return s, aligned(lv, shape, l, aligns).astype(np.int64)


def level_rows_align_l(signs: np.ndarray, planes: np.ndarray, shape, l: int, aligns):
    """signs uint8 [B, n l / 8], planes uint8 [B, P, n l / 8] -> (uint8 [B, A, n l / 8], uint8 [B, A, P, n l / 8]): the levels travel as numbers, not as planes"""
    P = planes.shape[1]
    s, lv = aligned_rows(signs, KS.levels_of_planes(planes), shape, l, aligns)
    return s, np.stack([KS.planes_of_levels(lv[:, a], P) for a in range(lv.shape[1])], axis=1)


def level_counts_align_l(signs: np.ndarray, lv: np.ndarray, shape, l: int, aligns, ks_row: np.ndarray, M: int):
    """-> (score, wsum) int64 [B, A, M] over the n l cipher positions: score[b, a, t] = sum over p = t (mod M) of level_p (2 d_p - 1), wsum the same of level_p"""
    s, w = aligned_rows(signs, lv, shape, l, aligns)
    B, A, nb = w.shape
    score = np.stack([KS.margins(s[:, a], w[:, a], ks_row, M // 8) for a in range(A)], axis=1)
    return score, w.reshape(B, A, nb // M, M).sum(axis=2)


def rows_of(z, thr: np.ndarray, l: int):
    """latents (a torch tensor [B, ...]) and float32 tables [l, levels] or [B, l, levels] -> (signs uint8 [B, n l / 8], levels int64 [B, n l], flags [B])"""
    r = SL.level_rows(SL.widen64(z), np.asarray(thr, dtype=np.float32), l)
    return r["signs"], KS.levels_of_planes(r["planes"]), r["flags"]


def key_stats(signs, lv, shape, l: int, aligns, ks: np.ndarray, msg_bytes: int) -> np.ndarray:
    """S[b, a, u]: the level-weighted blind statistic of image b under alignment a and key u, int64"""
    s, w = aligned_rows(signs, lv, shape, l, aligns)
    return np.stack([KS.stats(s[:, a], w[:, a], ks, msg_bytes) for a in range(s.shape[1])], axis=1)


def shared_search(z, thr, l: int, aligns, ks_row: np.ndarray, registry: np.ndarray):
    """-> (score [B, A, M], S [B, A, U], wsq [B]) of the shared-key level-weighted search at l"""
    signs, lv, _ = rows_of(z, thr, l)
    score, _ = level_counts_align_l(signs, lv, tuple(z.shape[1:]), l, aligns, ks_row, registry.shape[1] * 8)
    return score, TS.shared_scores(score, registry), (lv * lv).sum(axis=1)


def keyed_search(z, thr, l: int, aligns, codewords: np.ndarray):
    """-> (S [B, A, U], wsq [B]) of the keyed level-weighted search at l; codewords uint8 [U, n l / 8] (`trace_align_reference.codewords`)"""
    signs, lv, _ = rows_of(z, thr, l)
    s, w = aligned_rows(signs, lv, tuple(z.shape[1:]), l, aligns)
    return TS.keyed_scores(s, w, codewords), (lv * lv).sum(axis=1)


merge = TR.merge
trace_host = TS.trace_host


def detect_host(z, thr, l: int, aligns, ks: np.ndarray, msg_bytes: int, log10_p_any):
    """The restatement of detect_latents_aligned_soft_l(k=1): [(key index, alignment index, stat, Bonferroni bound over K A of the Chernoff bound given the
    levels under that alignment, soft-voted message under that key on the aligned image)]"""
    shape = tuple(z.shape[1:])
    signs, lv, _ = rows_of(z, thr, l)
    key, al, st = AR.merge(key_stats(signs, lv, shape, l, aligns, ks, msg_bytes), 1)
    M = 8 * msg_bytes
    out = []
    for b in range(signs.shape[0]):
        u, a, s = int(key[b, 0]), int(al[b, 0]), int(st[b, 0])
        s_a, w_a = aligned_rows(signs[b:b + 1], lv[b:b + 1], shape, l, [aligns[a]])
        out.append((u, a, s, log10_p_any(KS.log10_bound(s, w_a[0, 0], M), ks.shape[0] * len(aligns)), KS.voted_message(s_a[0, 0], w_a[0, 0], ks[u], msg_bytes)))
    return out


# ---- the sign searches at l, for the comparison of item 7: the quantised rows of the same latents through the same alignments
def quant_rows(z, l: int) -> np.ndarray:
    Z = SL.widen64(z)
    return np.stack([np.packbits(SL.window_bits(SL.windows(Z[b], l)[0], l).astype(np.uint8)) for b in range(Z.shape[0])])


def sign_detect_host(z, l: int, aligns, ks: np.ndarray, msg_bytes: int, log10_p_blind, log10_p_any):
    """detect_latents(align=, l=) restated: [(key, alignment index, stat, bound)]"""
    rows = quant_rows(z, l)
    key, al, st = AR.search_keys(rows, tuple(z.shape[1:]), l, aligns, ks, msg_bytes, 1)
    M, nb = 8 * msg_bytes, rows.shape[1] * 8
    return [(int(key[b, 0]), int(al[b, 0]), int(st[b, 0]), log10_p_any(log10_p_blind(int(st[b, 0]), M, nb // M), ks.shape[0] * len(aligns))) for b in range(rows.shape[0])]


def sign_shared_host(z, l: int, aligns, ks_row, registry, log10_p_soft, log10_p_any):
    """trace_latents_aligned(l=) restated: [(record, alignment index, score, bound)]"""
    rows = quant_rows(z, l)
    M, nb = registry.shape[1] * 8, rows.shape[1] * 8
    c = TR.counts_align(rows, tuple(z.shape[1:]), l, aligns, ks_row, M)
    return TR.trace_host(TR.scores(c, nb // M, registry), nb, log10_p_soft, log10_p_any)


def sign_keyed_host(z, l: int, aligns, codewords, log10_p_soft, log10_p_any):
    """trace_latents_keyed_aligned(l=) restated: [(record, alignment index, score, bound)]"""
    rows = quant_rows(z, l)
    return TR.trace_host(TR.keyed_scores(AR.rows_align(rows, tuple(z.shape[1:]), l, aligns), codewords), rows.shape[1] * 8, log10_p_soft, log10_p_any)


# ---- end to end (item 7): six 4 x 32 x 32 latents embedded at l by the quantile rule z = ndtri((u + y) / 2^l), y the element's window of cipher bits, each under
# its own key of a 12-key ring (`align_reference.E2E`'s rows, attacks, seed and draws), attacked, plus sigma x unit Gaussian noise, fp16.  The traces plant the
# six records among 1000 (shared key: the first image's key for all, `trace_align_reference.SHARED`'s rows; keyed: `trace_align_reference.KEYED`'s rows).
E2E = dict(AR.E2E, levels=15, U=1000, shared_rows=TR.SHARED["rows"], keyed_rows=TR.KEYED["rows"])
# The noise.  tools/align_soft_l_sigma_walk.py walks sigma = 0.25, 0.5, .. 10 for the three searches at l = 2 and 4 (profiles/align_soft_l_sigma_walk.txt): on
# this grid there is NO sigma at which the level statistic names all six and the sign statistic fewer -- wherever the levels name six the signs name six too, and
# from FIRST_LOSS on the levels have lost an image while the signs hold at least as many.  So the end-to-end tests assert the exact reproduction at SIGMA, one
# grid step below the largest value at which every (search, l) still names all six by levels (at 3.75 one bound lies within 0.05 of the limit), and
# tests/test_align_soft_l_host.py holds FIRST_LOSS to "no gap".
SIGMA = 3.5
FIRST_LOSS = {("detect", 4): 4.0, ("detect", 2): 4.0, ("shared", 4): 5.25, ("shared", 2): 5.0, ("keyed", 4): 4.5, ("keyed", 2): 5.0}


def embed_l(msg: bytes, key: bytes, nonce: bytes, u: np.ndarray, l: int) -> np.ndarray:
    """float64 [n]: element e holds the window y_e = cipher bits [e l, e l + l), MSB first, cipher = keystream ^ (message repeated)"""
    from scipy.special import ndtri
    n = u.size
    cw = TR.codewords([(key, nonce, msg)], n * l)[0]
    y = (np.unpackbits(cw).reshape(n, l).astype(np.int64) << np.arange(l - 1, -1, -1)).sum(axis=1)
    return ndtri((u + y) / 2.0 ** l)


def e2e_setup(l: int):
    """-> dict(pairs, msgs, clean float64 [6, C, H, W] as embedded at l under each image's own key, shared_clean the same under pairs[0] with the registry's
    messages, noise float64 torch [6, C, H, W], blank torch fp16 [4, C, H, W], registry uint8 [U, mb], records [(key, nonce, msg)] x U, ks [K, n l / 8])"""
    import torch
    E = E2E
    rng = np.random.default_rng(E["seed"])
    n = int(np.prod(E["shape"]))
    pairs = [(bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8))) for _ in range(E["K"])]
    msgs = [bytes(rng.integers(0, 256, E["msg_bytes"], dtype=np.uint8)) for _ in E["rows"]]
    u = np.random.RandomState(E["seed"]).uniform(0, 1, (len(E["rows"]), n))
    g = torch.Generator().manual_seed(E["seed"])
    noise = torch.randn(len(msgs), *E["shape"], generator=g, dtype=torch.float64)
    blank = torch.randn(4, *E["shape"], generator=g).half()
    rr = np.random.default_rng(E["seed"] + 1)
    registry = rr.integers(0, 256, (E["U"], E["msg_bytes"]), dtype=np.uint8)
    records = [(bytes(rr.integers(0, 256, 32, dtype=np.uint8)), bytes(rr.integers(0, 256, 16, dtype=np.uint8)), bytes(rr.integers(0, 256, E["msg_bytes"], dtype=np.uint8)))
               for _ in range(E["U"])]
    for row, ring_row, msg in zip(E["keyed_rows"], E["rows"], msgs):
        records[row] = (*pairs[ring_row], msg)
    clean = np.stack([embed_l(m, *pairs[r], u[b], l).reshape(E["shape"]) for b, (r, m) in enumerate(zip(E["rows"], msgs))])
    shared_clean = np.stack([embed_l(bytes(registry[r]), *pairs[0], u[b], l).reshape(E["shape"]) for b, r in enumerate(E["shared_rows"])])
    return dict(pairs=pairs, msgs=msgs, clean=clean, shared_clean=shared_clean, noise=noise, blank=blank, registry=registry, records=records,
                ks=R.keystreams(pairs, n * l))


def attack(clean: np.ndarray, noise, sigma: float):
    """clean [6, C, H, W] -> torch fp16 [6, C, H, W]: every image through its attack, plus sigma x noise, held below the value the reference refuses"""
    import torch
    attacked = np.stack([AR.apply_np(clean[b], a) for b, a in enumerate(E2E["attacks"])])
    return TS.hold((torch.from_numpy(attacked).double() + float(sigma) * noise).half())


def restoring(aligns) -> list:
    """the index in `aligns` of the alignment that undoes each image's attack"""
    H, W = E2E["shape"][1:]
    idx = np.arange(H * W).reshape(H, W)
    out = []
    for a in E2E["attacks"]:
        t = AR.apply_np(idx, a)
        out.append(next(i for i, c in enumerate(aligns) if np.array_equal(AR.apply_np(t, c), idx)))
    return out


def e2e_host(search: str, s: dict, l: int, sigma: float, cands, cw, mods):
    """One search of item 7 on the restatement -> dict(z torch fp16 [6, C, H, W], thr float32 [6, l, levels], rows the six planted rows, levels [(index, alignment
    index, statistic, bound, ...)], signs the same of the sign search).  search: "detect" | "shared" | "keyed"; cw: `trace_align_reference.codewords` of
    s["records"] over n l bits (the keyed search reads it); mods = (soft, trace, detect) of the package, for the threshold table and the statistics alone"""
    S, T, D = mods
    mb = E2E["msg_bytes"]
    z = attack(s["shared_clean"] if search == "shared" else s["clean"], s["noise"], sigma)
    thr = S.window_thresholds(z, l, E2E["levels"]).numpy()
    if search == "detect":
        lev = detect_host(z, thr, l, cands, s["ks"], mb, T.log10_p_any)
        sig = sign_detect_host(z, l, cands, s["ks"], mb, D.log10_p_blind, T.log10_p_any)
        rows = E2E["rows"]
    elif search == "shared":
        _, Sl, wsq = shared_search(z, thr, l, cands, s["ks"][0], s["registry"])
        lev = trace_host(Sl, wsq, S.log10_p, T.log10_p_any)
        sig = sign_shared_host(z, l, cands, s["ks"][0], s["registry"], T.log10_p_soft, T.log10_p_any)
        rows = E2E["shared_rows"]
    else:
        Kl, wsq = keyed_search(z, thr, l, cands, cw)
        lev = trace_host(Kl, wsq, S.log10_p, T.log10_p_any)
        sig = sign_keyed_host(z, l, cands, cw, T.log10_p_soft, T.log10_p_any)
        rows = E2E["keyed_rows"]
    return dict(z=z, thr=thr, rows=rows, levels=lev, signs=sig)


def named(result, rows, want_al, limit: float):
    """(rightly named, wrongly named) among the images of one search's result: named = bound <= limit, rightly = the planted row AND the restoring alignment"""
    ok = [b for b, r in enumerate(result) if r[3] <= limit]
    right = [b for b in ok if result[b][0] == rows[b] and result[b][1] == want_al[b]]
    return len(right), len(ok) - len(right)
