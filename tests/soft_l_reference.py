"""NumPy restatement of the soft-decision vote for multi-bit windows (`codec.extract_soft_l` / gsw_extract_soft_l and `codec.level_pack_l` /
gsw_level_pack_l): the window y, the level of every cipher bit, score, wsum, wsq, bits, flags and the packed rows from the
latents, the keystream bytes and the thresholds.  Plain float64 arithmetic and compares on `codec.quant_thresholds(l)`; shares no code with the
device path; a plain module, no pytest plugin."""
import numpy as np
import torch

import gs_oracle as O

SAT = 8.292361075813597          # norm.cdf(z) == 1.0 from here on: the window is all ones and the image is flagged
FLAG_SATURATED, FLAG_NAN = 1, 2


def boundaries(l: int) -> np.ndarray:
    """T_1 .. T_(2^l - 1) as float64, at index 1 .. 2^l - 1 (index 0 and 2^l are unused)"""
    from gswm_amd import codec
    T = codec.quant_thresholds(l)
    assert T.dtype == np.float64 and T.shape == ((1 << l) - 1,)
    return np.concatenate([[np.nan], T, [np.nan]])


def widen64(t: torch.Tensor) -> np.ndarray:
    """a tensor [B, ...] of a supported dtype as float64 [B, n]: exact for fp16, bf16, fp32 and fp64"""
    return t.detach().cpu().reshape(t.shape[0], -1).to(torch.float64).numpy()


def windows(Z: np.ndarray, l: int):
    """y = #{ j : Z >= T_j } per element (a NaN gives 0) and the image's flags"""
    T = boundaries(l)[1:-1]
    with np.errstate(invalid="ignore"):
        y = (Z[:, None] >= T[None, :]).sum(axis=1).astype(np.int64)
        flags = (FLAG_SATURATED if (Z >= SAT).any() else 0) | (FLAG_NAN if np.isnan(Z).any() else 0)
    return y, flags


def levels_of(Z: np.ndarray, y: np.ndarray, thr: np.ndarray, l: int) -> np.ndarray:
    """level(e, w) as int64 [n, l].  Z float64 [n], y its windows, thr float32 [l, levels]."""
    assert Z.dtype == np.float64 and thr.dtype == np.float32 and thr.shape[0] == l
    T = boundaries(l)
    full = 1 << l
    out = np.zeros((Z.size, l), dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for w in range(l):
            s = 1 << (l - 1 - w)
            a = (y // s) * s
            c = a + s
            t = thr[w].astype(np.float64)                              # [levels]
            Ta = np.where(a == 0, 0.0, T[np.clip(a, 1, full - 1)])
            Tc = np.where(c == full, 0.0, T[np.clip(c, 1, full - 1)])
            lower = (a == 0)[:, None] | (Z[:, None] >= (Ta[:, None] + t[None, :]))
            upper = (c == full)[:, None] | (Z[:, None] <= (Tc[:, None] - t[None, :]))
            ok = lower & upper & ~np.isnan(t)[None, :] & ~np.isnan(Z)[:, None]
            out[:, w] = ok.sum(axis=1)
    return out


def window_bits(y: np.ndarray, l: int) -> np.ndarray:
    """the n l cipher-order bits of the windows: bit e l + w = bit (l - 1 - w) of y_e"""
    return ((y[:, None] >> (l - 1 - np.arange(l))[None, :]) & 1).reshape(-1)


def soft_vote(Z: np.ndarray, ks: np.ndarray, thr: np.ndarray, msg_bits: int, l: int) -> dict:
    """One image.  Z: float64 [n], ks: uint8 [n l / 8] keystream bytes, thr: float32 [l, levels]."""
    n, M = Z.size, int(msg_bits)
    Nb = n * l
    assert n % 8 == 0 and Nb % M == 0 and ks.size * 8 == Nb
    y, flags = windows(Z, l)
    p = window_bits(y, l) ^ np.unpackbits(np.asarray(ks, dtype=np.uint8)).astype(np.int64)
    lv = levels_of(Z, y, thr, l).reshape(-1)
    score = (lv * (2 * p - 1)).reshape(Nb // M, M).sum(axis=0)
    return {"score": score, "wsum": lv.reshape(Nb // M, M).sum(axis=0), "wsq": int((lv * lv).sum()),
            "bits": np.packbits((score > 0).astype(np.uint8)), "flags": flags}


def soft_vote_batch(Z: np.ndarray, records, thr: np.ndarray, msg_bytes: int, l: int) -> dict:
    """Z [B, n] (`widen64`), records: [(key, nonce, msg)] per image, thr float32 [l, levels] or [B, l, levels] -> the six outputs stacked"""
    B, n = Z.shape
    out = {k: [] for k in ("score", "wsum", "wsq", "bits", "flags", "matches")}
    for b in range(B):
        key, nonce, msg = records[b]
        ks = np.frombuffer(O.chacha20_keystream(key, nonce, n * l // 8), dtype=np.uint8)
        r = soft_vote(Z[b], ks, thr if thr.ndim == 2 else thr[b], 8 * msg_bytes, l)
        r["matches"] = 8 * msg_bytes - int(np.unpackbits(r["bits"] ^ np.frombuffer(msg, dtype=np.uint8)).sum())
        for k in out:
            out[k].append(r[k])
    return {k: np.stack([np.asarray(v) for v in vs]) for k, vs in out.items()}


def level_rows(Z: np.ndarray, thr: np.ndarray, l: int) -> dict:
    """Z [B, n], thr [l, levels] or [B, l, levels] -> signs uint8 [B, n l / 8], planes uint8 [B, P, n l / 8], wsum, wsq, flags [B]"""
    B, n = Z.shape
    levels = thr.shape[-1]
    P = int(levels).bit_length()
    out = {k: [] for k in ("signs", "planes", "wsum", "wsq", "flags")}
    for b in range(B):
        y, flags = windows(Z[b], l)
        lv = levels_of(Z[b], y, thr if thr.ndim == 2 else thr[b], l).reshape(-1)
        out["signs"].append(np.packbits(window_bits(y, l).astype(np.uint8)))
        out["planes"].append(np.stack([np.packbits(((lv >> k) & 1).astype(np.uint8)) for k in range(P)]))
        out["wsum"].append(int(lv.sum()))
        out["wsq"].append(int((lv * lv).sum()))
        out["flags"].append(flags)
    return {k: np.stack([np.asarray(v) for v in vs]) for k, vs in out.items()}


def hard_counts(Z: np.ndarray, ks: np.ndarray, msg_bits: int, l: int) -> np.ndarray:
    """the l-bit sign vote's counts: how many of the copies of message bit t decrypt to 1"""
    y, _ = windows(Z, l)
    p = window_bits(y, l) ^ np.unpackbits(np.asarray(ks, dtype=np.uint8)).astype(np.int64)
    return p.reshape(-1, int(msg_bits)).sum(axis=0)


def window_thresholds(Z: np.ndarray, l: int, levels: int = 15, clip: float = 2.5) -> np.ndarray:
    """float64 restatement of `soft.window_thresholds`: [B, l, levels]"""
    T = boundaries(l)
    fin = np.isfinite(Z)
    rms = np.sqrt(np.where(fin, Z * Z, 0.0).sum(axis=1) / np.maximum(fin.sum(axis=1), 1))
    steps = (np.arange(1, levels + 1) - 0.5) / levels
    out = np.zeros((Z.shape[0], l, levels))
    for w in range(l):
        s = 1 << (l - 1 - w)
        flips = [T[i] for i in range(s, 1 << l, s)]
        c = clip * rms
        if w > 0:
            c = np.minimum(c, max(b - a for a, b in zip(flips, flips[1:])) / 2.0)
        out[:, w, :] = c[:, None] * steps[None, :]
    return out
