"""NumPy restatement of the soft-decision vote (`codec.extract_soft` / gsw_extract_soft): levels, score, wsum, wsq, bits and
flags from the latents, the keystream bytes and the thresholds.  Shares no code with the device path; a plain module, no pytest plugin."""
import numpy as np
import torch

import gs_oracle as O


def widen(t: torch.Tensor) -> np.ndarray:
    """a tensor [B, ...] of a supported dtype as the array it is compared in: float32 (fp16 / bf16 / fp32, widened exactly) or float64; [B, n]"""
    t = t.detach().cpu().reshape(t.shape[0], -1)
    return t.numpy() if t.dtype == torch.float64 else t.to(torch.float32).numpy()


def levels_of(z: np.ndarray, thr: np.ndarray) -> np.ndarray:
    """level_j = #{ i : |z_j| >= thr[i] }, compared in z's own type (float32, or float64 against the thresholds widened); NaN -> 0"""
    assert z.dtype in (np.float32, np.float64) and thr.dtype == np.float32
    with np.errstate(invalid="ignore"):
        return (np.abs(z)[:, None] >= thr.astype(z.dtype)[None, :]).sum(axis=1).astype(np.int64)


def soft_vote(z: np.ndarray, ks: np.ndarray, thr: np.ndarray, msg_bits: int) -> dict:
    """One image.  z: float32 / float64 [n] (`widen`), ks: uint8 [n / 8] keystream bytes, thr: float32 [levels]."""
    n, M = z.size, int(msg_bits)
    assert n % 8 == 0 and n % M == 0 and ks.size * 8 == n
    z64 = z.astype(np.float64)
    with np.errstate(invalid="ignore"):
        q = (z64 >= O.Y1_THRESHOLD).astype(np.int64)                  # y >= 1 of int(norm.cdf(z) * 2); a NaN packs as 0
        flags = (1 if (z64 >= O.Y2_THRESHOLD).any() else 0) | (2 if np.isnan(z64).any() else 0)
    p = q ^ np.unpackbits(np.asarray(ks, dtype=np.uint8)).astype(np.int64)
    lv = levels_of(z, thr)
    score = (lv * (2 * p - 1)).reshape(n // M, M).sum(axis=0)
    return {"score": score, "wsum": lv.reshape(n // M, M).sum(axis=0), "wsq": int((lv * lv).sum()),
            "bits": np.packbits((score > 0).astype(np.uint8)), "flags": flags}


def soft_vote_batch(z: np.ndarray, records, thr: np.ndarray, msg_bytes: int) -> dict:
    """z [B, n] (`widen`), records: [(key, nonce, msg)] per image, thr float32 [levels] or [B, levels] -> the six outputs stacked, matches included"""
    B, n = z.shape
    out = {k: [] for k in ("score", "wsum", "wsq", "bits", "flags", "matches")}
    for b in range(B):
        key, nonce, msg = records[b]
        ks = np.frombuffer(O.chacha20_keystream(key, nonce, n // 8), dtype=np.uint8)
        r = soft_vote(z[b], ks, thr if thr.ndim == 1 else thr[b], 8 * msg_bytes)
        r["matches"] = 8 * msg_bytes - int(np.unpackbits(r["bits"] ^ np.frombuffer(msg, dtype=np.uint8)).sum())
        for k in out:
            out[k].append(r[k])
    return {k: np.stack([np.asarray(v) for v in vs]) for k, vs in out.items()}


def sign_thresholds() -> np.ndarray:
    """the one-level table under which the soft vote is the sign vote"""
    return np.zeros(1, dtype=np.float32)
