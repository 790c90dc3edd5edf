"""Soft-decision vote: every lattice element votes with an integer reliability level taken from its magnitude.

The embed draws z from a half-normal on the side its cipher bit selects; after sampling, VAE, attack and inversion the decoder sees roughly
z + noise.  An element far from zero is almost surely still on its side, one near zero is a coin flip -- the sign-only vote counts both the
same.  `codec.extract_soft` (gsw_extract_soft, one launch) weights element j by level_j = #{ i : |z_j| >= thresholds[i] }, an integer in
0..levels, so the result is exact in every dtype and independent of the order of summation.  This module holds the threshold tables
(`uniform_thresholds`: scaled to the image's own RMS, needs no noise estimate; `llr_thresholds`: calibrated to a known noise level), the
shared-key convenience `extract_soft` and the significance bound of a level-weighted score (`log10_p`).

Multi-bit windows (l = 2, 4): `codec.extract_soft_l` gives every cipher BIT of an element a level, the element's distance from the
nearest quantiser boundary at which that bit would have come out differently, counted against a table per window bit (`window_thresholds`);
`extract_soft_l` is the shared-key convenience, and `log10_p` bounds its score as it stands (the coins are now per cipher bit).
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import codec

MAX_LEVELS = codec.SOFT_MAX_LEVELS


def _check_table(levels, clip) -> tuple:
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 1 <= int(levels) <= MAX_LEVELS:
        raise ValueError(f"levels must be an int in 1..{MAX_LEVELS}, got {levels!r}")
    if isinstance(clip, bool) or not isinstance(clip, (int, float, np.integer, np.floating)) or not (math.isfinite(clip) and clip > 0):
        raise ValueError(f"clip must be a positive finite number, got {clip!r}")
    return int(levels), float(clip)


def uniform_thresholds(z: torch.Tensor, levels: int = 15, clip: float = 2.5) -> torch.Tensor:
    """float32 [B, levels] on z's device: per image t_i = (i - 1/2) clip rms / levels for i = 1..levels, with rms = sqrt(mean z^2) taken in
    fp32 over the image's finite elements (an image without any gets rms 0: every non-NaN element then has the top level, which is the sign
    vote).  The table spans [0, clip rms] in equal steps: |z| above clip rms counts `levels`, |z| below half a step counts nothing.  It
    scales with the image, so it needs no estimate of the noise.  A few torch ops, not a hot path."""
    levels, clip = _check_table(levels, clip)
    if z.dim() < 2 or z.shape[0] < 1:
        raise ValueError("z must be [B, ...] with at least one image")
    zf = z.detach().reshape(z.shape[0], -1).to(torch.float32)
    ok = torch.isfinite(zf)
    sq = torch.where(ok, zf * zf, torch.zeros((), dtype=torch.float32, device=zf.device)).sum(dim=1)
    rms = torch.sqrt(sq / ok.sum(dim=1).clamp(min=1).to(torch.float32))
    steps = (torch.arange(1, levels + 1, dtype=torch.float32, device=zf.device) - 0.5) * (clip / levels)
    return (rms[:, None] * steps[None, :]).contiguous()


def window_gaps(l: int) -> list:
    """g_w for w = 0 .. l-1: the largest gap between neighbouring flip boundaries of window bit w, T_(i+s) - T_i over the boundaries
    T_i = codec.quant_thresholds(l)[i-1] with s = 2**(l-1-w) dividing i; inf for w = 0, whose only flip boundary is the median."""
    T = codec.quant_thresholds(l)
    out = []
    for w in range(l):
        s = 1 << (l - 1 - w)
        flips = [float(T[i - 1]) for i in range(s, 1 << l, s)]
        out.append(max((b - a for a, b in zip(flips, flips[1:])), default=math.inf))
    return out


def window_thresholds(z: torch.Tensor, l: int, levels: int = 15, clip: float = 2.5) -> torch.Tensor:
    """float32 [B, l, levels] on z's device, the table of `codec.extract_soft_l`: per image and window bit w,
    t[w][i] = (i - 1/2) c_w / levels for i = 1..levels.  c_0 = clip rms (the first bit has one flip boundary, the median, and behaves as at
    l = 1; rms as `uniform_thresholds`); for w > 0 c_w = min(clip rms, g_w / 2), g_w = `window_gaps(l)[w]`: an element cannot be further
    than half the widest gap from both of its flip boundaries, so a wider table would leave its top levels to the two tails alone."""
    levels, clip = _check_table(levels, clip)
    l = codec.check_window(l)
    span = uniform_thresholds(z, levels, clip)                       # [B, levels]: (i - 1/2) clip rms / levels
    top = span[:, -1:] * (levels / (levels - 0.5))                    # clip rms
    steps = (torch.arange(1, levels + 1, dtype=torch.float32, device=span.device) - 0.5) / levels
    rows = [span]
    for g in window_gaps(l)[1:]:
        c = torch.clamp(top, max=g / 2.0)
        rows.append(c * steps[None, :])
    return torch.stack(rows, dim=1).contiguous()


def _log_erfc(u: float) -> float:
    """log erfc(u); past the underflow of math.erfc by the leading term of its expansion"""
    if u < 25.0:
        return math.log(math.erfc(u))
    return -u * u - math.log(u * math.sqrt(math.pi)) + math.log1p(-0.5 / (u * u))


def _llr(x: float, a: float) -> float:
    """log Phi(a x) - log Phi(-a x), Phi(y) = erfc(-y / sqrt 2) / 2"""
    u = a * x / math.sqrt(2.0)
    return _log_erfc(-u) - _log_erfc(u)


def llr_thresholds(sigma: float, levels: int = 15, clip: float = 2.5) -> torch.Tensor:
    """float32 [levels] on the host: the table calibrated to a known noise level.  For z' = z + sigma n with z half-normal on the side of
    its bit, the log-likelihood ratio of the bit given z' = x is L(x) = log Phi(a x) - log Phi(-a x), a = 1 / (sigma sqrt(1 + sigma^2)).
    L is quantised uniformly up to x_max = clip sqrt(1 + sigma^2) (clip standard deviations of z'): t_i solves
    L(t_i) = (i - 1/2) L(x_max) / levels, found by bisection.  For large sigma L is linear over the range and the table tends to
    `uniform_thresholds` of an image with rms sqrt(1 + sigma^2)."""
    levels, clip = _check_table(levels, clip)
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.integer, np.floating)) or not (math.isfinite(sigma) and sigma > 0):
        raise ValueError(f"sigma must be a positive finite number, got {sigma!r}")
    sigma = float(sigma)
    spread = math.sqrt(1.0 + sigma * sigma)
    a, x_max = 1.0 / (sigma * spread), clip * spread
    top = _llr(x_max, a)
    out = []
    for i in range(1, levels + 1):
        want = (i - 0.5) * top / levels
        lo, hi = 0.0, x_max                               # L is increasing, L(0) = 0 < want < L(x_max)
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if mid <= lo or mid >= hi:
                break
            if _llr(mid, a) < want:
                lo = mid
            else:
                hi = mid
        out.append(hi)
    return torch.tensor(out, dtype=torch.float64).to(torch.float32)


def shared_records(key: bytes, nonce: bytes, msg_bytes: int, batch: int, device) -> torch.Tensor:
    """uint8 [batch, stride] record rows key | nonce | zero message: the rows `codec.extract_soft` wants when every image shares one key"""
    codec._check_key_nonce(key, nonce)
    row = np.zeros(codec.keyed_record_stride(msg_bytes), dtype=np.uint8)
    row[:codec.KEYED_RECORD_HEAD] = np.frombuffer(bytes(key) + bytes(nonce), dtype=np.uint8)
    return torch.from_numpy(row).to(device).expand(int(batch), -1).contiguous()


def _default_table(z: torch.Tensor, l: int, levels: int, clip: float = 2.5) -> torch.Tensor:
    """The table a decoder uses when it is given none: `uniform_thresholds` at l = 1, `window_thresholds` at l = 2 and 4"""
    return uniform_thresholds(z, levels, clip) if l == 1 else window_thresholds(z, l, levels, clip)


def _extract_shared_key(z: torch.Tensor, key: bytes, nonce: bytes, message_length: int, l: int, levels: int, clip: float, thresholds) -> codec.SoftVote:
    """`extract_soft` (l = 1) and `extract_soft_l` (l = 2, 4)"""
    M = int(message_length)
    if M < 8 or M % 8 or M > 8 * codec.N.GSW_MSG_INLINE_MAX:
        raise ValueError(f"the soft vote needs a message_length that is a multiple of 8 in 8..{8 * codec.N.GSW_MSG_INLINE_MAX}, got {message_length!r}")
    thresholds = _default_table(z, l, levels, clip) if thresholds is None else thresholds.to(z.device)
    records = shared_records(key, nonce, M // 8, z.shape[0], z.device)
    vote = codec.extract_soft(z, records, M // 8, thresholds) if l == 1 else codec.extract_soft_l(z, records, M // 8, thresholds, l)
    return vote._replace(matches=None)


def extract_soft(latents: torch.Tensor, key: bytes, nonce: bytes, message_length: int, *, levels: int = 15, clip: float = 2.5,
                 thresholds: Optional[torch.Tensor] = None) -> codec.SoftVote:
    """`codec.extract_soft` for a batch under ONE key and nonce: latents [B, ...] on the device -> `codec.SoftVote` with matches = None (there
    is no message to compare with).  thresholds: float32 [levels] or [B, levels]; None: `uniform_thresholds(latents, levels, clip)`.
    message_length: a multiple of 8 up to 2048 bits; one cipher bit per element (l = 1)."""
    return _extract_shared_key(latents, key, nonce, message_length, 1, levels, clip, thresholds)


def extract_soft_l(latents: torch.Tensor, key: bytes, nonce: bytes, message_length: int, l: int, *, levels: int = 15, clip: float = 2.5,
                   thresholds: Optional[torch.Tensor] = None) -> codec.SoftVote:
    """`codec.extract_soft_l` for a batch under ONE key and nonce, as `extract_soft` is for l = 1 (to which l = 1 delegates, bit for bit).
    thresholds: float32 [l, levels] or [B, l, levels]; None: `window_thresholds(latents, l, levels, clip)`."""
    l = codec.check_window(l)
    if l == 1:
        return extract_soft(latents, key, nonce, message_length, levels=levels, clip=clip, thresholds=thresholds)
    return _extract_shared_key(latents, key, nonce, message_length, l, levels, clip, thresholds)


def log10_p(score_total, wsq) -> float:
    """Upper BOUND of log10 P[S >= score_total] for an image that is independent of the key: -s^2 / (2 wsq ln 10) for s > 0, else 0.

    score_total = sum_t (2 r_t - 1) score[t] for a fixed message r, wsq = sum_j level_j^2.  Given the levels, the decrypted bits of a
    key-independent image are independent fair coins, so S = sum_j level_j e_j with e_j = +-1 and Hoeffding's inequality gives
    P[S >= s] <= exp(-s^2 / (2 wsq)).  The bound holds conditional on |z|, hence also with thresholds chosen from |z|
    (`uniform_thresholds`).  It is a bound, NOT the exact tail: the margin statistic (`trace.log10_p_soft`) has an exact binomial tail,
    the level-weighted one has none in closed form, and Hoeffding's bound is looser than the true tail."""
    s, q = int(score_total), int(wsq)
    if s <= 0 or q <= 0:
        return 0.0
    return -(s * s) / (2.0 * q * math.log(10.0))
