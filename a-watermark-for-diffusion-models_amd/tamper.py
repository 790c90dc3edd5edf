"""Localising edits: which parts of an image still carry the watermark, and a vote that listens to those parts.

Every tile x tile block of lattice elements (all C channels of it) carries n_t = C tile^2 l cipher bits, each of which can be compared with
a known codeword.  `codec.tile_agreement` counts the agreeing bits per tile in one launch; this module holds what is made of the counts.

Map (`tamper_map`, `TraceResult.tamper`).  Against a message that is known independently of the image (a registry record, the
`--original_message_hex` of extract) a tile whose content is independent of the key -- erased, pasted over, cropped to black -- has
agree ~ Bin(n_t, 1/2) EXACTLY, so `trace.log10_p_soft(2 agree - n_t, n_t)` is its tail and a tile is called `intact` when its count reaches
`tile_threshold(n_t, n_tiles, fpr)`: the watermark's presence in that tile is proven at rate fpr over the whole map (Bonferroni over the
tiles).  A tile that is not `intact` is not proven edited: it only carries no proof.  Against a message decoded from the same image the
counts are biased upwards (the vote picked the message that agrees most); such maps are labelled `decoded` and carry no p-values.

Weighted vote (`extract_robust`).  The reference's vote gives a destroyed region full weight and pure noise.  `codec.vote_tiled` weights each
vote by its tile, `default_weights` turns a map into weights -- max(0, 2 agree - n_t - isqrt(n_t)): the tile's excess agreement over one
standard deviation of the null, an exact integer that needs no threshold -- and the decode alternates: plain vote, map against the
decoded message, weights, weighted vote.  The weighted score is selected on the data and is NOT a test statistic: attribution
(`trace`) keeps the unweighted p-values.

With levels (`extract_robust_soft`).  The same alternation with every cipher bit voting at its reliability level (`soft`) times the weight of its tile,
all rounds in ONE launch (`codec.decode_robust`, csrc/gswm_tamper.hip): a tile's weight is `soft_weights` = max(0, excess - isqrt(wsq)), its
level-weighted excess agreement over one standard deviation of its null, which is `default_weights` at unit levels.  DESIGN.md section 4.24.

Everything that runs per lattice bit is a HIP kernel (csrc/gswm_tamper.hip); the host sees [th, tw] counts.  DESIGN.md section 4.14.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from fractions import Fraction
from typing import List, NamedTuple, Optional, Tuple, Union

import numpy as np

from . import codec
from . import trace as T

SOURCES = ("registry", "message", "decoded")


# ===================================================================================================================== statistics
def tile_threshold(n_t: int, n_tiles: int, fpr: float) -> int:
    """The smallest k with P[Bin(n_t, 1/2) >= k] <= fpr / n_tiles, exactly (integer tails, `fpr` taken as the rational number the float
    is); n_t + 1 when even agree == n_t is more likely than that: no count then proves anything."""
    n_t, n_tiles = int(n_t), int(n_tiles)
    if n_t < 1 or n_tiles < 1:
        raise ValueError("n_t and n_tiles must be positive")
    if not 0.0 < float(fpr) <= 1.0:
        raise ValueError("fpr must be in (0, 1]")
    q = Fraction(float(fpr)) / n_tiles
    bound = (q.numerator << n_t) // q.denominator           # tail <= bound  <=>  tail / 2^n_t <= q, for integer tails
    lo, hi = 0, n_t + 1                                      # the tail falls as k grows: bisect for the first k that meets the bound
    while lo < hi:
        mid = (lo + hi) // 2
        if T._binomial_tail(n_t, mid) <= bound:
            hi = mid
        else:
            lo = mid + 1
    return lo


def weight_slack(n_t: int) -> int:
    """isqrt(n_t): one standard deviation of 2 agree - n_t under the null"""
    return math.isqrt(int(n_t))


def default_weights(agree, n_t: int):
    """max(0, 2 agree - n_t - isqrt(n_t)) as uint16 (at most n_t <= 16384), for a torch tensor (stays on its device) or anything NumPy reads"""
    n_t = int(n_t)
    if not 1 <= n_t <= 16384:
        raise ValueError("n_t must be in 1..16384")
    off = n_t + weight_slack(n_t)
    try:
        import torch
    except ImportError:                                      # pragma: no cover
        torch = None
    if torch is not None and isinstance(agree, torch.Tensor):
        return (2 * agree.to(torch.int32) - off).clamp_(min=0).to(torch.int16).view(torch.uint16)      # <= 16384: the int16 bits are the uint16's
    return np.maximum(2 * np.asarray(agree).astype(np.int64) - off, 0).astype(np.uint16)


# ===================================================================================================================== the map
@dataclass
class TamperMap:
    agree: np.ndarray                    # int32 [th, tw]: bits of the tile equal to the codeword
    n_t: int                             # bits per tile, C tile^2 l
    tile: int                            # tile edge in lattice elements
    intact: np.ndarray                   # bool [th, tw]: agree >= tile_threshold(n_t, th tw, fpr)
    log10_p: Optional[np.ndarray]        # float64 [th, tw]: log10 P[Bin(n_t, 1/2) >= agree]; None when source == "decoded"
    source: str                          # "registry" / "message": the message was known independently of the image; "decoded": it was not

    @property
    def n_intact(self) -> int:
        return int(self.intact.sum())

    @property
    def n_tiles(self) -> int:
        return int(self.intact.size)


def make_map(agree, n_t: int, tile: int, fpr: float = 1e-6, source: str = "message") -> TamperMap:
    """One image's [th, tw] counts -> TamperMap"""
    if source not in SOURCES:
        raise ValueError(f"source must be one of {SOURCES}")
    a = np.ascontiguousarray(np.asarray(agree), dtype=np.int32)
    if a.ndim != 2:
        raise ValueError("agree must be the [th, tw] counts of one image")
    intact = a >= tile_threshold(n_t, a.size, fpr)
    lp = None
    if source != "decoded":
        tails = {int(v): T.log10_p_soft(2 * int(v) - n_t, n_t) for v in np.unique(a)}
        lp = np.vectorize(tails.__getitem__, otypes=[np.float64])(a)
    return TamperMap(a, int(n_t), int(tile), intact, lp, source)


def _lattice(latents) -> Tuple[int, int, int]:
    if latents.dim() != 4:
        raise ValueError(f"latents must be [B, C, h, w] (got {tuple(latents.shape)}): the tiles are cut from the last two dimensions")
    return tuple(int(s) for s in latents.shape[1:])


def keys_tensor(records, device):
    """[(key, nonce16)] -> uint8 [B, 48] on the device: the per-image keys operand of `codec.tile_agreement` / `codec.vote_tiled`"""
    import torch
    for key, nonce in records:
        codec._check_key_nonce(key, nonce)
    rows = np.frombuffer(b"".join(k + n for k, n in records), dtype=np.uint8).reshape(len(records), codec.KEYED_RECORD_HEAD)
    return torch.from_numpy(rows.copy()).to(device)


def _message_rows(messages, msg_bits: int, device):
    import torch
    mb = msg_bits // 8
    rows = []
    for m in messages:
        m = bytes(m)
        if not m or mb % len(m):
            raise ValueError(f"a message of {len(m)} bytes does not tile {msg_bits} bits")
        rows.append(m * (mb // len(m)))
    return torch.from_numpy(np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), mb).copy()).to(device)


def _flag_error(flag: int) -> Optional[ValueError]:
    from . import _native as N
    if flag & N.GSW_FLAG_NAN:
        return ValueError("cannot convert float NaN to integer")
    if flag & N.GSW_FLAG_SATURATED:
        return ValueError("invalid literal for int() with base 2")
    return None


def tamper_map(latents, key: bytes, nonce: bytes, message_bytes: bytes, *, l: int = 1, tile: int = 8, fpr: float = 1e-6,
               message_length: Optional[int] = None) -> List[Union[TamperMap, ValueError]]:
    """latents [B, C, h, w] on the device, all under one key, against ONE message known independently of the images -> a TamperMap per
    image (source "message"), or the ValueError the reference raises for that image (a saturated / NaN latent), as `trace.trace_latents`.
    message_length: bits the message is repeated to before it is tiled over the lattice (default: its own length).
    One quantise-and-pack launch, one map launch; the host receives the counts."""
    shape = _lattice(latents)
    z = latents.contiguous()
    B = z.shape[0]
    M = 8 * len(message_bytes) if message_length is None else int(message_length)
    l = codec.check_window(l)
    codec.vote_copies(shape[0] * shape[1] * shape[2], M, l)
    packed, flags = codec.quant_pack(z, l)
    agree = codec.tile_agreement(packed, keys_tensor([(key, nonce)] * B, z.device), _message_rows([message_bytes] * B, M, z.device), M, shape, l, tile)
    agree_h, flags_h = agree.cpu().numpy(), flags.cpu().numpy()
    n_t = shape[0] * tile * tile * l
    return [_flag_error(int(flags_h[b])) or make_map(agree_h[b], n_t, tile, fpr, "message") for b in range(B)]


# ===================================================================================================================== the vote
def extract_robust(latents, key: bytes, nonce: bytes, message_length: int, *, l: int = 1, tile: int = 8, iters: int = 2):
    """Decode latents [B, C, h, w] with the tile-weighted vote: d <- the plain vote; `iters` times: map against d, `default_weights`,
    d <- weighted vote.  iters = 0 is the plain vote (`codec.extract_batch`'s bits).

    Returns (bits uint8 [B, M / 8], flags int32 [B], score int32 [B, M], wsum int32 [B, M], agree int32 [B, th, tw]), all on the device:
    bits / flags as `extract_batch`, score and wsum of the LAST vote, agree the map against the returned bits (a `decoded` map: biased
    upwards, no p-values).  One quantise-and-pack launch, then iters + 1 votes and iters + 1 maps; nothing visits the host in between."""
    import torch
    shape = _lattice(latents)
    iters = int(iters)
    if iters < 0:
        raise ValueError("iters must be >= 0")
    codec._check_key_nonce(key, nonce)
    l = codec.check_window(l)
    M = int(message_length)
    codec.vote_copies(shape[0] * shape[1] * shape[2], M, l)
    z = latents.contiguous()
    B = z.shape[0]
    packed, flags = codec.quant_pack(z, l)
    keys = keys_tensor([(key, nonce)] * B, z.device)
    th, tw = shape[1] // int(tile), shape[2] // int(tile)
    n_t = shape[0] * int(tile) * int(tile) * l
    ones = torch.ones((B, max(th, 1), max(tw, 1)), dtype=torch.int16, device=z.device).view(torch.uint16)
    bits, score, wsum = codec.vote_tiled(packed, keys, ones, M, shape, l, tile)
    agree = codec.tile_agreement(packed, keys, bits, M, shape, l, tile)
    for _ in range(iters):
        bits, score, wsum = codec.vote_tiled(packed, keys, default_weights(agree, n_t), M, shape, l, tile)
        agree = codec.tile_agreement(packed, keys, bits, M, shape, l, tile)
    return bits, flags, score, wsum, agree


def soft_weights(excess, wsq):
    """max(0, excess - isqrt(wsq)) as int32: the weight rule of `codec.decode_robust`, a tile's level-weighted excess agreement over one
    standard deviation of its null, for torch tensors (stays on their device) or anything NumPy reads.  With unit levels excess = 2 agree - n_t
    and wsq = n_t: `default_weights(agree, n_t)`.  wsq must be in 0..2^31 - 1; the square root is the exact floor."""
    try:
        import torch
    except ImportError:                                      # pragma: no cover
        torch = None
    if torch is not None and isinstance(excess, torch.Tensor):
        q = torch.as_tensor(wsq, device=excess.device).to(torch.int64)
        if bool(((q < 0) | (q > 2**31 - 1)).any()):
            raise ValueError("wsq must be in 0..2^31 - 1")
        r = q.to(torch.float64).sqrt().to(torch.int64)       # exact below 2^52; the two corrections keep it so whatever sqrt rounds to
        r = r - (r * r > q).to(torch.int64)
        r = r + ((r + 1) * (r + 1) <= q).to(torch.int64)
        return (excess.to(torch.int64) - r).clamp_(min=0).to(torch.int32)
    q = np.asarray(wsq).astype(np.int64)
    if ((q < 0) | (q > 2**31 - 1)).any():
        raise ValueError("wsq must be in 0..2^31 - 1")
    r = np.sqrt(q.astype(np.float64)).astype(np.int64)
    r = r - (r * r > q)
    r = r + ((r + 1) * (r + 1) <= q)
    return np.maximum(np.asarray(excess).astype(np.int64) - r, 0).astype(np.int32)


class RobustSoftVote(NamedTuple):
    """What `extract_robust_soft` returns, all on the latents' device: `codec.RobustVote`'s fields of the last round, and the packer's flags"""
    bits: "torch.Tensor"      # uint8 [B, M / 8]
    score: "torch.Tensor"     # int32 [B, M]
    wsum: "torch.Tensor"      # int32 [B, M]
    excess: "torch.Tensor"    # int32 [B, th, tw]
    wsq: "torch.Tensor"       # int32 [B, th, tw]
    weights: "torch.Tensor"   # int32 [B, th, tw]
    flags: "torch.Tensor"     # int32 [B], GSW_FLAG_*, as `extract_batch`


def extract_robust_soft(latents, key: bytes, nonce: bytes, message_length: int, *, l: int = 1, tile: int = 8, iters: int = 2, levels: int = 15,
                        clip: float = 2.5, thresholds=None, sign_rounds: int = 1) -> RobustSoftVote:
    """Decode latents [B, C, h, w] with tile weights AND reliability levels, in two launches: `codec.level_pack` / `level_pack_l` (the row and the
    level planes; the table `soft`'s default for this l when `thresholds` is None) and `codec.decode_robust` (all `iters` + 1 rounds).
    sign_rounds = 1 (default) takes the first round at unit levels: a pasted region louder than the watermarked rest gets the top levels and
    would wreck a first vote that listens to them; sign_rounds = 0 lets the levels count from the start, which is stronger where the damage is
    quiet.  levels = 0 packs with `codec.quant_pack` and passes no planes: the two-launch form of `extract_robust`.
    thresholds: float32 [levels] / [B, levels] (l = 1) or [l, levels] / [B, l, levels] on the latents' device; its own width replaces `levels`."""
    from . import soft
    shape = _lattice(latents)
    codec._check_key_nonce(key, nonce)
    l = codec.check_window(l)
    M = int(message_length)
    codec.vote_copies(shape[0] * shape[1] * shape[2], M, l)
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 0 <= int(levels) <= codec.SOFT_MAX_LEVELS:
        raise ValueError(f"levels must be an int in 0..{codec.SOFT_MAX_LEVELS} (0: unit levels), got {levels!r}")
    iters = codec._small_int(iters, "iters", 0, codec.ROBUST_MAX_ITERS)
    sign_rounds = codec._small_int(sign_rounds, "sign_rounds", 0, 1)
    if int(levels) == 0 and thresholds is not None:
        raise ValueError("levels = 0 votes at unit levels and takes no thresholds")
    z = latents.contiguous()
    keys = keys_tensor([(key, nonce)] * z.shape[0], z.device)
    if int(levels) == 0:
        signs, flags = codec.quant_pack(z, l)
        planes = None
    else:
        table = soft._default_table(z, l, int(levels), clip) if thresholds is None else thresholds.to(z.device)
        rows = codec.level_pack(z, table) if l == 1 else codec.level_pack_l(z, table, l)
        signs, planes, flags = rows.signs, rows.planes, rows.flags
    v = codec.decode_robust(signs, planes, keys, M, shape, l, tile, iters, sign_rounds)
    return RobustSoftVote(v.bits, v.score, v.wsum, v.excess, v.wsq, v.weights, flags)


# ===================================================================================================================== files
def save_map(tm: TamperMap, path_stem: str, image_size=None) -> Tuple[str, str]:
    """Write `<stem>.tamper.npy` (the int32 counts) and `<stem>.tamper.png` (8-bit grey, one square of 8 tile pixels per tile -- a lattice
    element is 8 x 8 pixels of the image -- 255 where intact, 0 elsewhere).  image_size = (width, height) of the image the map belongs to:
    when it differs from the map's own size the picture is resampled (nearest) to it.  Returns the two paths."""
    from PIL import Image
    npy, png = f"{path_stem}.tamper.npy", f"{path_stem}.tamper.png"
    d = os.path.dirname(npy)
    if d:
        os.makedirs(d, exist_ok=True)
    np.save(npy, np.ascontiguousarray(tm.agree, dtype=np.int32))
    px = 8 * int(tm.tile)
    img = Image.fromarray(np.kron(np.where(tm.intact, 255, 0).astype(np.uint8), np.ones((px, px), dtype=np.uint8)))
    if image_size is not None and tuple(int(s) for s in image_size) != img.size:
        img = img.resize(tuple(int(s) for s in image_size), Image.NEAREST)
    img.save(png)
    return npy, png


def map_stem(directory: str, image_path: str) -> str:
    """<directory>/<image file name without its extension>"""
    return os.path.join(directory, os.path.splitext(os.path.basename(image_path))[0])
