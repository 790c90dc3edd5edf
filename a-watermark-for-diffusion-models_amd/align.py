"""Alignment search: detect through flips, quarter turns and lattice shifts of the image.

The keystream is tied to the lattice position, so an image that was mirrored, turned by a quarter or translated by a multiple of the VAE's 8
pixels before inversion decrypts to coin flips under its own key.  Up to border effects those attacks act on the inverted latent as the same
transform of its [H, W] planes, and there are few of them: this module enumerates the candidates (`alignments`), writes every candidate
alignment of the image's packed row in one launch (`codec.rows_align`) and hands the rows to the blind key search unchanged
(`codec.key_search_topk`), then merges per image on the device (`search_keys`).  One inversion, one quantisation, whatever the number of
candidates.

An alignment is a = (d, dy, dx), d in 0..7 and dy, dx integers; `apply(z, a)` is EXACTLY

    t = torch.flip(z, dims=(-1,)) if d & 4 else z
    t = torch.rot90(t, d & 3, dims=(-2, -1))
    t = torch.roll(t, shifts=(dy, dx), dims=(-2, -1))          # cyclic: the wrapped border votes as noise

The search reports the alignment that UNDOES the attack: `apply(attacked, found)` is the lattice as embedded.

Null law.  Under a key the image is independent of, the keystream is uniform, so the decrypted bits of ANY fixed permutation of the row are fair
coins: `detect.log10_p_blind` holds for every (key, alignment) pair, and the Bonferroni bound over the K A pairs is valid whatever the
dependence between the alignments of one image.

Reliability levels (`search_keys_soft`, `extract_aligned_soft`, `detect.detect_latents_aligned_soft`; l = 1): the same search with every lattice
element weighted by its level.  `codec.level_rows_align` writes every alignment of `codec.level_pack`'s sign row AND of its level planes in one
launch and `codec.key_search_soft_topk` scores them; the thresholds are those of the un-aligned latents, since a permutation moves an element
with its level.  The null bound (`detect.log10_p_blind_soft`) is taken given the levels UNDER the alignment: it changes which elements vote on
which message position.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import codec

Alignment = Tuple[int, int, int]
GROUPS = {"none": (0,), "flips": (0, 2, 4, 6), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}
ROWS_BUDGET_BYTES = 256 << 20           # aligned rows alive at a time in `search_keys` (the images are cut into chunks that stay below it)
SEARCH_MAX_ROWS = 65535                 # rows of one `codec.key_search_topk` launch
_INT32_MIN = -2 ** 31


# ===================================================================================================================== the model
def _check(a, H: Optional[int] = None, W: Optional[int] = None) -> Alignment:
    try:
        d, dy, dx = a
    except (TypeError, ValueError):
        raise ValueError(f"an alignment is (d, dy, dx), got {a!r}") from None
    for v in (d, dy, dx):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"an alignment is three integers, got {a!r}")
    d, dy, dx = int(d), int(dy), int(dx)
    if not 0 <= d <= 7:
        raise ValueError(f"alignment d must be in 0..7, got {d}")
    if d & 1 and H is not None and H != W:
        raise ValueError(f"an odd d (a quarter turn) needs a square lattice, got H = {H}, W = {W}")
    return d, dy, dx


def apply(z: torch.Tensor, a) -> torch.Tensor:
    """The alignment a = (d, dy, dx) of the last two dimensions of z [..., H, W] (the module docstring's three lines)"""
    if z.dim() < 2:
        raise ValueError("apply needs a [..., H, W] tensor")
    d, dy, dx = _check(a, z.shape[-2], z.shape[-1])
    t = torch.flip(z, dims=(-1,)) if d & 4 else z
    t = torch.rot90(t, d & 3, dims=(-2, -1))
    return torch.roll(t, shifts=(dy, dx), dims=(-2, -1))


def _shift_order(shift: int) -> List[int]:
    return [0] + [s for r in range(1, shift + 1) for s in (r, -r)]


def alignments(group: str, shift: int, H: int, W: int) -> List[Alignment]:
    """The candidates of a search on an [H, W] lattice, identity first: A = |group| (2 shift + 1)^2 triples.

    group: "none" (d = 0), "flips" (d in 0, 2, 4, 6: identity, half turn, the two mirrors) or "d4" (all eight; needs H == W).
    Order: d ascending within the group; for each d, dy over 0, 1, -1, 2, -2, .., shift, -shift and, for each dy, dx over the same sequence.
    2 shift < min(H, W), so that no two candidates are the same permutation."""
    if group not in GROUPS:
        raise ValueError(f"group must be one of {sorted(GROUPS)}, got {group!r}")
    if isinstance(shift, bool) or not isinstance(shift, (int, np.integer)) or shift < 0:
        raise ValueError(f"shift must be a non-negative integer, got {shift!r}")
    H, W, shift = int(H), int(W), int(shift)
    if H < 1 or W < 1:
        raise ValueError("H and W must be positive")
    if group == "d4" and H != W:
        raise ValueError(f"group 'd4' holds quarter turns and needs a square lattice, got H = {H}, W = {W}")
    if 2 * shift >= min(H, W):
        raise ValueError(f"shift {shift} must satisfy 2 shift < min(H, W) = {min(H, W)}: beyond it two candidates coincide")
    order = _shift_order(shift)
    return [(d, dy, dx) for d in GROUPS[group] for dy in order for dx in order]


def describe(a) -> str:
    """A short stable text: `identity`, `hflip+rot90 shift (1,-2)`, `rot180`, `shift (0,3)`"""
    d, dy, dx = _check(a)
    names = (["hflip"] if d & 4 else []) + ([f"rot{90 * (d & 3)}"] if d & 3 else [])
    parts = (["+".join(names)] if names else []) + ([f"shift ({dy},{dx})"] if dy or dx else [])
    return " ".join(parts) if parts else "identity"


def inverse(a, H: int, W: int) -> Alignment:
    """The alignment that undoes a on an [H, W] lattice: apply(apply(z, a), inverse(a, H, W)) == z, shifts in (-H/2, H/2] x (-W/2, W/2]"""
    a = _check(a, H, W)
    idx = torch.arange(H * W).view(H, W)
    t = apply(idx, a)
    for d in range(8):
        if d & 1 and H != W:
            continue
        u = apply(t, (d, 0, 0))
        at = int((u.reshape(-1) == 0).nonzero()[0])
        dy, dx = (-(at // W)) % H, (-(at % W)) % W
        if torch.equal(torch.roll(u, (dy, dx), (-2, -1)), idx):
            return d, dy - H if 2 * dy > H else dy, dx - W if 2 * dx > W else dx
    raise AssertionError("the eight orientations are a group")


def _as_list(aligns, H: int, W: int) -> List[Alignment]:
    out = [_check(a, H, W) for a in aligns]
    if not out:
        raise ValueError("the list of alignments is empty")
    return out


def unalign(latents: torch.Tensor, aligns: Sequence[Alignment], index) -> torch.Tensor:
    """latents [B, C, H, W] with image b put through apply(., aligns[index[b]]): what the search found, undone"""
    return torch.stack([apply(latents[b], aligns[int(i)]) for b, i in enumerate(index)]).contiguous()


# ===================================================================================================================== the search
def _merge(key: torch.Tensor, stat: torch.Tensor, align: torch.Tensor, k: int):
    """Candidates [B, n] (key -1 / stat INT32_MIN: none) -> the k best keys per image, [B, k] each: for every key its best alignment (stat
    descending, alignment ascending), then (stat descending, key ascending, alignment ascending).  Stable sorts only."""
    def take(order, *ts):
        return tuple(torch.gather(t, 1, order) for t in ts)

    order = torch.sort(align, dim=1, stable=True).indices
    key, stat, align = take(order, key, stat, align)
    order = torch.sort(stat, dim=1, descending=True, stable=True).indices
    key, stat, align = take(order, key, stat, align)
    order = torch.sort(key, dim=1, stable=True).indices
    key, stat, align = take(order, key, stat, align)                 # (key, stat descending, alignment): a key's best entry leads its run
    first = torch.ones_like(key, dtype=torch.bool)
    first[:, 1:] = key[:, 1:] != key[:, :-1]
    keep = first & (key >= 0)
    stat = torch.where(keep, stat, torch.full_like(stat, _INT32_MIN))
    order = torch.sort(stat, dim=1, descending=True, stable=True).indices[:, :k]
    key, stat, align, keep = take(order, key, stat, align, keep)
    none = torch.full_like(key, -1)
    key, align = torch.where(keep, key, none), torch.where(keep, align, none)
    if key.shape[1] < k:                                             # fewer candidates than k: pad as the searches do
        pad = (key.shape[0], k - key.shape[1])
        key, align = (torch.cat([t, t.new_full(pad, -1)], 1) for t in (key, align))
        stat = torch.cat([stat, stat.new_full(pad, _INT32_MIN)], 1)
    return key.contiguous(), align.contiguous(), stat.contiguous()


def _merge_best(key: torch.Tensor, stat: torch.Tensor, n_keys: int, stat_bits: int = 21):
    """`_merge` for k = 1, where a row's candidate IS its alignment's best key: the one entry that leads by (stat descending, key ascending, alignment
    ascending), found as the maximum of one int64 per entry -- a dozen launches instead of four sorts.  key, stat [B, A], column = alignment index.
    stat_bits: the bits of the largest statistic (21: the sign search's, at most 1 048 576 lattice bits; `search_keys_soft` passes 25 for 15 times that).
    None when the three fields do not fit 63 bits (the caller then sorts)."""
    n = key.shape[1]
    ab, kb = max(1, (n - 1).bit_length()), max(1, (int(n_keys) - 1).bit_length())
    if stat_bits + kb + ab > 62:
        return None
    pos = torch.arange(n, dtype=torch.int64, device=key.device)
    c = stat.long() * (1 << (kb + ab)) - key.long() * (1 << ab) - pos
    at = c.argmax(dim=1, keepdim=True)                               # (no two entries of a row are equal: the column is part of the value)
    return key.gather(1, at), at.int(), stat.gather(1, at)


_TABLES: dict = {}                      # (alignments, lattice, device) -> the int32 [A, 3] table on that device, checked once


def _device_table(aligns: Sequence[Alignment], shape, device) -> torch.Tensor:
    at = (tuple(aligns), tuple(int(s) for s in shape), str(device))
    t = _TABLES.get(at)
    if t is None:
        if len(_TABLES) >= 8:
            _TABLES.clear()
        t = _TABLES[at] = torch.from_numpy(codec.align_table(aligns, shape)).to(device)
    return t


def _search_chunks(B: int, per_image: int, table: torch.Tensor, keys_dev: torch.Tensor, k: int, budget_bytes: Optional[int], take, search, **merge_best):
    """The cuts and the merge of the two searches.  per_image: bytes of ONE aligned image; merge_best: `_merge_best`'s stat_bits where its default (the sign statistic's) is too few; table: the int32 [A, 3] alignments on the
    device; take(b0, b1) -> the packed operand of images b0:b1; search(operand, table[a0:a1]) -> (idx, stat) int32 [nb (a1 - a0), k] of `codec.key_search_topk` /
    `codec.key_search_soft_topk` on that operand's aligned rows, image-major."""
    A = table.shape[0]
    k = int(k)
    if not 1 <= k <= 8:
        raise ValueError("k must be in 1..8")
    budget = int(ROWS_BUDGET_BYTES if budget_bytes is None else budget_bytes)
    a_step = max(1, min(A, SEARCH_MAX_ROWS, budget // per_image))                          # alignments per launch (all of them unless one image's rows pass the budget)
    b_step = max(1, min(B, SEARCH_MAX_ROWS // a_step, budget // (a_step * per_image)))     # images per launch
    join = lambda ts: ts[0] if len(ts) == 1 else torch.cat(ts, 1)
    outs = []
    for b0 in range(0, B, b_step):
        nb = min(b_step, B - b0)
        operand = take(b0, b0 + nb)
        keys, stats = [], []
        for a0 in range(0, A, a_step):
            na = min(a_step, A - a0)
            idx, stat = search(operand, table[a0:a0 + na])
            keys.append(idx.view(nb, na * k))
            stats.append(stat.view(nb, na * k))
        best = _merge_best(join(keys), join(stats), keys_dev.shape[0], **merge_best) if k == 1 else None
        if best is None:
            als = torch.arange(A, dtype=torch.int32, device=table.device).repeat_interleave(k).expand(nb, A * k)
            best = _merge(join(keys), join(stats), als, k)
        outs.append(best)
    return outs[0] if len(outs) == 1 else tuple(torch.cat([o[i] for o in outs]) for i in range(3))


def _search_packed(packed: torch.Tensor, shape, l: int, keys_dev: torch.Tensor, msg_bytes: int, aligns: Sequence[Alignment], k: int,
                   budget_bytes: Optional[int] = None):
    """`search_keys` from the packed rows on: packed uint8 [B, rowbytes] of a [C, H, W] lattice at l bits per element"""
    shape = tuple(int(s) for s in shape)
    table = _device_table(aligns, shape, packed.device)
    B, rowbytes = packed.shape

    def take(b0, b1):
        rows_b = packed[b0:b1]
        return rows_b.clone() if rows_b.data_ptr() % 16 else rows_b

    def search(rows_b, aligns_dev):
        rows = codec._rows_align_launch(rows_b, shape, l, aligns_dev)
        return codec.key_search_topk(rows.view(-1, rowbytes), rowbytes * 8, keys_dev, msg_bytes, k=int(k))

    return _search_chunks(B, rowbytes, table, keys_dev, k, budget_bytes, take, search)


def search_keys(latents: torch.Tensor, keys_dev: torch.Tensor, msg_bytes: int, aligns: Sequence[Alignment], *, l: int = 1, k: int = 1,
                budget_bytes: Optional[int] = None):
    """The k best keys of a keyring per image over every candidate alignment: (key_idx, align_idx, stat), int32 [B, k] each, on the device.

    latents [B, C, H, W] on the device, keys_dev as `codec.key_search_topk` takes them, aligns from `alignments`.  One `codec.quant_pack`, then
    per chunk of images one `codec.rows_align` and one `codec.key_search_topk` on its [B A, rowbytes] rows, and a merge per image: every key
    keeps its best alignment, the keys are ordered by (stat descending, key index ascending, alignment index ascending) and the first k are
    returned (key -1, alignment -1, stat INT32_MIN past the keyring's end).  The images are cut so that one search sees at most 65 535 rows
    and at most `budget_bytes` (default `ROWS_BUDGET_BYTES`, 256 MiB) of aligned rows; if the rows of ONE image pass the budget its
    alignments are cut too.  The result does not depend on the cuts."""
    if latents.dim() != 4:
        raise ValueError(f"search_keys needs latents [B, C, H, W], got {tuple(latents.shape)}")
    l = codec.check_window(l)
    packed, _ = codec.quant_pack(latents.contiguous(), l)
    return _search_packed(packed, latents.shape[1:], l, keys_dev, msg_bytes, _as_list(aligns, *latents.shape[2:]), k, budget_bytes)


SOFT_STAT_BITS = 25                     # the level-weighted statistic is at most 15 x 1 048 576 < 2^24 (`_merge_best`'s stat field, with its sign)


def _search_level_rows(rows: "codec.LevelRows", shape, keys_dev: torch.Tensor, msg_bytes: int, aligns: Sequence[Alignment], k: int,
                       budget_bytes: Optional[int] = None, l: int = 1):
    """`search_keys_soft` from `codec.level_pack`'s rows on, and `search_keys_soft_l` from `codec.level_pack_l`'s at that l: `_search_packed` with 1 + P rows per
    aligned image"""
    shape = tuple(int(s) for s in shape)
    table = _device_table(aligns, shape, rows.signs.device)
    B, rowbytes = rows.signs.shape
    P = rows.planes.shape[1]

    def search(rows_b, aligns_dev):
        signs, planes = codec._level_rows_align_launch(rows_b, shape, aligns_dev, l)
        al = codec.LevelRows(signs.view(-1, rowbytes), planes.view(-1, P, rowbytes), rows_b.wsum, rows_b.wsq, rows_b.flags)   # (the search reads signs and planes alone)
        return codec.key_search_soft_topk(al, rowbytes * 8, keys_dev, msg_bytes, k=int(k))

    return _search_chunks(B, (1 + P) * rowbytes, table, keys_dev, k, budget_bytes,
                          lambda b0, b1: codec.LevelRows(*(t[b0:b1] for t in rows)), search, stat_bits=SOFT_STAT_BITS)         # an aligned image: its sign row and its P planes


def search_keys_soft(latents: torch.Tensor, keys_dev: torch.Tensor, msg_bytes: int, aligns: Sequence[Alignment], *, levels: int = 15,
                     thresholds: Optional[torch.Tensor] = None, k: int = 1, budget_bytes: Optional[int] = None):
    """`search_keys` ranked by reliability levels: (key_idx, align_idx, stat), int32 [B, k] each, on the device; stat is
    `codec.key_search_soft_topk`'s level-weighted statistic of the image under that alignment.

    latents [B, C, H, W] on the device, one cipher bit per element.  thresholds: float32 [levels] or [B, levels] as `codec.level_pack` takes
    them (`levels` is then not read); None: `soft.uniform_thresholds(latents, levels)`, computed ONCE on the un-aligned latents (an alignment
    permutes the elements, so their levels travel with them).  One `codec.level_pack`, then per chunk of images one `codec.level_rows_align` launch and one
    `codec.key_search_soft_topk` on its [B A] rows, and `search_keys`' merge per image.  The cuts are `search_keys`' with (1 + P) rows counted
    per aligned image against `budget_bytes`; the result does not depend on them."""
    if latents.dim() != 4:
        raise ValueError(f"search_keys_soft needs latents [B, C, H, W], got {tuple(latents.shape)}")
    table = _as_list(aligns, *latents.shape[2:])
    z = latents.contiguous()
    if thresholds is None:
        from . import soft as S
        thresholds = S.uniform_thresholds(z, levels)
    rows = codec.level_pack(z, thresholds)
    codec._level_rows_align_checks(rows, z.shape[1:])
    return _search_level_rows(rows, z.shape[1:], keys_dev, msg_bytes, table, k, budget_bytes)


def search_keys_soft_l(latents: torch.Tensor, keys_dev: torch.Tensor, msg_bytes: int, aligns: Sequence[Alignment], l: int, *, levels: int = 15,
                       clip: float = 2.5, thresholds: Optional[torch.Tensor] = None, k: int = 1, budget_bytes: Optional[int] = None):
    """`search_keys_soft` for multi-bit windows (l = 2 or 4): (key_idx, align_idx, stat), int32 [B, k] each, on the device; stat is
    `codec.key_search_soft_topk`'s level-weighted statistic over the n l cipher bits of the image under that alignment.

    thresholds: float32 [l, levels] or [B, l, levels] as `codec.level_pack_l` takes them (`levels` and `clip` are then not read); None:
    `soft.window_thresholds(latents, l, levels, clip)`, computed ONCE on the un-aligned latents.  One `codec.level_pack_l`, then per chunk of images one
    `codec.level_rows_align_l` launch -- the l window bits of an element and its l level bits in every plane move together -- and one
    `codec.key_search_soft_topk` on its [B A] rows with n_bits = n l, and `search_keys`' merge per image.  The cuts and the merge are `search_keys_soft`'s.
    l = 1 is refused: that is `search_keys_soft`."""
    l = codec._multi_bit_window(l, "search_keys_soft")
    if latents.dim() != 4:
        raise ValueError(f"search_keys_soft_l needs latents [B, C, H, W], got {tuple(latents.shape)}")
    table = _as_list(aligns, *latents.shape[2:])
    z = latents.contiguous()
    if thresholds is None:
        from . import soft as S
        thresholds = S.window_thresholds(z, l, levels, clip)
    rows = codec.level_pack_l(z, thresholds, l)
    codec._level_rows_align_checks(rows, z.shape[1:], l)
    return _search_level_rows(rows, z.shape[1:], keys_dev, msg_bytes, table, k, budget_bytes, l)


# ===================================================================================================================== known key
@dataclass
class AlignedExtract:
    alignment: Alignment            # the best candidate: apply(latent, alignment) is what was decoded
    align_index: int
    stat: int
    log10_p: float                  # Bonferroni bound of the blind statistic over the A candidates
    detected: bool                  # log10_p <= log10(fpr)
    bits: np.ndarray                # uint8 [message_length / 8], MSB first: `codec.extract_records` on the un-aligned latent
    flags: int                      # GSW_FLAG_* of the image


def extract_aligned(latents: torch.Tensor, key: bytes, nonce: bytes, message_length: int, aligns: Sequence[Alignment], *, l: int = 1,
                    fpr: float = 1e-6) -> List[AlignedExtract]:
    """The known-key case, a keyring of one: per image the best alignment with its bound over the A candidates and the message voted on the
    latent with that alignment applied.  latents [B, C, H, W] on the device."""
    from . import detect as D, trace as T
    codec._check_key_nonce(key, nonce)
    limit = T._log10_fpr(fpr)
    mb = D._message_bytes(message_length)
    M = 8 * mb
    l = codec.check_window(l)
    if latents.dim() != 4:
        raise ValueError(f"extract_aligned needs latents [B, C, H, W], got {tuple(latents.shape)}")
    z = latents.contiguous()
    B = z.shape[0]
    table = _as_list(aligns, *z.shape[2:])
    V = codec.vote_copies(z.numel() // max(B, 1), M, l)
    rows = torch.zeros((B, codec.keyed_record_stride(mb)), dtype=torch.uint8, device=z.device)
    rows[:, :codec.KEYED_RECORD_HEAD] = torch.from_numpy(np.frombuffer(key + nonce, dtype=np.uint8).copy()).to(z.device)
    packed, flags = codec.quant_pack(z, l)
    _, aidx, stat = _search_packed(packed, z.shape[1:], l, rows[:1], mb, table, 1)          # (a record row is a key row: bytes past 48 are ignored)
    pairs = torch.stack([aidx[:, 0], stat[:, 0]]).cpu().numpy()
    bits, _, _ = codec.extract_records(unalign(z, table, pairs[0]), rows, mb, l=l)
    bits_h, flags_h = bits.cpu().numpy(), flags.cpu().numpy()
    out = []
    for b in range(B):
        i, s = int(pairs[0, b]), int(pairs[1, b])
        p = T.log10_p_any(D.log10_p_blind(s, M, V), len(table))
        out.append(AlignedExtract(table[i], i, s, p, p <= limit, bits_h[b].copy(), int(flags_h[b])))
    return out


def extract_aligned_soft(latents: torch.Tensor, key: bytes, nonce: bytes, message_length: int, aligns: Sequence[Alignment], *, levels: int = 15,
                         fpr: float = 1e-6) -> List[AlignedExtract]:
    """`extract_aligned` ranked by reliability levels (l = 1), a keyring of one through `detect.detect_latents_aligned_soft`: per image the best
    alignment by the level-weighted statistic, its Chernoff bound given the levels under that alignment over the A candidates, and the soft vote
    (`codec.extract_soft`, the same thresholds) on the latent with that alignment applied."""
    from . import detect as D
    codec._check_key_nonce(key, nonce)
    ring = D.Keyring()
    ring.add("key", key, nonce)
    return _aligned_extracts(*D._aligned_soft(latents, ring, message_length, aligns, levels, 1, fpr))


def _aligned_extracts(results, aidx, bits) -> List[AlignedExtract]:
    out = []
    for r, i, row in zip(results, aidx, bits):
        c = r.candidates[0]
        out.append(AlignedExtract(c.alignment, int(i), c.stat, c.log10_p_any, r.key_id is not None, row.copy(), r.flags))
    return out


def extract_aligned_soft_l(latents: torch.Tensor, key: bytes, nonce: bytes, message_length: int, aligns: Sequence[Alignment], l: int, *, levels: int = 15,
                           fpr: float = 1e-6) -> List[AlignedExtract]:
    """`extract_aligned_soft` for multi-bit windows (l = 2 or 4), a keyring of one through `detect.detect_latents_aligned_soft_l`: per image the best alignment
    by the level-weighted statistic over its n l cipher bits, its Chernoff bound given the levels under that alignment over the A candidates, and the soft vote
    (`codec.extract_soft_l`, the same thresholds) on the latent with that alignment applied.  l = 1 is refused: that is `extract_aligned_soft`."""
    from . import detect as D
    codec._check_key_nonce(key, nonce)
    l = codec._multi_bit_window(l, "extract_aligned_soft")
    ring = D.Keyring()
    ring.add("key", key, nonce)
    return _aligned_extracts(*D._aligned_soft(latents, ring, message_length, aligns, levels, 1, fpr, l))
