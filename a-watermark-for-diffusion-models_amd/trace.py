"""Traceability: given inverted latents and a registry of issued messages, which user made the image -- and how sure are we.

The reference stops at "bit accuracy against the one message you already know" (extract.py:103-110).  A service that issues one
message per user asks the opposite question: the message is unknown, the candidates are every message ever issued.  This module
holds the registry (`Registry`), the search (`trace_latents`: `codec.extract_batch` vote counts -> `codec.trace_topk`, one HIP launch
over the packed registry) and the statistics that turn a score into a false-positive bound, plus a front end
(`python -m gswm_amd.trace`) on `extract`'s image -> latent -> inversion harness.

Scores.  With c[t] the number of '1' votes of message bit t out of V and r[t] the candidate's bit,
    soft (default): s = sum_t (2 r[t] - 1) (2 c[t] - V)      the vote margins: a bit that won 64:0 counts more than one that won 33:31
    hard:           s = 2 agree - M                          agree = bits of the reference's majority vote (ties -> 0) equal to r

Null model (the paper's): for an image that carries no watermark under this key the decrypted signs are independent fair bits.
* soft: s is a signed sum over all n = M V lattice bits, so for any fixed message s = 2 X - n with X ~ Bin(n, 1/2) EXACTLY, ties and
  all (`log10_p_soft`).  When the lattice size is not a multiple of 8 the up-to-7 padding bits are keystream, not image; they are fair
  bits as well, but not the image's.
* hard: ties -> 0 bias the voted bits when V is even, so agree is not Bin(M, 1/2); it is stochastically dominated by Bin(M, q),
  q = (1 + C(V, V/2) / 2^V) / 2 (q = 1/2 for odd V), and the tail of that is an upper bound (`log10_p_hard`).
Both tails are summed as Python integers and converted to a double once, at the end.  Over a registry of U users the reported value is
the Bonferroni bound min(0, log10 p + log10 U); an image is attributed iff that is <= log10(fpr).

Single key (`Registry`, `trace_latents`): every candidate shares one ChaCha20 key / nonce.

Reliability levels (`trace_latents(..., reliability=T)`, `--reliability T`; single key, l = 1): the vote is the soft-decision vote of `soft.py`, every
lattice bit weighted by an integer level 0..T taken from its element's magnitude, s = sum_t (2 r[t] - 1) score[t].  The same search launch ranks
it (`reliability_counts`).  Given the levels the null model still makes every decrypted bit a fair coin, but the weighted sum has no closed-form
tail: the reported value is the Hoeffding bound `soft.log10_p(s, sum level^2)`, valid but looser than an exact tail.

Per-record keys (`KeyedRegistry`, `trace_latents_keyed`, `--per_record_keys`): what gs_insert logs when key and nonce are left blank --
a fresh random key and nonce per run, so the log is a list of (key, nonce, message) triples.  Decrypting the image under a record's
key and comparing with its message is the same as comparing the image's quantised sign bits h with the record's codeword
e = keystream(key, nonce) XOR (message repeated), the cipher bits the embed plants: s = n - 2 popcount(h XOR e).  The image is
quantised and packed once (`codec.sign_pack`) and one launch (`codec.trace_keyed_topk`) generates every record's keystream in
registers.  For records that share one key s IS the soft score above; under the null model s = 2 X - n, X ~ Bin(n, 1/2) exactly for
any fixed record and any key, so `log10_p_soft` and the Bonferroni bound carry over.  Only the soft statistic exists across keys.

Reliability levels across keys (`trace_latents_keyed_soft`, `--per_record_keys --keyed_reliability T`; l = 1): the image is quantised once
into its sign row AND the bit planes of its levels (`codec.level_pack`), and one launch (`codec.trace_keyed_soft_topk`) ranks every record
by s = sum_j level_j (1 - 2 (h_j XOR e_j)) -- for records of one key the number `reliability=T` ranks by.  Given the levels, the bits of a
key-independent image under any key are fair coins, so the Hoeffding bound `soft.log10_p(s, sum level^2)` holds across keys as it does
within one.

The same at l = 2 and 4 (`trace_latents_keyed_soft_l`, `--per_record_keys --window_reliability T --l 2|4`): every cipher BIT of an element carries
a level, its element's distance from the nearest quantiser boundary that would flip it (`codec.level_pack_l`); the search and the bound are the
ones above over the n l bits.

Where (`tamper_tile=`, `--tamper_map DIR`): an attributed image can also be asked WHERE it still carries the record's watermark --
`TraceResult.tamper`, the per-tile agreement with the attributed record's codeword (`tamper.TamperMap`, one `codec.tile_agreement` launch more
per batch).  The record comes from the registry, not from the image, so each tile's count has the exact binomial null as well.

Through flips, quarter turns and lattice shifts (`trace_latents_aligned`, `trace_latents_keyed_aligned`, `--align flips|d4 [--align_shift R]`): the search runs
over every (record, alignment) pair of `align.alignments` after one inversion and one quantisation.  Under one key `codec.counts_align` writes the vote counts
of every alignment in one launch and `codec.trace_topk` ranks them; across keys `codec.rows_align` feeds `codec.trace_keyed_topk`.  For a fixed pair the null
law is unchanged, the bound is Bonferroni over the U A pairs, and the tamper map is taken on the un-aligned latent.

The aligned searches ranked by reliability levels: `trace_latents_aligned_soft`, `trace_latents_keyed_aligned_soft` (`--align_reliability LEVELS`, l = 1,
DESIGN.md section 4.26) and, for multi-bit windows, `trace_latents_aligned_soft_l`, `trace_latents_keyed_aligned_soft_l` (`--align_window_reliability LEVELS
--l 2|4`, section 4.28): `codec.level_counts_align[_l]` under one key, `codec.level_rows_align[_l]` + `codec.trace_keyed_soft_topk` across keys.
"""
from __future__ import annotations

import math
import os
import sys
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import codec

INT32_MIN = -2 ** 31
_LOG10_2 = math.log10(2.0)


# ===================================================================================================================== statistics
def _log10_ratio(num: int, den: int) -> float:
    """log10(num / den) for integers 0 <= num <= den of any size; the only inexact steps are one correctly rounded division and
    the logarithm of its result."""
    if num <= 0:
        return -math.inf
    if num >= den:
        return 0.0
    if 2 * num > den:                                   # close to 1: go through the complement
        return math.log1p(-((den - num) / den)) / math.log(10.0)
    shift = den.bit_length() - num.bit_length()         # (num << shift) / den is in (1/2, 2): no underflow however small the ratio
    return math.log10((num << shift) / den) - shift * _LOG10_2


def _binomial_tail(n: int, x0: int, a: int = 1, b: int = 1) -> int:
    """sum_{x >= x0} C(n, x) a^x b^(n-x), exact"""
    x0 = max(int(x0), 0)
    if x0 > n:
        return 0
    c = math.comb(n, x0)
    if a == 1 and b == 1:
        total = 0
        for x in range(x0, n + 1):
            total += c
            c = c * (n - x) // (x + 1)
        return total
    total = 0
    pa, pb = a ** x0, [1] * (n - x0 + 1)
    for i in range(1, n - x0 + 1):
        pb[i] = pb[i - 1] * b
    for x in range(x0, n + 1):
        total += c * pa * pb[n - x]
        c = c * (n - x) // (x + 1)
        pa *= a
    return total


def log10_p_soft(score: int, n: int) -> float:
    """log10 P[S >= score] for S = 2 X - n, X ~ Bin(n, 1/2): the soft score of a fixed message under the null model, n = M V."""
    score, n = int(score), int(n)
    if n < 1:
        raise ValueError("n must be positive")
    x0 = -((-(score + n)) // 2)                         # ceil((score + n) / 2)
    return _log10_ratio(_binomial_tail(n, x0), 1 << n)


def hard_match_probability(V: int) -> Tuple[int, int]:
    """q = (1 + C(V, V/2) / 2^V) / 2 as a ratio of integers (1/2 for odd V): the largest probability with which a voted bit of an
    unwatermarked image equals a given message bit (a tie votes 0, which favours message bits that are 0)."""
    V = int(V)
    if V < 1:
        raise ValueError("V must be positive")
    if V % 2:
        return 1, 2
    return (1 << V) + math.comb(V, V // 2), 1 << (V + 1)


def log10_p_hard(agree: int, M: int, V: int) -> float:
    """Upper bound of log10 P[agree' >= agree] under the null model: the tail of Bin(M, q), q = hard_match_probability(V)."""
    agree, M = int(agree), int(M)
    if M < 1:
        raise ValueError("M must be positive")
    a, d = hard_match_probability(V)
    return _log10_ratio(_binomial_tail(M, agree, a, d - a), d ** M)


def log10_p_any(log10_p: float, n_users: int) -> float:
    """Bonferroni bound over a registry: min(0, log10 p + log10 U)"""
    return min(0.0, log10_p + math.log10(int(n_users)))


# ===================================================================================================================== host oracle
def topk_host(counts, copies: int, registry_bits, k: int, soft: bool = True):
    """NumPy restatement of `codec.trace_topk` (int64 arithmetic, a stable sort): (idx int32 [B, k], score int32 [B, k]).
    counts [B, M] '1'-votes, registry_bits uint8 [U, M/8] MSB first.  Shares no code with the device path."""
    c = np.asarray(counts).astype(np.int64)
    reg = np.asarray(registry_bits, dtype=np.uint8)
    B, M = c.shape
    U = reg.shape[0]
    V = int(copies)
    if reg.shape[1] * 8 != M:
        raise ValueError("registry rows and counts disagree on the message length")
    w = (2 * c - V) if soft else np.where(2 * c > V, 1, -1).astype(np.int64)
    scores = np.empty((B, U), dtype=np.int64)
    step = max(1, (1 << 24) // max(M, 1))
    for u0 in range(0, U, step):
        r = np.unpackbits(reg[u0:u0 + step], axis=1, bitorder="big").astype(np.int64)
        scores[:, u0:u0 + step] = w @ (2 * r - 1).T
    idx = np.full((B, k), -1, dtype=np.int32)
    out = np.full((B, k), INT32_MIN, dtype=np.int32)
    order = np.argsort(-scores, axis=1, kind="stable")[:, :k]          # stable: equal scores keep ascending index
    m = order.shape[1]
    idx[:, :m] = order
    out[:, :m] = np.take_along_axis(scores, order, axis=1)
    return idx, out


def keyed_topk_host(signs, codewords, k: int):
    """NumPy restatement of `codec.trace_keyed_topk` that takes the codewords as an argument (int64 arithmetic, a stable sort):
    signs uint8 [B, n/8], codewords uint8 [U, n/8] (the packed cipher bits of each record, e.g. np.packbits of the oracle's
    `cipher_bits`) -> (idx int32 [B, k], score int32 [B, k]), score = n - 2 popcount(signs ^ codeword).  Shares no code with the device path."""
    h = np.asarray(signs, dtype=np.uint8)
    e = np.asarray(codewords, dtype=np.uint8)
    if h.ndim != 2 or e.ndim != 2 or h.shape[1] != e.shape[1]:
        raise ValueError("sign rows and codewords disagree on the lattice size")
    B, U, n = h.shape[0], e.shape[0], 8 * h.shape[1]
    hb = np.unpackbits(h, axis=1).astype(np.int64)
    scores = np.empty((B, U), dtype=np.int64)
    step = max(1, (1 << 24) // max(n, 1))
    for u0 in range(0, U, step):
        eb = np.unpackbits(e[u0:u0 + step], axis=1).astype(np.int64)
        scores[:, u0:u0 + step] = (2 * hb - 1) @ (2 * eb - 1).T              # agreeing bits minus differing bits = n - 2 popcount(h ^ e)
    idx = np.full((B, k), -1, dtype=np.int32)
    out = np.full((B, k), INT32_MIN, dtype=np.int32)
    order = np.argsort(-scores, axis=1, kind="stable")[:, :k]
    m = order.shape[1]
    idx[:, :m] = order
    out[:, :m] = np.take_along_axis(scores, order, axis=1)
    return idx, out


def keyed_soft_topk_host(signs, planes, wsum, codewords, k: int):
    """NumPy restatement of `codec.trace_keyed_soft_topk` that takes the codewords as an argument (int64 arithmetic, a stable sort):
    signs uint8 [B, n/8], planes uint8 [B, P, n/8] (plane k = bit k of the levels), wsum [B] (must be the sum of the levels the planes
    hold), codewords uint8 [U, n/8] -> (idx int32 [B, k], score int32 [B, k]),
    score = wsum - 2 sum_k 2^k popcount(plane_k & (signs ^ codeword)).  Shares no code with the device path."""
    h = np.asarray(signs, dtype=np.uint8)
    pl = np.asarray(planes, dtype=np.uint8)
    e = np.asarray(codewords, dtype=np.uint8)
    W = np.asarray(wsum).astype(np.int64)
    if h.ndim != 2 or e.ndim != 2 or pl.ndim != 3 or h.shape[1] != e.shape[1] or pl.shape[0] != h.shape[0] or pl.shape[2] != h.shape[1]:
        raise ValueError("sign rows, level planes and codewords disagree on the batch or the lattice size")
    if not 1 <= pl.shape[1] <= 4 or W.shape != (h.shape[0],):
        raise ValueError("planes must be [B, P, n/8] with P in 1..4 and wsum [B]")
    B, U, n = h.shape[0], e.shape[0], 8 * h.shape[1]
    lv = np.zeros((B, n), dtype=np.int64)
    for p in range(pl.shape[1]):
        lv += np.unpackbits(pl[:, p], axis=1).astype(np.int64) << p
    if not np.array_equal(lv.sum(axis=1), W):
        raise ValueError("wsum is not the sum of the levels in the planes")
    scores = np.empty((B, U), dtype=np.int64)
    step = max(1, (1 << 24) // max(n, 1))
    signed = lv * (1 - 2 * np.unpackbits(h, axis=1).astype(np.int64))        # level_j (1 - 2 h_j)
    for u0 in range(0, U, step):
        eb = np.unpackbits(e[u0:u0 + step], axis=1).astype(np.int64)
        scores[:, u0:u0 + step] = signed @ (1 - 2 * eb).T                     # 1 - 2 (h ^ e) = (1 - 2 h)(1 - 2 e): the weight of the agreeing bits minus the differing
    idx = np.full((B, k), -1, dtype=np.int32)
    out = np.full((B, k), INT32_MIN, dtype=np.int32)
    order = np.argsort(-scores, axis=1, kind="stable")[:, :k]
    m = order.shape[1]
    idx[:, :m] = order
    out[:, :m] = np.take_along_axis(scores, order, axis=1)
    return idx, out


# ===================================================================================================================== registry
def _check_user_id(user_id) -> None:
    if not isinstance(user_id, str) or not user_id or any(ch in user_id for ch in "\t\r\n"):
        raise ValueError(f"user id {user_id!r} must be a non-empty string without tabs or line breaks")


def _as_bytes(x, what: str) -> Optional[bytes]:
    if x is None:
        return None
    if isinstance(x, str):
        return bytes.fromhex(x)
    if isinstance(x, (bytes, bytearray)):
        return bytes(x)
    raise TypeError(f"{what} must be bytes or a hex string")


class Registry:
    """Ordered, unique user_id -> message bytes, all of one length (`message_bytes`, default 32 = what gs_insert embeds)."""

    def __init__(self, message_bytes: int = 32):
        if int(message_bytes) < 1:
            raise ValueError("message_bytes must be positive")
        self.message_bytes = int(message_bytes)
        self._ids: List[str] = []
        self._messages: List[bytes] = []
        self._by_id: Dict[str, int] = {}
        self._by_message: Dict[bytes, int] = {}
        self._device_cache = {}

    # -- content
    def __len__(self) -> int:
        return len(self._ids)

    @property
    def message_bits(self) -> int:
        return 8 * self.message_bytes

    @property
    def user_ids(self) -> List[str]:
        return list(self._ids)

    def message(self, user_id: str) -> bytes:
        return self._messages[self._by_id[user_id]]

    def user_at(self, index: int) -> str:
        return self._ids[index]

    def message_at(self, index: int) -> bytes:
        return self._messages[index]

    def add(self, user_id: str, message: Union[str, bytes]) -> int:
        """Register `message` for `user_id`; returns the row index.  A str is what gs_insert would embed for it
        (`codec.pad_message`: UTF-8, zero-padded or cut to message_bytes); bytes must have the registry's length."""
        _check_user_id(user_id)
        if isinstance(message, str):
            if not message:
                raise ValueError(f"user {user_id!r}: an empty message string cannot be registered (pad_message would draw random bytes)")
            msg = codec.pad_message(message, self.message_bytes)
        elif isinstance(message, (bytes, bytearray)):
            msg = bytes(message)
            if len(msg) != self.message_bytes:
                raise ValueError(f"user {user_id!r}: message has {len(msg)} bytes, the registry holds {self.message_bytes}-byte messages")
        else:
            raise TypeError(f"user {user_id!r}: message must be str or bytes")
        if user_id in self._by_id:
            raise ValueError(f"user id {user_id!r} is already registered")
        if msg in self._by_message:
            raise ValueError(f"user {user_id!r}: message {msg.hex()} is already registered to {self._ids[self._by_message[msg]]!r}")
        self._by_id[user_id] = self._by_message[msg] = len(self._ids)
        self._ids.append(user_id)
        self._messages.append(msg)
        self._device_cache.clear()
        return len(self._ids) - 1

    # -- files
    def save(self, path) -> None:
        """one `user_id<TAB>message_hex` per line"""
        with open(path, "w") as f:
            for uid, msg in zip(self._ids, self._messages):
                f.write(f"{uid}\t{msg.hex()}\n")

    @classmethod
    def load(cls, path) -> "Registry":
        reg = None
        with open(path) as f:
            for no, line in enumerate(f, 1):
                line = line.rstrip("\r\n")
                if not line:
                    continue
                uid, sep, hx = line.partition("\t")
                if not sep or "\t" in hx:                # (bytes.fromhex skips tabs: a keyed registry would load as one long message)
                    raise ValueError(f"{path}:{no}: expected 'user_id<TAB>message_hex'" + (" (a registry with per-record keys? see KeyedRegistry)" if sep else ""))
                try:
                    msg = bytes.fromhex(hx.strip())
                except ValueError:
                    raise ValueError(f"{path}:{no}: message of user {uid!r} is not hexadecimal") from None
                if reg is None:
                    reg = cls(len(msg))
                reg.add(uid, msg)
        if reg is None:
            raise ValueError(f"{path}: no registry entries")
        return reg

    @classmethod
    def from_info_data(cls, path, key=None, nonce=None) -> "Registry":
        """The log gs_insert (and the reference, gs_insert.py:68-74) appends per issued watermark -- records of
        `Time: / key: / nonce: / message: / ------` lines -- read as a registry: the records of the given key and nonce (bytes or hex;
        None keeps any), repeated messages dropped, ids `info:<record number>` (1-based over ALL records of the file)."""
        key, nonce = _as_bytes(key, "key"), _as_bytes(nonce, "nonce")
        reg = None
        for number, rec_key, rec_nonce, message in _info_data_records(path):
            if (key is None or rec_key == key.hex()) and (nonce is None or rec_nonce == nonce.hex()):
                msg = bytes.fromhex(message)
                if reg is None:
                    reg = cls(len(msg))
                if msg not in reg._by_message:
                    reg.add(f"info:{number}", msg)
        if reg is None:
            raise ValueError(f"{path}: no record matches the given key / nonce")
        return reg

    @classmethod
    def from_file(cls, path, key=None, nonce=None) -> "Registry":
        """Either format, told apart by the first line"""
        return cls.from_info_data(path, key, nonce) if detect_format(path) == "info_data" else cls.load(path)

    # -- device
    def packed(self, message_length: Optional[int] = None) -> np.ndarray:
        """uint8 [U, message_length / 8]: one message per row, MSB first as the codec packs them; a message_length that is a multiple
        of the registered length repeats the rows (the embed repeats its message over the lattice in the same way)."""
        m = self.message_bits if message_length is None else int(message_length)
        if m <= 0 or m % self.message_bits:
            raise ValueError(f"message_length {m} is not a multiple of the registered length {self.message_bits}")
        if not self._ids:
            raise ValueError("the registry is empty")
        t = self._device_cache.get(("host", m))
        if t is None:
            rows = np.frombuffer(b"".join(self._messages), dtype=np.uint8).reshape(len(self._ids), self.message_bytes)
            t = self._device_cache[("host", m)] = np.ascontiguousarray(np.tile(rows, (1, m // self.message_bits)))
        return t

    def to_device(self, device="cuda", message_length: Optional[int] = None):
        import torch
        m = self.message_bits if message_length is None else int(message_length)
        k = (str(torch.device(device)), m)
        t = self._device_cache.get(k)
        if t is None:
            t = self._device_cache[k] = torch.from_numpy(self.packed(m)).to(device)
        return t


def detect_format(path) -> str:
    """'info_data' when the first non-empty line is a `Time:` line of gs_insert's log, 'keyed_registry' when it has the four columns
    `KeyedRegistry.save` writes, else 'registry'"""
    with open(path) as f:
        for line in f:
            if line.strip():
                if line.startswith("Time:") and "\t" not in line:
                    return "info_data"
                return "keyed_registry" if line.rstrip("\r\n").count("\t") == 3 else "registry"
    raise ValueError(f"{path} is empty")


def _info_data_records(path):
    """(record number, key_hex, nonce_hex, message_hex) of every record of a gs_insert log that has a message, numbered from 1"""
    rec, number = {}, 0
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith("-----"):
                if "message" in rec:
                    number += 1
                    yield number, rec.get("key"), rec.get("nonce"), rec["message"]
                rec = {}
                continue
            name, sep, value = line.partition(":")
            if sep and name in ("key", "nonce", "message"):
                rec[name] = value.strip().lower()


class KeyedRegistry:
    """Ordered user_id -> (key, nonce, message) records, each with its own ChaCha20 key and nonce: unique ids, unique triples, all
    messages of one length (`message_bytes`, default 32 = what gs_insert embeds)."""

    def __init__(self, message_bytes: int = 32):
        if not 1 <= int(message_bytes) <= 256:
            raise ValueError("message_bytes must be in 1..256")
        self.message_bytes = int(message_bytes)
        self._ids: List[str] = []
        self._records: List[Tuple[bytes, bytes, bytes]] = []
        self._by_id: Dict[str, int] = {}
        self._by_record: Dict[Tuple[bytes, bytes, bytes], int] = {}
        self._device_cache = {}

    # -- content
    def __len__(self) -> int:
        return len(self._ids)

    @property
    def message_bits(self) -> int:
        return 8 * self.message_bytes

    @property
    def user_ids(self) -> List[str]:
        return list(self._ids)

    @property
    def n_keys(self) -> int:
        """distinct (key, nonce) pairs"""
        return len({(k, n) for k, n, _ in self._records})

    def record(self, user_id: str) -> Tuple[bytes, bytes, bytes]:
        return self._records[self._by_id[user_id]]

    def user_at(self, index: int) -> str:
        return self._ids[index]

    def record_at(self, index: int) -> Tuple[bytes, bytes, bytes]:
        return self._records[index]

    def add(self, user_id: str, key: Union[str, bytes], nonce: Union[str, bytes], message: Union[str, bytes]) -> int:
        """Register (key, nonce, message) for `user_id`; returns the row index.  key (32 bytes) and nonce (16 bytes) are bytes or hex
        strings; a str message is what gs_insert would embed for it (`codec.pad_message`), bytes must have the registry's length."""
        _check_user_id(user_id)
        try:
            key, nonce = _as_bytes(key, "key"), _as_bytes(nonce, "nonce")
        except ValueError:
            raise ValueError(f"user {user_id!r}: key and nonce must be hexadecimal") from None
        if key is None or len(key) != 32:
            raise ValueError(f"user {user_id!r}: the ChaCha20 key must be 32 bytes")
        if nonce is None or len(nonce) != 16:
            raise ValueError(f"user {user_id!r}: the ChaCha20 nonce must be 16 bytes")
        if isinstance(message, str):
            if not message:
                raise ValueError(f"user {user_id!r}: an empty message string cannot be registered (pad_message would draw random bytes)")
            msg = codec.pad_message(message, self.message_bytes)
        elif isinstance(message, (bytes, bytearray)):
            msg = bytes(message)
            if len(msg) != self.message_bytes:
                raise ValueError(f"user {user_id!r}: message has {len(msg)} bytes, the registry holds {self.message_bytes}-byte messages")
        else:
            raise TypeError(f"user {user_id!r}: message must be str or bytes")
        if user_id in self._by_id:
            raise ValueError(f"user id {user_id!r} is already registered")
        rec = (key, nonce, msg)
        if rec in self._by_record:
            raise ValueError(f"user {user_id!r}: this key, nonce and message {msg.hex()} are already registered to {self._ids[self._by_record[rec]]!r}")
        self._by_id[user_id] = self._by_record[rec] = len(self._ids)
        self._ids.append(user_id)
        self._records.append(rec)
        self._device_cache.clear()
        return len(self._ids) - 1

    # -- files
    def save(self, path) -> None:
        """one `user_id<TAB>key_hex<TAB>nonce_hex<TAB>message_hex` per line"""
        with open(path, "w") as f:
            for uid, (key, nonce, msg) in zip(self._ids, self._records):
                f.write(f"{uid}\t{key.hex()}\t{nonce.hex()}\t{msg.hex()}\n")

    @classmethod
    def load(cls, path) -> "KeyedRegistry":
        reg = None
        with open(path) as f:
            for no, line in enumerate(f, 1):
                line = line.rstrip("\r\n")
                if not line:
                    continue
                cols = line.split("\t")
                if len(cols) != 4:
                    raise ValueError(f"{path}:{no}: expected 'user_id<TAB>key_hex<TAB>nonce_hex<TAB>message_hex'")
                try:
                    key, nonce, msg = (bytes.fromhex(c.strip()) for c in cols[1:])
                except ValueError:
                    raise ValueError(f"{path}:{no}: record of user {cols[0]!r} is not hexadecimal") from None
                if reg is None:
                    reg = cls(len(msg))
                reg.add(cols[0], key, nonce, msg)
        if reg is None:
            raise ValueError(f"{path}: no registry entries")
        return reg

    @classmethod
    def from_info_data(cls, path) -> "KeyedRegistry":
        """EVERY record of the log gs_insert appends per issued watermark, each under its own key and nonce; ids `info:<record number>`
        (numbered as `Registry.from_info_data` numbers them), repeated (key, nonce, message) triples dropped."""
        reg = None
        for number, key, nonce, message in _info_data_records(path):
            if key is None or nonce is None:
                raise ValueError(f"{path}: record {number} has no key / nonce")
            rec = (bytes.fromhex(key), bytes.fromhex(nonce), bytes.fromhex(message))
            if reg is None:
                reg = cls(len(rec[2]))
            if rec not in reg._by_record:
                reg.add(f"info:{number}", *rec)
        if reg is None:
            raise ValueError(f"{path}: no records")
        return reg

    @classmethod
    def from_file(cls, path) -> "KeyedRegistry":
        """gs_insert's log or the four-column format, told apart by the first line"""
        fmt = detect_format(path)
        if fmt == "registry":
            raise ValueError(f"{path}: 'user_id<TAB>message_hex' lines carry no keys: this is a single-key registry (trace without --per_record_keys)")
        return cls.from_info_data(path) if fmt == "info_data" else cls.load(path)

    # -- device
    @property
    def record_stride(self) -> int:
        return codec.keyed_record_stride(self.message_bytes)

    def packed(self) -> np.ndarray:
        """uint8 [U, record_stride]: a row is key[32] | nonce[16] | message, zero-padded to a multiple of 16 bytes
        (the record rows of `codec.trace_keyed_topk`)"""
        if not self._ids:
            raise ValueError("the registry is empty")
        t = self._device_cache.get("host")
        if t is None:
            t = np.zeros((len(self._ids), self.record_stride), dtype=np.uint8)
            flat = np.frombuffer(b"".join(k + n + m for k, n, m in self._records), dtype=np.uint8)
            used = codec.KEYED_RECORD_HEAD + self.message_bytes
            t[:, :used] = flat.reshape(len(self._ids), used)
            self._device_cache["host"] = t
        return t

    def to_device(self, device="cuda"):
        import torch
        k = str(torch.device(device))
        t = self._device_cache.get(k)
        if t is None:
            t = self._device_cache[k] = torch.from_numpy(self.packed()).to(device)
        return t


# ===================================================================================================================== tracing
@dataclass
class Candidate:
    user_id: str
    index: int
    score: int
    agree: int                  # voted bits equal to the candidate's message (what codec.bit_matches gives for it)
    log10_p_any: float          # Bonferroni bound over the registry (over the registry x alignments pairs of an aligned search)
    alignment: Optional[Tuple[int, int, int]] = None   # aligned searches: this record's best alignment; `align.apply(latent, alignment)` is what matched


@dataclass
class TraceResult:
    candidates: List[Candidate] = field(default_factory=list)
    attributed: Optional[str] = None       # the best candidate's user id if its bound is <= log10(fpr), else None: no registered user
    tamper: Optional["TamperMap"] = None   # tamper.TamperMap against the attributed record (tamper_tile=...): where the image still carries it
    alignment: Optional[Tuple[int, int, int]] = None   # aligned searches: the attributed record's alignment (None: not attributed, or no alignments searched)


def _attach_tamper_maps(out, z, packed, records, M: int, l: int, tile: int, fpr: float) -> None:
    """Fill `TraceResult.tamper` of every attributed image: one `codec.tile_agreement` launch over the batch, each image against the
    (key, nonce, message) of its own best candidate (records[b]; None for an image that was not attributed, whose row is ignored).
    The message comes from the registry, not from the image, so the counts are Bin(n_t, 1/2) under the null: source "registry"."""
    from . import tamper as TM
    if z.dim() != 4:
        raise ValueError(f"tamper_tile needs latents [B, C, h, w] (got {tuple(z.shape)}): the tiles are cut from the last two dimensions")
    todo = [b for b, r in enumerate(records) if r is not None]
    if not todo:
        return
    shape = tuple(int(s) for s in z.shape[1:])
    blank = (bytes(32), bytes(16), bytes(M // 8))
    rows = [r if r is not None else blank for r in records]
    agree = codec.tile_agreement(packed, TM.keys_tensor([(k, n) for k, n, _ in rows], z.device), TM._message_rows([m for _, _, m in rows], M, z.device),
                                 M, shape, l, tile).cpu().numpy()
    n_t = shape[0] * int(tile) * int(tile) * codec.check_window(l)
    for b in todo:
        out[b].tamper = TM.make_map(agree[b], n_t, tile, fpr, "registry")


def _log10_fpr(fpr) -> float:
    """log10 of a false-positive rate in (0, 1], or ValueError"""
    if not 0.0 < float(fpr) <= 1.0:
        raise ValueError("fpr must be in (0, 1]")
    return math.log10(float(fpr))


def _pairs_to_host(idx, score):
    """(idx, score) [B, k] of a search on the device -> the two host arrays: the B k pairs in one copy"""
    import torch
    pairs = torch.stack([idx, score]).cpu().numpy()
    return pairs[0], pairs[1]


def _flag_error(flags: int) -> Optional[ValueError]:
    """The ValueError the reference raises for an image with these GSW_FLAG_* (a NaN / saturated latent, extract.py:84-86), or None"""
    from . import _native as N
    if flags & N.GSW_FLAG_NAN:
        return ValueError("cannot convert float NaN to integer")
    if flags & N.GSW_FLAG_SATURATED:
        return ValueError("invalid literal for int() with base 2")


def _candidate_lists(idx_h, score_h, flags_h, limit: float, candidate, result, refuse: bool = True) -> list:
    """One result per image from the host pairs of a search: result(b, candidates, attributed) with candidate(b, j, index, score) for every entry before
    the list's end (index -1), best first; the attribution rule: the best candidate's bound is <= limit.  refuse: a flagged image gets the reference's
    ValueError instead of a result (`detect_latents` reports the flags and goes on)."""
    out = []
    for b in range(idx_h.shape[0]):
        err = _flag_error(int(flags_h[b])) if refuse else None
        if err is not None:
            out.append(err)
            continue
        found = []
        for j in range(idx_h.shape[1]):
            i = int(idx_h[b, j])
            if i < 0:
                break
            found.append(candidate(b, j, i, int(score_h[b, j])))
        out.append(result(b, found, bool(found) and found[0].log10_p_any <= limit))
    return out


def _trace_result(b, candidates, attributed):
    return TraceResult(candidates, candidates[0].user_id if attributed else None)


def _best_records(out, record_at) -> list:
    """`_attach_tamper_maps`' records: record_at(index of the best candidate) of every attributed image, None for the others"""
    return [record_at(r.candidates[0].index) if isinstance(r, TraceResult) and r.attributed is not None else None for r in out]


def reliability_counts(score, levels: int, copies: int):
    """The (counts', copies') that make `codec.trace_topk`'s soft weight 2 c' - copies' equal to 2 score[b, t], the level-weighted vote of
    `codec.extract_soft`: c' = score + levels copies (0 <= c' <= copies'), copies' = 2 levels copies.  Works on tensors and arrays; raises
    where gsw_trace_topk's limits on copies' would not hold."""
    T, V = int(levels), int(copies)
    M = int(score.shape[-1])
    if 2 * T * V > 2000000 or M * 2 * T * V >= 2 ** 31:
        raise ValueError(f"reliability={T} with {V} copies of {M} message bits is beyond the registry search's limits "
                         "(2 levels copies <= 2 000 000 and msg_bits 2 levels copies < 2^31)")
    return score + T * V, 2 * T * V


def trace_latents(latents, key: bytes, nonce: bytes, registry: Registry, *, message_length: Optional[int] = None, k: int = 1,
                  fpr: float = 1e-6, soft: bool = True, l: int = 1, tamper_tile: Optional[int] = None,
                  reliability: Optional[int] = None) -> List[Union[TraceResult, ValueError]]:
    """latents [B, ...] on the device -> one TraceResult per image (best candidate first), or the ValueError the reference raises for
    that image (a saturated / NaN latent, extract.py:84-86), like `extract.recover_exactracted_message_batch`.

    One vote kernel, one search launch over the packed registry; the host receives the B k pairs (plus the vote's flags and bits).
    l: cipher bits per lattice element the images were embedded with (a property of the deployment, like the key).
    tamper_tile: 8, 16 or 32 -> every attributed image also gets `TraceResult.tamper`, the per-tile agreement with its best candidate's
    codeword (one quantise-and-pack and one `codec.tile_agreement` launch more per batch); None: nothing more runs.
    reliability: None, or the number of reliability levels (1..15) of the level-weighted statistic: the vote is `soft.extract_soft` with
    thresholds scaled to each image's RMS, a candidate's score is sum_t (2 r[t] - 1) score[t] (the same search launch, fed through
    `reliability_counts`), `Candidate.agree` counts the soft vote's bits and the p-value is the Hoeffding bound `soft.log10_p` with the
    image's wsq -- a bound, not the exact binomial tail of the margin statistic.  Not with soft=False, l = 1 only."""
    import torch
    limit = _log10_fpr(fpr)
    l = codec.check_window(l)
    if reliability is not None:
        if not soft:
            raise ValueError("reliability cannot be combined with --hard (soft=False): the level-weighted statistic ranks by weighted margins")
        if l != 1:
            raise ValueError(f"reliability cannot be combined with l = {l}: reliability levels are defined for one cipher bit per element")
        from . import soft as S
        reliability = S._check_table(reliability, 2.5)[0]
    M = registry.message_bits if message_length is None else int(message_length)
    z = latents.contiguous()
    B = z.shape[0]
    rows = registry.packed(M)                            # (a message_length the registry cannot be tiled to fails here)
    V = codec.vote_copies(z.numel() // max(B, 1), M, l)
    reg_dev = registry.to_device(z.device, M)
    wsq_h = None
    if reliability is None:
        bits, flags, counts = codec.extract_batch(z, key, nonce, M, return_counts=True, l=l)
        idx, score = codec.trace_topk(counts, V, reg_dev, k=k, soft=soft)
    else:
        vote = S.extract_soft(z, key, nonce, M, levels=reliability)
        bits, flags = vote.bits, vote.flags
        counts, copies = reliability_counts(vote.score, reliability, V)
        idx, score = codec.trace_topk(counts, copies, reg_dev, k=k, soft=True)
        score = torch.where(idx >= 0, score // 2, score)                 # the search weighs 2 score[b, t]: every score is even
        wsq_h = vote.wsq.cpu().numpy()
    idx_h, score_h = _pairs_to_host(idx, score)          # flags and voted bits are the vote's own outputs
    flags_h, bits_h, U = flags.cpu().numpy(), bits.cpu().numpy(), len(registry)

    def candidate(b, j, i, s):
        agree = M - int(np.unpackbits(bits_h[b] ^ rows[i]).sum())
        lp = S.log10_p(s, int(wsq_h[b])) if wsq_h is not None else log10_p_soft(s, M * V) if soft else log10_p_hard(agree, M, V)
        return Candidate(registry.user_at(i), i, s, agree, log10_p_any(lp, U))

    out = _candidate_lists(idx_h, score_h, flags_h, limit, candidate, _trace_result)
    if tamper_tile is not None:
        best = _best_records(out, lambda i: (key, nonce, bytes(rows[i])))
        if any(r is not None for r in best):
            _attach_tamper_maps(out, z, codec.quant_pack(z, l)[0], best, M, l, tamper_tile, fpr)
    return out


def trace_latents_keyed(latents, registry: KeyedRegistry, *, k: int = 1, fpr: float = 1e-6, l: int = 1,
                        tamper_tile: Optional[int] = None, reliability: Optional[int] = None) -> List[Union[TraceResult, ValueError]]:
    """`trace_latents` against a registry whose records carry their own keys: latents [B, ...] on the device -> one TraceResult per
    image (best candidate first), or the ValueError the reference raises for that image (a saturated / NaN latent).

    One quantise-and-pack kernel, one search launch over the record rows (every record's keystream is generated inside it); the host
    receives the B k (index, score) pairs and the flags.  score = n - 2 popcount(signs ^ codeword), whose null distribution is that of
    the soft score (`log10_p_soft(score, n)`), Bonferroni over the records.  `Candidate.agree` is the reference's voted-bit agreement
    under that candidate's own key: `codec.extract_batch` + `codec.bit_matches` for the reported candidates only, grouped by key.
    l: cipher bits per lattice element; the codewords then span n l bits.
    tamper_tile: as in `trace_latents`; the map of an image is taken under its best candidate's OWN key (one launch more per batch).
    reliability: must be None -- the level-weighted search across keys is a search kernel of its own: `trace_latents_keyed_soft`."""
    import torch
    if reliability is not None:
        raise ValueError("reliability cannot be combined with trace_latents_keyed (--per_record_keys): the level-weighted search across keys "
                         "is trace_latents_keyed_soft (--keyed_reliability)")
    limit = _log10_fpr(fpr)
    z = latents.contiguous()
    B = z.shape[0]
    n = z.numel() // max(B, 1)
    M = registry.message_bits
    codec.vote_copies(n, M, l)                           # (a lattice the messages do not tile fails here, as extract_batch would)
    nb = n * codec.check_window(l)
    rec_dev = registry.to_device(z.device)
    signs, flags = codec.quant_pack(z, l)
    idx, score = codec.trace_keyed_topk(signs, nb, rec_dev, registry.message_bytes, k=k)
    idx_h, score_h = _pairs_to_host(idx, score)
    flags_h, U = flags.cpu().numpy(), len(registry)
    reported: Dict[Tuple[bytes, bytes], Dict[bytes, List[Tuple[int, Candidate]]]] = {}      # (key, nonce) -> message -> (image, candidate)

    def candidate(b, j, i, s):
        c = Candidate(registry.user_at(i), i, s, 0, log10_p_any(log10_p_soft(s, nb), U))
        key, nonce, msg = registry.record_at(i)
        reported.setdefault((key, nonce), {}).setdefault(msg, []).append((b, c))
        return c

    out = _candidate_lists(idx_h, score_h, flags_h, limit, candidate, _trace_result)
    for (key, nonce), by_message in reported.items():
        images = sorted({b for pairs_ in by_message.values() for b, _ in pairs_})
        row = {b: r for r, b in enumerate(images)}
        bits, _ = codec.extract_batch(z[torch.tensor(images, device=z.device)].contiguous(), key, nonce, M, l=l)
        for msg, pairs_ in by_message.items():
            agree = codec.bit_matches(bits, M, msg).cpu().numpy()
            for b, c in pairs_:
                c.agree = int(agree[row[b]])
    if tamper_tile is not None:
        _attach_tamper_maps(out, z, signs, _best_records(out, registry.record_at), M, l, tamper_tile, fpr)
    return out


def _trace_keyed_soft(latents, registry: KeyedRegistry, l: int, levels: int, clip: float, thresholds, k: int, fpr: float,
                      tamper_tile: Optional[int]) -> List[Union[TraceResult, ValueError]]:
    """`trace_latents_keyed_soft` (l = 1) and `trace_latents_keyed_soft_l` (l = 2, 4): one level packer, one search over the n l bits, the candidate lists,
    and one soft vote over the reported (image, candidate) pairs for `Candidate.agree`"""
    import torch
    from . import soft as S
    limit = _log10_fpr(fpr)
    z = latents.contiguous()
    B = z.shape[0]
    n = z.numel() // max(B, 1)
    M, mb = registry.message_bits, registry.message_bytes
    codec.vote_copies(n, M, l)                           # (a lattice the messages do not tile fails here, as extract_batch would)
    if thresholds is None:
        thr = S._default_table(z, l, levels, clip)
    else:
        thr = thresholds.to(device=z.device, dtype=torch.float32).contiguous()
    shared = thr.dim() == (1 if l == 1 else 2)          # one table for all images
    rec_dev = registry.to_device(z.device)
    rows = codec.level_pack(z, thr) if l == 1 else codec.level_pack_l(z, thr, l)
    idx, score = codec.trace_keyed_soft_topk(rows, n * l, rec_dev, mb, k=k)
    idx_h, score_h = _pairs_to_host(idx, score)
    flags_h, wsq_h, U = rows.flags.cpu().numpy(), rows.wsq.cpu().numpy(), len(registry)
    reported: List[Tuple[int, Candidate]] = []          # (image, candidate), in order

    def candidate(b, j, i, s):
        c = Candidate(registry.user_at(i), i, s, 0, log10_p_any(S.log10_p(s, int(wsq_h[b])), U))
        reported.append((b, c))
        return c

    out = _candidate_lists(idx_h, score_h, flags_h, limit, candidate, _trace_result)
    if reported:                                        # the soft vote of every reported pair under the candidate's own record, one launch
        img = torch.tensor([b for b, _ in reported], device=z.device)
        rec = torch.tensor([c.index for _, c in reported], device=z.device)
        pairs = (z.reshape(B, -1)[img].contiguous(), rec_dev[rec].contiguous(), mb, thr if shared else thr[img].contiguous())
        vote = codec.extract_soft(*pairs) if l == 1 else codec.extract_soft_l(*pairs, l)
        for (_, c), a in zip(reported, vote.matches.cpu().tolist()):
            c.agree = int(a)
    if tamper_tile is not None:
        _attach_tamper_maps(out, z, rows.signs, _best_records(out, registry.record_at), M, l, tamper_tile, fpr)
    return out


def trace_latents_keyed_soft(latents, registry: KeyedRegistry, *, levels: int = 15, clip: float = 2.5, thresholds=None, k: int = 1,
                             fpr: float = 1e-6, tamper_tile: Optional[int] = None) -> List[Union[TraceResult, ValueError]]:
    """`trace_latents_keyed` ranked by reliability-weighted margins (one cipher bit per element): latents [B, ...] on the device -> one
    TraceResult per image (best candidate first), or the ValueError the reference raises for that image (a saturated / NaN latent).

    Every lattice element votes with an integer level 0..levels taken from its magnitude -- thresholds: float32 [levels] or [B, levels],
    None: `soft.uniform_thresholds(latents, levels, clip)`, scaled to each image's RMS.  One `codec.level_pack` launch, one search launch
    (`codec.trace_keyed_soft_topk`); a candidate's score is sum_j level_j (1 - 2 (sign_j ^ codeword_j)), for records of one key the number
    `trace_latents(..., reliability=levels)` ranks by.  The p-value is the Hoeffding bound `soft.log10_p(score, wsq)`, Bonferroni over the
    records: given the levels, the bits of a key-independent image under ANY key are fair coins, so the bound is as valid across keys as
    within one -- a bound, not the exact binomial tail of `trace_latents_keyed`.  `Candidate.agree` counts the bits of the soft vote under
    the candidate's own record: one `codec.extract_soft` launch over the reported (image, candidate) pairs.
    tamper_tile: as in `trace_latents_keyed`, on the packed sign row.  n (1 + P) may not exceed 1 048 576, P the bit length of `levels`."""
    return _trace_keyed_soft(latents, registry, 1, levels, clip, thresholds, k, fpr, tamper_tile)


def trace_latents_keyed_soft_l(latents, registry: KeyedRegistry, l: int, *, levels: int = 15, clip: float = 2.5, thresholds=None, k: int = 1,
                               fpr: float = 1e-6) -> List[Union[TraceResult, ValueError]]:
    """`trace_latents_keyed_soft` for multi-bit windows (l = 2 or 4): latents [B, ...] on the device -> one TraceResult
    per image (best candidate first), or the ValueError the reference raises for that image (a saturated / NaN latent).

    Every one of the n l cipher bits of an image votes with an integer level 0..levels, the distance of its element from the nearest
    quantiser boundary at which that bit would have come out differently -- thresholds: float32 [l, levels] or [B, l, levels], None:
    `soft.window_thresholds(latents, l, levels, clip)`.  One `codec.level_pack_l` launch, then the unchanged `codec.trace_keyed_soft_topk`
    with n_bits = n l.  The p-value is the Hoeffding bound `soft.log10_p(score, wsq)`, Bonferroni over the records: given the levels, the
    decrypted bits of a key-independent image are independent fair coins, now per cipher bit, so the bound holds as at l = 1.
    `Candidate.agree` counts the bits of the soft vote under the candidate's own record: one `codec.extract_soft_l` launch over the
    reported (image, candidate) pairs.  n l (1 + P) may not exceed 1 048 576, P the bit length of `levels`: the search refuses beyond
    (ValueError).  l = 1 is refused: that is `trace_latents_keyed_soft`."""
    l = codec.check_window(l)
    if l == 1:
        raise ValueError("l = 1 has no window bits: the level-weighted search across keys at l = 1 is trace_latents_keyed_soft (--keyed_reliability)")
    return _trace_keyed_soft(latents, registry, l, levels, clip, thresholds, k, fpr, None)


# ===================================================================================================================== tracing through flips, turns and shifts
ALIGNED_STAT_BITS = 21                  # `align._merge_best`'s stat field: a signed score of at most 1 048 576 lattice bits in magnitude


def _aligned_lattice(latents, what: str):
    if latents.dim() != 4:
        raise ValueError(f"{what} needs latents [B, C, H, W], got {tuple(latents.shape)}")
    z = latents.contiguous()
    return z, tuple(int(s) for s in z.shape[1:])


def _aligned_results(found, flags, cands, limit: float, candidate):
    """The host side of the two aligned searches: found = (index, alignment index, score) int32 [B, k] on the device, in one copy; candidate(b, index,
    score, alignment) -> Candidate.  -> (results, the alignment index of every image's best candidate, 0 where it has none)"""
    import torch
    idx_h, aidx_h, score_h = torch.stack(list(found)).cpu().numpy()
    out = _candidate_lists(idx_h, score_h, flags.cpu().numpy(), limit, lambda b, j, i, s: candidate(b, i, s, cands[int(aidx_h[b, j])]), _trace_result)
    for r in out:
        if isinstance(r, TraceResult) and r.attributed is not None:
            r.alignment = r.candidates[0].alignment
    best = [max(int(aidx_h[b, 0]), 0) if isinstance(r, TraceResult) else 0 for b, r in enumerate(out)]
    return out, best


def _attach_aligned_tamper_maps(out, z, cands, best, records, M: int, l: int, tile: int, fpr: float) -> None:
    """`_attach_tamper_maps` under the alignment: every image goes through its best candidate's alignment (`align.unalign`), is quantised again and
    mapped against its record, so the tiles are those of the lattice AS EMBEDDED"""
    from . import align as AL
    if any(r is not None for r in records):
        zu = AL.unalign(z, cands, best)
        _attach_tamper_maps(out, zu, codec.quant_pack(zu, l)[0], records, M, l, tile, fpr)


def trace_latents_aligned(latents, key: bytes, nonce: bytes, registry: Registry, aligns, *, message_length: Optional[int] = None, k: int = 1,
                          fpr: float = 1e-6, soft: bool = True, l: int = 1, tamper_tile: Optional[int] = None,
                          budget_bytes: Optional[int] = None) -> List[Union[TraceResult, ValueError]]:
    """`trace_latents` through flips, quarter turns and lattice shifts: the search runs over every (record, alignment) pair.  latents [B, C, H, W] on the
    device, aligns from `align.alignments` -> one TraceResult per image (best candidate first), or the reference's ValueError for a NaN / saturated latent.

    One `codec.quant_pack`; then per chunk of images one `codec.counts_align` launch (the vote counts of every alignment of every image, the aligned rows
    are never written) and one `codec.trace_topk` on the [B A, M] counts; then `align.search_keys`' merge per image: every record keeps its best
    alignment, the records are ordered by (score descending, record index ascending, alignment index ascending).  The cuts follow `budget_bytes` (default
    `align.ROWS_BUDGET_BYTES`) with 4 M bytes per aligned image; the result does not depend on them.
    The score of a pair is `trace_latents`' score of `align.apply(latent, alignment)`, so for a FIXED pair the null law is unchanged -- exactly
    Bin(M V, 1/2) for the margins -- and the reported bound is Bonferroni over the U A pairs: `log10_p_any(log10_p_soft(score, M V), U A)`, or
    `log10_p_hard` over U A with soft=False.  (Choosing the alignment first by the blind statistic and tracing afterwards would condition the margins on
    the selection and lose the exact tail)  `Candidate.alignment` is the record's best alignment, `TraceResult.alignment`
    the attributed record's: the alignment that UNDOES the attack.  `Candidate.agree`: the voted bits of the latent with that alignment applied, one
    `codec.extract_batch` launch over the reported (image, candidate) rows.
    tamper_tile: every attributed image is put through its alignment (`align.unalign`), quantised and mapped against its record as in `trace_latents`.
    The map is in the coordinates of the lattice AS EMBEDDED, not of the image as received; the border that a shift wrapped around votes as noise."""
    import torch
    from . import align as AL
    limit = _log10_fpr(fpr)
    l = codec.check_window(l)
    codec._check_key_nonce(key, nonce)
    z, shape = _aligned_lattice(latents, "trace_latents_aligned")
    cands = AL._as_list(aligns, *shape[1:])
    M = registry.message_bits if message_length is None else int(message_length)
    B = z.shape[0]
    rows = registry.packed(M)                            # (a message_length the registry cannot be tiled to fails here)
    V = codec.vote_copies(z.numel() // max(B, 1), M, l)
    M = codec._counts_align_message(shape, l, M)
    reg_dev = registry.to_device(z.device, M)
    packed, flags = codec.quant_pack(z, l)
    table = AL._device_table(cands, shape, z.device)

    def search(rows_b, aligns_dev):
        counts = codec._counts_align_launch(rows_b, shape, l, aligns_dev, key, nonce, M)
        return codec.trace_topk(counts.view(-1, M), V, reg_dev, k=int(k), soft=soft)

    found = AL._search_chunks(B, 4 * M, table, reg_dev, k, budget_bytes, lambda b0, b1: packed[b0:b1], search, stat_bits=ALIGNED_STAT_BITS)
    U, A = len(registry), len(cands)
    reported: List[Tuple[int, Candidate]] = []          # (image, candidate), in order

    def candidate(b, i, s, a):
        lp = log10_p_soft(s, M * V) if soft else log10_p_hard((s + M) // 2, M, V)          # hard: score = 2 agree - M
        c = Candidate(registry.user_at(i), i, s, 0, log10_p_any(lp, U * A), a)
        reported.append((b, c))
        return c

    out, best = _aligned_results(found, flags, cands, limit, candidate)
    if reported:                                        # the vote of every reported pair on its aligned latent, one launch
        bits, _ = codec.extract_batch(torch.stack([AL.apply(z[b], c.alignment) for b, c in reported]).contiguous(), key, nonce, M, l=l)
        for (_, c), row in zip(reported, bits.cpu().numpy()):
            c.agree = M - int(np.unpackbits(row ^ rows[c.index]).sum())
    if tamper_tile is not None:
        _attach_aligned_tamper_maps(out, z, cands, best, _best_records(out, lambda i: (key, nonce, bytes(rows[i]))), M, l, tamper_tile, fpr)
    return out


def trace_latents_keyed_aligned(latents, registry: KeyedRegistry, aligns, *, k: int = 1, fpr: float = 1e-6, l: int = 1,
                                tamper_tile: Optional[int] = None, budget_bytes: Optional[int] = None) -> List[Union[TraceResult, ValueError]]:
    """`trace_latents_keyed` through flips, quarter turns and lattice shifts: the composition `align.search_keys` uses, with the registry search in place of
    the key search.  latents [B, C, H, W] on the device, aligns from `align.alignments` -> one TraceResult per image, or the reference's ValueError.

    One `codec.quant_pack`; then per chunk of images one `codec.rows_align` launch and one `codec.trace_keyed_topk` on its [B A] rows; then the merge of
    `trace_latents_aligned`.  The score of a (record, alignment) pair is n - 2 popcount(aligned row ^ codeword), for a fixed pair 2 X - n with
    X ~ Bin(n, 1/2) exactly under the null; the bound is `log10_p_any(log10_p_soft(score, n), U A)`.  `Candidate.agree` is the voted-bit agreement of
    the latent with the candidate's alignment applied under the candidate's own key (grouped by key, as in `trace_latents_keyed`).
    tamper_tile: as in `trace_latents_aligned`, each map under its record's own key, in the coordinates of the lattice as embedded."""
    import torch
    from . import align as AL
    limit = _log10_fpr(fpr)
    l = codec.check_window(l)
    z, shape = _aligned_lattice(latents, "trace_latents_keyed_aligned")
    cands = AL._as_list(aligns, *shape[1:])
    B = z.shape[0]
    n = z.numel() // max(B, 1)
    M, mb = registry.message_bits, registry.message_bytes
    codec.vote_copies(n, M, l)                           # (a lattice the messages do not tile fails here, as extract_batch would)
    nb = n * l
    if nb > codec.ROW_MAX_BITS:
        raise ValueError(f"a lattice of {shape} at l = {l} holds {nb} bits, more than {codec.ROW_MAX_BITS}")
    rec_dev = registry.to_device(z.device)
    signs, flags = codec.quant_pack(z, l)
    table = AL._device_table(cands, shape, z.device)
    rowbytes = signs.shape[1]

    def take(b0, b1):
        rows_b = signs[b0:b1]
        return rows_b.clone() if rows_b.data_ptr() % 16 else rows_b

    def search(rows_b, aligns_dev):
        al = codec._rows_align_launch(rows_b, shape, l, aligns_dev)
        return codec.trace_keyed_topk(al.view(-1, rowbytes), nb, rec_dev, mb, k=int(k))

    found = AL._search_chunks(B, rowbytes, table, rec_dev, k, budget_bytes, take, search, stat_bits=ALIGNED_STAT_BITS)
    U, A = len(registry), len(cands)
    reported: Dict[Tuple[bytes, bytes], List[Tuple[int, Candidate]]] = {}      # (key, nonce) -> (image, candidate)

    def candidate(b, i, s, a):
        c = Candidate(registry.user_at(i), i, s, 0, log10_p_any(log10_p_soft(s, nb), U * A), a)
        reported.setdefault(registry.record_at(i)[:2], []).append((b, c))
        return c

    out, best = _aligned_results(found, flags, cands, limit, candidate)
    for (key, nonce), pairs_ in reported.items():       # one vote per key over its (image, alignment) rows, one comparison per message
        at = {ba: r for r, ba in enumerate(sorted({(b, c.alignment) for b, c in pairs_}))}
        bits, _ = codec.extract_batch(torch.stack([AL.apply(z[b], a) for b, a in at]).contiguous(), key, nonce, M, l=l)
        by_message: Dict[bytes, List[Tuple[int, Candidate]]] = {}
        for b, c in pairs_:
            by_message.setdefault(registry.record_at(c.index)[2], []).append((b, c))
        for msg, group in by_message.items():
            agree = codec.bit_matches(bits, M, msg).cpu().numpy()
            for b, c in group:
                c.agree = int(agree[at[(b, c.alignment)]])
    if tamper_tile is not None:
        _attach_aligned_tamper_maps(out, z, cands, best, _best_records(out, registry.record_at), M, l, tamper_tile, fpr)
    return out


# ===================================================================================================================== the aligned searches ranked by reliability levels
def _aligned_soft_table(z, levels, clip, thresholds, l: int = 1):
    """(levels, P, make) of an aligned level-weighted search: the number of levels and of planes, known before anything is launched, and make() -> the float32
    table on z's device (`soft.uniform_thresholds` of the UN-aligned latents, at l = 2 and 4 `soft.window_thresholds`, or the given one)"""
    import torch
    from . import soft as S
    if thresholds is None:
        T, clip = S._check_table(levels, clip)
        return T, codec.level_planes(T), lambda: S._default_table(z, l, T, clip)
    if l == 1:
        if not isinstance(thresholds, torch.Tensor) or thresholds.dim() not in (1, 2):
            raise ValueError("thresholds must be float32 [levels] or [B, levels]")
    elif not isinstance(thresholds, torch.Tensor) or thresholds.dim() not in (2, 3) or thresholds.shape[-2] != l:
        raise ValueError(f"thresholds must be float32 [{l}, levels] or [B, {l}, levels]")
    T = int(thresholds.shape[-1])
    return T, codec.level_planes(T), lambda: thresholds.to(device=z.device, dtype=torch.float32).contiguous()


def _aligned_stack(z, pairs, thr, l: int = 1):
    """The aligned latents of (image, alignment) pairs and the threshold rows that go with them: the operands of one soft vote over the pairs"""
    import torch
    from . import align as AL
    zs = torch.stack([AL.apply(z[b], a) for b, a in pairs]).contiguous()
    shared = thr.dim() == (1 if l == 1 else 2)           # one table for all images
    return zs, thr if shared else thr[torch.tensor([b for b, _ in pairs], device=z.device)].contiguous()


def _aligned_soft_domain(shape, l: int, P: int) -> None:
    """The soft searches' domain for the rows of an aligned level-weighted search: n l (1 + P) bits of one image"""
    if shape[0] * shape[1] * shape[2] * l * (1 + P) > codec.ROW_MAX_BITS:
        at = "" if l == 1 else f" at l = {l}"
        raise ValueError(f"a lattice of {shape}{at} with {P} level planes is beyond the search's domain: n{'' if l == 1 else ' l'} (1 + P) <= {codec.ROW_MAX_BITS}")


def _trace_aligned_soft(what: str, latents, key: bytes, nonce: bytes, registry: Registry, aligns, l: int, levels: int, clip: float, thresholds,
                        message_length: Optional[int], k: int, fpr: float, tamper_tile: Optional[int], budget_bytes: Optional[int]):
    """`trace_latents_aligned_soft` (l = 1) and `trace_latents_aligned_soft_l` (l = 2, 4) after the check of l: one level packer, per chunk one launch of the
    level-weighted counts of every alignment over the n l cipher bits and one registry search, the merge, the bounds and the read-back"""
    import torch
    from . import align as AL
    from . import soft as S
    limit = _log10_fpr(fpr)
    codec._check_key_nonce(key, nonce)
    z, shape = _aligned_lattice(latents, what)
    cands = AL._as_list(aligns, *shape[1:])
    M = registry.message_bits if message_length is None else int(message_length)
    B = z.shape[0]
    rows = registry.packed(M)                            # (a message_length the registry cannot be tiled to fails here)
    V = codec.vote_copies(z.numel() // max(B, 1), M, l)
    M = codec._counts_align_message(shape, l, M)
    T, P, table_of = _aligned_soft_table(z, levels, clip, thresholds, l)
    if 2 * T * V > 2000000 or M * 2 * T * V >= 2 ** 31:
        raise ValueError(f"levels={T} with {V} copies of {M} message bits is beyond the registry search's limits "
                         "(2 levels copies <= 2 000 000 and msg_bits 2 levels copies < 2^31)")
    _aligned_soft_domain(shape, l, P)
    bias = codec._level_counts_align_limits(shape, P, M, T * V, l)
    reg_dev = registry.to_device(z.device, M)
    thr = table_of()
    lrows = codec.level_pack(z, thr) if l == 1 else codec.level_pack_l(z, thr, l)
    codec._level_rows_align_checks(lrows, shape, l)
    table = AL._device_table(cands, shape, z.device)

    def search(rows_b, aligns_dev):
        counts = codec._level_counts_align_launch(rows_b, shape, aligns_dev, key, nonce, M, bias, l=l)
        idx, score = codec.trace_topk(counts.view(-1, M), 2 * T * V, reg_dev, k=int(k), soft=True)
        return idx, torch.where(idx >= 0, score // 2, score)             # the search weighs 2 score[b, a, t]: every score is even

    found = AL._search_chunks(B, 4 * M, table, reg_dev, k, budget_bytes, lambda b0, b1: codec.LevelRows(*(t[b0:b1] for t in lrows)), search,
                              stat_bits=AL.SOFT_STAT_BITS)
    U, A = len(registry), len(cands)
    wsq_h = lrows.wsq.cpu().numpy()
    reported: List[Tuple[int, Candidate]] = []          # (image, candidate), in order

    def candidate(b, i, s, a):
        c = Candidate(registry.user_at(i), i, s, 0, log10_p_any(S.log10_p(s, int(wsq_h[b])), U * A), a)
        reported.append((b, c))
        return c

    out, best = _aligned_results(found, lrows.flags, cands, limit, candidate)
    if reported:                                        # the soft vote of every reported pair on its aligned latent, one launch
        zs, thr_rows = _aligned_stack(z, [(b, c.alignment) for b, c in reported], thr, l)
        vote = S.extract_soft_l(zs, key, nonce, M, l, thresholds=thr_rows)                # (l = 1: `soft.extract_soft`, to which it delegates)
        for (_, c), row in zip(reported, vote.bits.cpu().numpy()):
            c.agree = M - int(np.unpackbits(row ^ rows[c.index]).sum())
    if tamper_tile is not None:
        _attach_aligned_tamper_maps(out, z, cands, best, _best_records(out, lambda i: (key, nonce, bytes(rows[i]))), M, l, tamper_tile, fpr)
    return out


def trace_latents_aligned_soft(latents, key: bytes, nonce: bytes, registry: Registry, aligns, *, levels: int = 15, clip: float = 2.5, thresholds=None,
                               message_length: Optional[int] = None, k: int = 1, fpr: float = 1e-6, tamper_tile: Optional[int] = None,
                               budget_bytes: Optional[int] = None) -> List[Union[TraceResult, ValueError]]:
    """`trace_latents_aligned` ranked by reliability levels (one cipher bit per element): the search runs over every (record,
    alignment) pair and every lattice element votes with an integer level 0..levels taken from its magnitude.  latents [B, C, H, W] on the device, aligns
    from `align.alignments` -> one TraceResult per image (best candidate first), or the reference's ValueError for a NaN / saturated latent.

    thresholds: float32 [levels] or [B, levels]; None: `soft.uniform_thresholds(latents, levels, clip)`, taken ONCE on the un-aligned latents (an alignment
    permutes the elements, so their levels travel with them).  One `codec.level_pack`; then per chunk of images one `codec.level_counts_align` launch with
    bias = levels V -- its output is already the counts' of `reliability_counts` -- and one `codec.trace_topk(counts', 2 levels V)`, whose scores are halved
    as in `trace_latents(reliability=)`; then `trace_latents_aligned`'s merge.  The cuts follow `budget_bytes` with 4 M bytes per aligned image; the result
    does not depend on them.  The limits are `reliability_counts`', raised before any launch.
    The score of a pair is sum_t (2 r_t - 1) score[t] of `soft.extract_soft(align.apply(latent, alignment))`.  For a FIXED pair and an image independent of
    the key the decrypted bits are fair coins given the levels, so Hoeffding's bound `soft.log10_p(score, wsq)` holds with the image's own wsq (a permutation
    keeps it); the reported bound is Bonferroni over the U A pairs.  A bound, not the exact tail of `trace_latents_aligned`.
    `Candidate.agree`: the soft vote's bits of the latent with that alignment applied, one `soft.extract_soft` launch over the reported (image, alignment)
    rows, each with its image's own threshold row.  tamper_tile: as in `trace_latents_aligned`, on the sign row of the un-aligned latent."""
    return _trace_aligned_soft("trace_latents_aligned_soft", latents, key, nonce, registry, aligns, 1, levels, clip, thresholds, message_length, k, fpr,
                               tamper_tile, budget_bytes)


def trace_latents_aligned_soft_l(latents, key: bytes, nonce: bytes, registry: Registry, aligns, l: int, *, levels: int = 15, clip: float = 2.5,
                                 thresholds=None, message_length: Optional[int] = None, k: int = 1, fpr: float = 1e-6, tamper_tile: Optional[int] = None,
                                 budget_bytes: Optional[int] = None) -> List[Union[TraceResult, ValueError]]:
    """`trace_latents_aligned_soft` for multi-bit windows (l = 2 or 4): the search runs over every (record, alignment) pair and every
    one of the n l cipher bits votes with its level 0..levels of `codec.extract_soft_l`.  latents [B, C, H, W] on the device, aligns from `align.alignments`.

    thresholds: float32 [l, levels] or [B, l, levels]; None: `soft.window_thresholds(latents, l, levels, clip)`, taken ONCE on the un-aligned latents (an
    alignment permutes elements, and the l level bits of an element travel with it).  One `codec.level_pack_l`; then per chunk of images one
    `codec.level_counts_align_l` launch with bias = levels V, V = n l / M, and one `codec.trace_topk(counts', 2 levels V)`; then `trace_latents_aligned`'s
    merge.  The limits are `reliability_counts`', n l (1 + P) <= 1 048 576 and `codec.level_counts_align_l`'s LDS cap, all raised before any launch.
    The bound is `trace_latents_aligned_soft`'s: Hoeffding's `soft.log10_p(score, wsq)` with the image's own wsq over its n l bits, Bonferroni over the U A
    pairs.  `Candidate.agree`: the bits of `soft.extract_soft_l` on the latent with that alignment applied, one launch over the reported pairs.  tamper_tile: as
    in `trace_latents_aligned` at that l.  l = 1 is refused: that is `trace_latents_aligned_soft`."""
    l = codec._multi_bit_window(l, "trace_latents_aligned_soft")
    return _trace_aligned_soft("trace_latents_aligned_soft_l", latents, key, nonce, registry, aligns, l, levels, clip, thresholds, message_length, k, fpr,
                               tamper_tile, budget_bytes)


def _trace_keyed_aligned_soft(what: str, latents, registry: KeyedRegistry, aligns, l: int, levels: int, clip: float, thresholds, k: int, fpr: float,
                              tamper_tile: Optional[int], budget_bytes: Optional[int]):
    """`trace_latents_keyed_aligned_soft` (l = 1) and `trace_latents_keyed_aligned_soft_l` (l = 2, 4) after the check of l: one level packer, per chunk one
    launch of every alignment of the 1 + P rows of n l bits and one keyed soft search, the merge, the bounds and the read-back"""
    import torch
    from . import align as AL
    from . import soft as S
    limit = _log10_fpr(fpr)
    z, shape = _aligned_lattice(latents, what)
    cands = AL._as_list(aligns, *shape[1:])
    B = z.shape[0]
    n = z.numel() // max(B, 1)
    M, mb = registry.message_bits, registry.message_bytes
    codec.vote_copies(n, M, l)                           # (a lattice the messages do not tile fails here, as extract_batch would)
    T, P, table_of = _aligned_soft_table(z, levels, clip, thresholds, l)
    _aligned_soft_domain(shape, l, P)
    rec_dev = registry.to_device(z.device)
    thr = table_of()
    lrows = codec.level_pack(z, thr) if l == 1 else codec.level_pack_l(z, thr, l)
    codec._level_rows_align_checks(lrows, shape, l)
    table = AL._device_table(cands, shape, z.device)
    rowbytes = lrows.signs.shape[1]

    def search(rows_b, aligns_dev):
        signs, planes = codec._level_rows_align_launch(rows_b, shape, aligns_dev, l)
        al = codec.LevelRows(signs.view(-1, rowbytes), planes.view(-1, P, rowbytes), rows_b.wsum.repeat_interleave(aligns_dev.shape[0]), rows_b.wsq, rows_b.flags)
        return codec.trace_keyed_soft_topk(al, n * l, rec_dev, mb, k=int(k))

    found = AL._search_chunks(B, (1 + P) * rowbytes, table, rec_dev, k, budget_bytes, lambda b0, b1: codec.LevelRows(*(t[b0:b1] for t in lrows)), search,
                              stat_bits=AL.SOFT_STAT_BITS)
    U, A = len(registry), len(cands)
    wsq_h = lrows.wsq.cpu().numpy()
    reported: List[Tuple[int, Candidate]] = []          # (image, candidate), in order

    def candidate(b, i, s, a):
        c = Candidate(registry.user_at(i), i, s, 0, log10_p_any(S.log10_p(s, int(wsq_h[b])), U * A), a)
        reported.append((b, c))
        return c

    out, best = _aligned_results(found, lrows.flags, cands, limit, candidate)
    if reported:                                        # the soft vote of every reported pair under the candidate's own record, one launch
        zs, thr_rows = _aligned_stack(z, [(b, c.alignment) for b, c in reported], thr, l)
        rec = torch.tensor([c.index for _, c in reported], device=z.device)
        pairs_ = (zs, rec_dev[rec].contiguous(), mb, thr_rows)
        vote = codec.extract_soft(*pairs_) if l == 1 else codec.extract_soft_l(*pairs_, l)
        for (_, c), a in zip(reported, vote.matches.cpu().tolist()):
            c.agree = int(a)
    if tamper_tile is not None:
        _attach_aligned_tamper_maps(out, z, cands, best, _best_records(out, registry.record_at), M, l, tamper_tile, fpr)
    return out


def trace_latents_keyed_aligned_soft(latents, registry: KeyedRegistry, aligns, *, levels: int = 15, clip: float = 2.5, thresholds=None, k: int = 1,
                                     fpr: float = 1e-6, tamper_tile: Optional[int] = None,
                                     budget_bytes: Optional[int] = None) -> List[Union[TraceResult, ValueError]]:
    """`trace_latents_keyed_aligned` ranked by reliability levels (one cipher bit per element): `trace_latents_keyed_soft` over every
    (record, alignment) pair.  latents [B, C, H, W] on the device, aligns from `align.alignments` -> one TraceResult per image, or the reference's ValueError.

    thresholds as in `trace_latents_aligned_soft`.  One `codec.level_pack`; then per chunk of images one `codec.level_rows_align` launch and one
    `codec.trace_keyed_soft_topk` on its [B A] rows (wsum repeated: a permutation keeps it); then `trace_latents_aligned`'s merge, with (1 + P) rows counted
    per aligned image against `budget_bytes`.  No kernel of its own.  The score of a pair is sum_j level_j (1 - 2 (sign_j ^ codeword_j)) of the aligned
    rows; the bound is `log10_p_any(soft.log10_p(score, wsq), U A)`, Hoeffding's with the image's wsq for a fixed pair, Bonferroni over the pairs.
    `Candidate.agree` counts the bits of the soft vote of the aligned latent under the candidate's own record: one `codec.extract_soft` launch over the
    reported (image, candidate) pairs.  tamper_tile: as in `trace_latents_keyed_aligned`.  n (1 + P) may not exceed 1 048 576, P the bit length of `levels`."""
    return _trace_keyed_aligned_soft("trace_latents_keyed_aligned_soft", latents, registry, aligns, 1, levels, clip, thresholds, k, fpr, tamper_tile, budget_bytes)


def trace_latents_keyed_aligned_soft_l(latents, registry: KeyedRegistry, aligns, l: int, *, levels: int = 15, clip: float = 2.5, thresholds=None, k: int = 1,
                                       fpr: float = 1e-6, tamper_tile: Optional[int] = None,
                                       budget_bytes: Optional[int] = None) -> List[Union[TraceResult, ValueError]]:
    """`trace_latents_keyed_aligned_soft` for multi-bit windows (l = 2 or 4): `trace_latents_keyed_soft_l` over every (record,
    alignment) pair.  latents [B, C, H, W] on the device, aligns from `align.alignments`.

    thresholds as in `trace_latents_aligned_soft_l`.  One `codec.level_pack_l`; then per chunk of images one `codec.level_rows_align_l` launch and the unchanged
    `codec.trace_keyed_soft_topk` on its [B A] rows with n_bits = n l; then `trace_latents_aligned`'s merge.  The bound is
    `log10_p_any(soft.log10_p(score, wsq), U A)`.  `Candidate.agree`: one `codec.extract_soft_l` launch over the reported (image, candidate) pairs.
    tamper_tile: as in `trace_latents_keyed_aligned` at that l.  n l (1 + P) may not exceed 1 048 576.  l = 1 is refused: that is
    `trace_latents_keyed_aligned_soft`."""
    l = codec._multi_bit_window(l, "trace_latents_keyed_aligned_soft")
    return _trace_keyed_aligned_soft("trace_latents_keyed_aligned_soft_l", latents, registry, aligns, l, levels, clip, thresholds, k, fpr, tamper_tile, budget_bytes)


# ===================================================================================================================== tracing a SET of images to one user
@dataclass
class SetTraceResult:
    candidates: List[Candidate] = field(default_factory=list)   # best first; `score` is the pooled score, the sum of the record's scores over the set's images
    attributed: Optional[str] = None       # the best candidate's user id if its bound is <= log10(fpr), else None
    size: int = 0                          # images pooled
    skipped: int = 0                       # images of the set left out: NaN / saturated latents
    wsq: int = 0                           # sum_j S_j^2 of the pooled row: what Hoeffding's bound divides by


def _pool_levels(levels, l: int) -> Tuple[int, int]:
    """(levels, l) of a pooled trace, or ValueError: levels = 0 pools `quant_pack` rows at l = 1, 2, 4; levels in 1..15 pools `level_pack` rows, l = 1 only"""
    l = codec.check_window(l)
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 0 <= int(levels) <= codec.SOFT_MAX_LEVELS:
        raise ValueError(f"levels must be 0 (unit levels) or an int in 1..{codec.SOFT_MAX_LEVELS}, got {levels!r}")
    if int(levels) and l != 1:
        raise ValueError(f"levels = {levels} cannot be combined with l = {l}: pooled reliability levels are defined for one cipher bit per element (l = 1)")
    return int(levels), l


def _pool_pack(z, levels: int, clip: float, l: int):
    """The rows a pooled trace adds up, packed once per image -> (signs [B, n l / 8], planes [B, P, n l / 8] or None, flags on the host)"""
    if levels == 0:
        signs, flags = codec.quant_pack(z, l)
        return signs, None, flags.cpu().numpy()
    from . import soft as S
    rows = codec.level_pack(z, S.uniform_thresholds(z, levels, clip))      # thresholds per image: a level means the same share of every image's range
    return rows.signs, rows.planes, rows.flags.cpu().numpy()


def _unpack_bits(rows):
    """uint8 [..., n / 8] on the device -> int64 [..., n], MSB first"""
    import torch
    shifts = torch.arange(7, -1, -1, device=rows.device, dtype=torch.int64)
    return ((rows.to(torch.int64)[..., None] >> shifts) & 1).reshape(*rows.shape[:-1], rows.shape[-1] * 8)


def _pooled_agree(pooled, row: int, record: Tuple[bytes, bytes, bytes]) -> int:
    """Message bits of the pooled level-weighted vote under the record's own key that equal its message: torch ops over one pooled row"""
    import torch
    key, nonce, msg = record
    signs = pooled.signs[row]
    S = _unpack_bits(pooled.planes[row])                                    # [Q, n]
    level = (S << torch.arange(S.shape[0], device=S.device, dtype=torch.int64)[:, None]).sum(dim=0)
    d = _unpack_bits(signs) ^ _unpack_bits(codec.keystream(key, nonce, signs.shape[0], device=signs.device))
    vote = (level * (2 * d - 1)).reshape(-1, 8 * len(msg)).sum(dim=0)      # position j votes for message bit j mod M
    want = _unpack_bits(torch.frombuffer(bytearray(msg), dtype=torch.uint8).to(signs.device))
    return int(((vote > 0).to(torch.int64) == want).sum())


def _trace_pooled(signs, planes, flags_h, sets, registry: KeyedRegistry, k: int, fpr: float) -> list:
    """Packed rows of B images, the sets as lists of image indices -> one SetTraceResult per set (or the ValueError of a set left empty): gather the
    unflagged images set by set, one `codec.pool_rows` launch, one `codec.trace_keyed_pooled_topk` launch, the candidates"""
    import torch
    from . import soft as S
    limit = _log10_fpr(fpr)
    B, n_bits, U = signs.shape[0], signs.shape[1] * 8, len(registry)
    out: list = [None] * len(sets)
    live = []                                            # (set, its unflagged images, how many were left out)
    for g, members in enumerate(sets):
        members = [int(b) for b in members]
        if not members:
            raise ValueError(f"set {g} is empty: a set holds at least one image")
        if min(members) < 0 or max(members) >= B:
            raise IndexError(f"set {g} names image {min(members) if min(members) < 0 else max(members)}, the batch holds {B}")
        kept = [b for b in members if _flag_error(int(flags_h[b])) is None]
        if kept:
            live.append((g, kept, len(members) - len(kept)))
        else:
            out[g] = _flag_error(int(flags_h[members[0]]))
    if not live:
        return out
    order = torch.tensor([b for _, kept, _ in live for b in kept], device=signs.device)
    pooled = codec.pool_rows(signs[order], planes[order] if planes is not None else None, [len(kept) for _, kept, _ in live])
    idx, score = codec.trace_keyed_pooled_topk(pooled, n_bits, registry.to_device(signs.device), registry.message_bytes, k=k)
    idx_h, score_h = _pairs_to_host(idx, score)
    wsq_h = pooled.wsq.cpu().numpy()
    for row, (g, kept, skipped) in enumerate(live):
        wsq, found = int(wsq_h[row]), []
        for j in range(idx_h.shape[1]):
            i = int(idx_h[row, j])
            if i < 0:
                break
            s = int(score_h[row, j])
            found.append(Candidate(registry.user_at(i), i, s, _pooled_agree(pooled, row, registry.record_at(i)), log10_p_any(S.log10_p(s, wsq), U)))
        out[g] = SetTraceResult(found, found[0].user_id if found and found[0].log10_p_any <= limit else None, len(kept), skipped, wsq)
    return out


def trace_sets_keyed(latents, sets, keyed_registry: KeyedRegistry, *, levels: int = 0, clip: float = 2.5, k: int = 1, fpr: float = 1e-6,
                     l: int = 1) -> List[Union[SetTraceResult, ValueError]]:
    """Trace SETS of images to one user each, pooling the evidence of a set's images: latents [B, ...] on the device, sets a
    list of lists of image indices (an image may appear in several sets) -> one SetTraceResult per set.

    Every keyed score is linear in the image, so the sum of a record's scores over a set is its score against one pooled row: `codec.pool_rows` adds
    the set's packed rows into S_j = sum_b lev_bj (1 - 2 h_bj), `codec.trace_keyed_pooled_topk` walks the records ONCE per set whatever its size.
    levels = 0 pools `codec.quant_pack` rows (unit levels; l = 1, 2 or 4), levels in 1..15 pools `codec.level_pack` rows under
    `soft.uniform_thresholds(latents, levels, clip)` taken per image (l = 1 only).
    The p-value is Hoeffding's bound `soft.log10_p(score, wsq)` with wsq = sum_j S_j^2, Bonferroni over the records.  It conditions on the images: a
    record whose key they are independent of has a uniform codeword, so the pooled score is sum_j +-|S_j| with fair signs -- whatever the dependence
    BETWEEN the images (eight copies of one image carry that image's own bound, not eight times its evidence; Bin(n |set|, 1/2) would be wrong).
    The sets are the caller's choice, made before looking at scores: trying several groupings costs Bonferroni over them.
    Images flagged NaN or saturated are left out of their set and counted in `skipped`; a set left empty gets the reference's ValueError for such an
    image.  `Candidate.agree` counts the message bits of the pooled level-weighted vote under the candidate's own key (torch ops over the reported
    rows).  A set holds at most 1023 images at unit levels and 1023 // (2**P - 1) at `levels` of P bits (68 at 15): ValueError beyond."""
    levels, l = _pool_levels(levels, l)
    _log10_fpr(fpr)
    z = latents.contiguous()
    B = z.shape[0]
    codec.vote_copies(z.numel() // max(B, 1), keyed_registry.message_bits, l)   # (a lattice the messages do not tile fails here, as extract_batch would)
    signs, planes, flags_h = _pool_pack(z, levels, clip, l)
    return _trace_pooled(signs, planes, flags_h, sets, keyed_registry, k, fpr)


def keyed_from_shared(registry: Registry, key: bytes, nonce: bytes, message_length: Optional[int] = None) -> KeyedRegistry:
    """The shared-key registry as keyed records: `key | nonce` in front of every message, same order, same user ids"""
    M = registry.message_bits if message_length is None else int(message_length)
    rows = registry.packed(M)
    keyed = KeyedRegistry(M // 8)
    for i in range(len(registry)):
        keyed.add(registry.user_at(i), key, nonce, bytes(rows[i]))
    return keyed


def trace_sets(latents, sets, key: bytes, nonce: bytes, registry: Registry, *, message_length: Optional[int] = None, levels: int = 0, clip: float = 2.5,
               k: int = 1, fpr: float = 1e-6, l: int = 1) -> List[Union[SetTraceResult, ValueError]]:
    """`trace_sets_keyed` for a registry whose users share one key: `key | nonce` is written in front of every message (`keyed_from_shared`) and the keyed
    form runs.  For records that share a key the scores are the same numbers as a vote-based search would give, and with a few sets the record walk
    is milliseconds against 2^20 records: there is no kernel path of its own."""
    return trace_sets_keyed(latents, sets, keyed_from_shared(registry, key, nonce, message_length), levels=levels, clip=clip, k=k, fpr=fpr, l=l)


# ===================================================================================================================== front end
def format_set_line(name: str, result) -> str:
    """One line per set of trace.txt / stdout, after the per-image lines: name, images, skipped, user or none, bound, score"""
    if isinstance(result, Exception):
        return f"set {name}, Error: {result}"
    head = f"set {name}, images, {result.size}, skipped, {result.skipped}, user: {result.attributed if result.attributed is not None else 'none'}"
    if not result.candidates:
        return head + ", log10 p, 0.0, score, nan"
    c = result.candidates[0]
    text = head + f", log10 p, {c.log10_p_any:.3f}, score, {c.score}"
    for o in result.candidates[1:]:
        text += f", next: {o.user_id} ({o.log10_p_any:.3f}, {o.score})"
    return text


class _PoolStore:
    """The packed rows of every traced image of a run, kept across device batches for --pool: file -> (sign row, plane rows or None, flags)"""

    def __init__(self, args, registry):
        self.levels = int(args.pool_reliability or 0)
        self.l, self.k, self.fpr = int(args.l), int(args.top), float(args.fpr)
        self.rows: Dict[str, tuple] = {}
        self.registry = registry if args.per_record_keys else keyed_from_shared(registry, args.key, args.nonce, args.message_length)

    def add(self, files: Sequence[str], latents) -> None:
        signs, planes, flags_h = _pool_pack(latents.contiguous(), self.levels, 2.5, self.l)
        for r, f in enumerate(files):
            self.rows[f] = (signs[r], planes[r] if planes is not None else None, int(flags_h[r]))

    def drop(self, f: str) -> None:
        self.rows.pop(f, None)

    def trace(self, named_sets: Sequence[Tuple[str, Sequence[str]]]) -> List[Tuple[str, object]]:
        """(name, files) per set -> (name, SetTraceResult or the exception) per set that has any traced image"""
        import torch
        files = [f for f in dict.fromkeys(f for _, fs in named_sets for f in fs) if f in self.rows]
        at = {f: i for i, f in enumerate(files)}
        named = [(name, [at[f] for f in fs if f in at]) for name, fs in named_sets]
        named = [(name, members) for name, members in named if members]
        if not named:
            return []
        signs = torch.stack([self.rows[f][0] for f in files])
        planes = torch.stack([self.rows[f][1] for f in files]) if self.levels else None
        flags_h = np.array([self.rows[f][2] for f in files])
        try:
            results = _trace_pooled(signs, planes, flags_h, [m for _, m in named], self.registry, self.k, self.fpr)
        except Exception:                                # (a set beyond the pooling limits): redone set by set so that each reports its own error
            results = []
            for _, members in named:
                try:
                    results += _trace_pooled(signs, planes, flags_h, [members], self.registry, self.k, self.fpr)
                except Exception as e:
                    results.append(e)
        return [(name, r) for (name, _), r in zip(named, results)]


def format_line(name: str, result, message_length: int) -> str:
    """One line of trace.txt / stdout"""
    if isinstance(result, Exception):
        return f"Error processing {name}: {result}"
    if not result.candidates:
        return f"{name}, user: none, agreement, nan, log10 p, 0.0"
    c = result.candidates[0]
    text = f"{name}, user: {result.attributed if result.attributed is not None else 'none'}, agreement, {c.agree / message_length}, log10 p, {c.log10_p_any:.3f}"
    for o in result.candidates[1:]:
        text += f", next: {o.user_id} ({o.agree / message_length}, {o.log10_p_any:.3f})"
    if result.tamper is not None:
        text += f", intact tiles {result.tamper.n_intact}/{result.tamper.n_tiles}"
    if result.alignment is not None:
        from . import align as AL
        text += f", alignment: {AL.describe(result.alignment)}"
    return text


def build_parser():
    import argparse

    class Parser(argparse.ArgumentParser):
        def parse_args(self, args=None, namespace=None):
            a = super().parse_args(args, namespace)
            if a.ecc is not None:                                   # the registries hold CODED messages and are searched as they are: the payload read is extract's and detect's
                if a.pool is not None:
                    self.error("--ecc cannot be combined with --pool yet: the payload read is not wired through pooled sets")
                if a.align != "none":
                    self.error("--ecc cannot be combined with --align yet: the payload read is not wired through the alignment search")
                self.error("--ecc is not a trace flag: registry rows hold the coded message and are matched unchanged; read payloads with extract --ecc conv "
                           "or detect --ecc conv")
            if a.pool_reliability is not None:
                if a.pool is None:
                    self.error("--pool_reliability requires --pool all or --pool subdirs: it sets the reliability levels of the rows a pooled trace adds up")
                if a.l != 1:
                    self.error(f"--pool_reliability cannot be combined with --l {a.l}: pooled reliability levels are defined for one cipher bit per "
                               "element (--l 1); --pool alone pools the --l rows at unit levels")
            if a.pool is not None:
                if a.hard:
                    self.error("--pool cannot be combined with --hard: pooled evidence is a sum of margins, the majority-voted bits do not add up")
                if a.align != "none":
                    self.error("--pool cannot be combined with --align: alignment searches inside a set are out of scope")
                if a.tamper_map:
                    self.error("--pool cannot be combined with --tamper_map: a tamper map belongs to one image")
                if a.pool == "subdirs" and str(a.is_traverse_subdirectories) != "1":
                    self.error("--pool subdirs needs --is_traverse_subdirectories 1: its sets are the directories that traversal visits")
            if a.align_window_reliability is not None:
                if a.align == "none":
                    self.error("--align_window_reliability requires --align flips or --align d4: it ranks the (record, alignment) pairs of an aligned search at "
                               "--l 2 or 4 (without alignments: --window_reliability with --per_record_keys)")
                if a.l == 1:
                    self.error("--align_window_reliability needs --l 2 or --l 4: at --l 1 the level-weighted trace through alignments is --align_reliability")
                if a.hard:
                    self.error("--align_window_reliability cannot be combined with --hard: the level-weighted statistic ranks by weighted margins")
                for name in ("reliability", "keyed_reliability", "window_reliability", "align_reliability", "pool"):
                    if getattr(a, name) is not None:
                        self.error(f"--align_window_reliability cannot be combined with --{name}")
            if a.align_reliability is not None:
                if a.align == "none":
                    self.error("--align_reliability requires --align flips or --align d4: it ranks the (record, alignment) pairs of an aligned search "
                               "(without alignments: --reliability, or --keyed_reliability with --per_record_keys)")
                if a.hard:
                    self.error("--align_reliability cannot be combined with --hard: the level-weighted statistic ranks by weighted margins")
                if a.l != 1:
                    self.error(f"--align_reliability cannot be combined with --l {a.l}: reliability levels under alignments are defined for one cipher bit "
                               "per element (--l 1)")
                for name in ("reliability", "keyed_reliability", "window_reliability"):
                    if getattr(a, name) is not None:
                        self.error(f"--align_reliability cannot be combined with --{name}: --{name} is the same statistic without alignments")
            if a.align != "none":
                for name in ("reliability", "keyed_reliability", "window_reliability"):
                    if getattr(a, name) is not None:
                        self.error(f"--align cannot be combined with --{name}: the level-weighted trace through alignments is --align_reliability (--l 1)")
            if a.align_shift < 0 or (a.align == "none" and a.align_shift):
                self.error("--align_shift is a non-negative number of lattice steps and needs --align flips or --align d4")
            if a.keyed_reliability is not None:
                if not a.per_record_keys:
                    self.error("--keyed_reliability requires --per_record_keys: it ranks a registry whose records carry their own keys "
                               "(one key for all users: --reliability)")
                if a.hard:
                    self.error("--keyed_reliability cannot be combined with --hard: the level-weighted statistic ranks by weighted margins")
                if a.reliability is not None:
                    self.error("--keyed_reliability cannot be combined with --reliability: --reliability is the shared-key form of the same statistic")
                if a.l != 1:
                    self.error(f"--keyed_reliability cannot be combined with --l {a.l}: reliability levels are defined for one cipher bit per element (--l 1)")
            if a.window_reliability is not None:
                if not a.per_record_keys:
                    self.error("--window_reliability requires --per_record_keys: it ranks a registry whose records carry their own keys")
                if a.l == 1:
                    self.error("--window_reliability needs --l 2 or --l 4: at --l 1 the level-weighted search across keys is --keyed_reliability")
                if a.hard:
                    self.error("--window_reliability cannot be combined with --hard: the level-weighted statistic ranks by weighted margins")
                if a.reliability is not None or a.keyed_reliability is not None:
                    self.error("--window_reliability cannot be combined with --reliability or --keyed_reliability: those are the --l 1 forms of the statistic")
                if a.tamper_map:
                    self.error("--window_reliability cannot be combined with --tamper_map")
            if a.reliability is not None:
                if a.hard:
                    self.error("--reliability cannot be combined with --hard: the level-weighted statistic ranks by weighted margins")
                if a.per_record_keys:
                    self.error("--reliability cannot be combined with --per_record_keys: the level-weighted search across keys is --keyed_reliability")
                if a.l != 1:
                    self.error(f"--reliability cannot be combined with --l {a.l}: reliability levels are defined for one cipher bit per element (--l 1)")
            if a.per_record_keys:
                if a.hard:
                    self.error("--hard cannot be combined with --per_record_keys: only the soft statistic exists across keys")
                if a.key_hex is not None or a.nonce_hex is not None:
                    self.error("--per_record_keys takes every key and nonce from the registry: drop --key_hex / --nonce_hex")
            elif a.key_hex is None or a.nonce_hex is None:
                self.error("the following arguments are required: --key_hex, --nonce_hex (or --per_record_keys with a registry that carries them)")
            return a

    p = Parser(prog="python -m gswm_amd.trace",
               description="Trace images to the registered user whose watermark they carry (single GPU; one key for all users, or per-user keys "
                           "with --per_record_keys: the log gs_insert writes when key and nonce are left blank; sharding over --gpus is out of "
                           "scope of this tool)")
    p.add_argument("--model_id", default="stabilityai/stable-diffusion-2-1-base")
    p.add_argument("--images_directory_path", default="", help="The path of directory containing images to process")
    p.add_argument("--single_image_path", default="")
    p.add_argument("--key_hex", default=None, help="Hexadecimal key used for encryption (required unless --per_record_keys)")
    p.add_argument("--nonce_hex", default=None, help="Hexadecimal nonce used for encryption, It will use the fixed part of the key if nonce is none "
                                                     "(required unless --per_record_keys)")
    p.add_argument("--registry", required=True, help="registry file: 'user_id<TAB>message_hex' lines, or the info_data.txt log gs_insert appends "
                                                      "(told apart by the first line; of a log, the records of this key / nonce are used)")
    p.add_argument("--per_record_keys", action="store_true",
                   help="every record of --registry carries its own key and nonce: ALL records of an info_data.txt log, or "
                        "'user_id<TAB>key_hex<TAB>nonce_hex<TAB>message_hex' lines (soft statistic only)")
    p.add_argument("--fpr", type=float, default=1e-6, help="false-positive rate per image, over the whole registry (Bonferroni)")
    p.add_argument("--top", type=int, default=1, choices=range(1, 9), metavar="K", help="candidates reported per image (1..8)")
    p.add_argument("--hard", action="store_true", help="rank by the majority-voted bits instead of the vote margins")
    p.add_argument("--reliability", type=int, default=None, choices=range(1, 16), metavar="LEVELS",
                   help="rank by level-weighted margins: every lattice element votes with one of LEVELS (1..15) reliability levels taken from its "
                        "magnitude, the p-value is a Hoeffding bound (shared key, --l 1, not with --hard)")
    p.add_argument("--keyed_reliability", type=int, default=None, choices=range(1, 16), metavar="LEVELS",
                   help="with --per_record_keys: rank by level-weighted margins across keys, LEVELS (1..15) reliability levels per lattice element, "
                        "the p-value is a Hoeffding bound (--l 1, not with --hard or --reliability)")
    p.add_argument("--window_reliability", type=int, default=None, choices=range(1, 16), metavar="LEVELS",
                   help="with --per_record_keys and --l 2 or 4: rank by level-weighted margins across keys, every cipher bit of a lattice element "
                        "votes with one of LEVELS (1..15) levels taken from its distance to the quantiser boundaries that would flip it, the p-value is "
                        "a Hoeffding bound (not with --hard, --reliability, --keyed_reliability or --tamper_map)")
    p.add_argument("--num_inference_steps", default=30, type=int, help="Number of inference steps for the model")
    p.add_argument("--scheduler", default="DDIM", help="Choose a scheduler between 'DPMs' and 'DDIM' to inverse the image")
    p.add_argument("--is_traverse_subdirectories", default=0, help="Whether to traverse subdirectories recursively")
    p.add_argument("--width", type=int, default=1024, help="Width of the input image")
    p.add_argument("--height", type=int, default=1024, help="Height of the input image")
    p.add_argument("--message_length", type=int, default=None, help="Length of the message in bits (default: the registry's own length; a multiple of it "
                                                                     "repeats the registered messages, which weakens --hard)")
    p.add_argument("--l", type=int, default=1, choices=codec.WINDOWS, help="cipher bits per lattice element the images were embedded with")
    p.add_argument("--allow_synthetic_weights", action="store_true", help="run without a checkpoint (pipeline tests / benchmarks only)")
    p.add_argument("--batch_size", type=int, default=16, help="images per device batch")
    p.add_argument("--tamper_map", default=None, metavar="DIR",
                   help="for every attributed image write DIR/<image>.tamper.npy (agreeing bits per tile with the attributed record's codeword) and "
                        "DIR/<image>.tamper.png (255 where the watermark's presence in the tile is proven at --fpr over the map), and report the intact tiles")
    p.add_argument("--tile", type=int, default=8, choices=codec.TILES, help="tile edge of --tamper_map, in lattice elements (one element = 8 x 8 pixels)")
    p.add_argument("--align", default="none", choices=("none", "flips", "d4"),
                   help="search every (record, alignment) pair over this group of alignments of the lattice: flips (half turn and the two mirrors) or d4 (all "
                        "eight orientations); the Bonferroni factor grows by the number of candidates (not with --reliability, --keyed_reliability or "
                        "--window_reliability); with --tamper_map the map is in the coordinates of the lattice as embedded")
    p.add_argument("--align_shift", type=int, default=0, metavar="R", help="with --align: also every lattice shift in [-R, R]^2 (8 R pixels)")
    p.add_argument("--align_reliability", type=int, default=None, choices=range(1, 16), metavar="LEVELS",
                   help="with --align flips or d4: rank the (record, alignment) pairs by level-weighted margins, LEVELS (1..15) reliability levels per lattice "
                        "element, the p-value is a Hoeffding bound over the pairs (with or without --per_record_keys; --l 1, not with --hard, --reliability, "
                        "--keyed_reliability or --window_reliability)")
    p.add_argument("--align_window_reliability", type=int, default=None, choices=range(1, 16), metavar="LEVELS",
                   help="with --align flips or d4 and --l 2 or 4: rank the (record, alignment) pairs by level-weighted margins, every cipher bit of a lattice "
                        "element votes with one of LEVELS (1..15) levels taken from its distance to the quantiser boundaries that would flip it, the p-value "
                        "is a Hoeffding bound over the pairs (with or without --per_record_keys, with --tamper_map; not with --hard, --reliability, "
                        "--keyed_reliability, --window_reliability, --align_reliability or --pool)")
    p.add_argument("--pool", default=None, choices=("all", "subdirs"),
                   help="after the per-image lines, trace SETS of images by pooled evidence, one line per set: all (every traced image is one set) or subdirs "
                        "(one set per directory; needs --is_traverse_subdirectories 1).  The sets are chosen before looking at scores; at most 1023 images per "
                        "set (not with --hard, --align or --tamper_map)")
    p.add_argument("--pool_reliability", type=int, default=None, choices=range(1, 16), metavar="LEVELS",
                   help="with --pool: pool rows of LEVELS (1..15) reliability levels per lattice element instead of unit levels; a set then holds at most "
                        "1023 // (2^P - 1) images, P the bit length of LEVELS (68 at 15) (--l 1)")
    p.add_argument("--ecc", default=None, choices=("conv", "conv23", "conv34"),
                   help="refused by name: messages issued with --ecc conv are registered CODED and traced unchanged; with --pool or --align the payload read is "
                        "not wired yet (extract --ecc conv and detect --ecc conv read payloads)")
    p.add_argument("--strict_kernels", type=int, choices=[0, 1], default=None,
                   help="1: raise when a GPU half-precision call would leave the hand-written kernels instead of warning (default: 1)")
    return p


def _trace_files(files: Sequence[str], args, registry, trace_batch=None, store=None) -> list:
    """files -> outcomes in order (TraceResult or the exception that file raised): decode on host threads, invert and trace in device
    batches; a batch that raises is redone image by image so that each reports its own error (extract._recover_items does the same).
    trace_batch: None, or what to do with a batch of inverted latents instead of the registry search (`detect` runs its key search here).
    store: None, or the `_PoolStore` that keeps every traced image's packed rows for --pool (a file that raises keeps none)."""
    from concurrent.futures import ThreadPoolExecutor
    from . import extract as X

    def decode(f):
        try:
            return X.decode_image_file(f)
        except Exception as e:
            return e

    def run(arrs, names=()):
        latents = X.invert_decoded_images(arrs, args)
        if store is not None:
            store.add(names, latents)
        if trace_batch is not None:
            return trace_batch(latents)
        tile = args.tile if getattr(args, "tamper_map", None) else None
        if getattr(args, "align", "none") != "none":
            from . import align as AL
            cands = AL.alignments(args.align, int(args.align_shift), latents.shape[-2], latents.shape[-1])
            wlevels = getattr(args, "align_window_reliability", None)
            if wlevels is not None and args.per_record_keys:
                return trace_latents_keyed_aligned_soft_l(latents, registry, cands, args.l, levels=wlevels, k=args.top, fpr=args.fpr, tamper_tile=tile)
            if wlevels is not None:
                return trace_latents_aligned_soft_l(latents, args.key, args.nonce, registry, cands, args.l, levels=wlevels, message_length=args.message_length,
                                                    k=args.top, fpr=args.fpr, tamper_tile=tile)
            levels = getattr(args, "align_reliability", None)
            if levels is not None and args.per_record_keys:
                return trace_latents_keyed_aligned_soft(latents, registry, cands, levels=levels, k=args.top, fpr=args.fpr, tamper_tile=tile)
            if levels is not None:
                return trace_latents_aligned_soft(latents, args.key, args.nonce, registry, cands, levels=levels, message_length=args.message_length,
                                                  k=args.top, fpr=args.fpr, tamper_tile=tile)
            if args.per_record_keys:
                return trace_latents_keyed_aligned(latents, registry, cands, k=args.top, fpr=args.fpr, l=args.l, tamper_tile=tile)
            return trace_latents_aligned(latents, args.key, args.nonce, registry, cands, message_length=args.message_length, k=args.top, fpr=args.fpr,
                                         soft=not args.hard, l=args.l, tamper_tile=tile)
        if args.per_record_keys and getattr(args, "window_reliability", None) is not None:
            return trace_latents_keyed_soft_l(latents, registry, args.l, levels=args.window_reliability, k=args.top, fpr=args.fpr)
        if args.per_record_keys and getattr(args, "keyed_reliability", None) is not None:
            return trace_latents_keyed_soft(latents, registry, levels=args.keyed_reliability, k=args.top, fpr=args.fpr, tamper_tile=tile)
        if args.per_record_keys:
            return trace_latents_keyed(latents, registry, k=args.top, fpr=args.fpr, l=args.l, tamper_tile=tile)
        return trace_latents(latents, args.key, args.nonce, registry, message_length=args.message_length, k=args.top, fpr=args.fpr, soft=not args.hard,
                             l=args.l, tamper_tile=tile, reliability=args.reliability)

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        decoded = list(pool.map(decode, files))
    out = list(decoded)
    ready = [i for i, r in enumerate(decoded) if not isinstance(r, Exception)]
    for k0 in range(0, len(ready), int(args.batch_size)):
        idx = ready[k0:k0 + int(args.batch_size)]
        try:
            results = run([decoded[i] for i in idx], [files[i] for i in idx])
        except Exception:
            results = []
            for i in idx:
                try:
                    results += run([decoded[i]], [files[i]])
                except Exception as e:
                    results.append(e)
                    if store is not None:
                        store.drop(files[i])
        for i, r in zip(idx, results):
            out[i] = r
    if getattr(args, "tamper_map", None):
        from . import tamper as TM
        for f, r in zip(files, out):
            if isinstance(r, TraceResult) and r.tamper is not None:
                TM.save_map(r.tamper, TM.map_stem(args.tamper_map, f), (args.width, args.height))
    return out


def _alignment_count(args) -> int:
    """the candidates of --align / --align_shift: 2 R < the lattice's side (an 8 x 8 pixel element), so it is the group times (2 R + 1)^2"""
    from . import align as AL
    return len(AL.GROUPS[args.align]) * (2 * int(args.align_shift) + 1) ** 2


def _statistic_name(args) -> str:
    """the `statistic` field of trace.txt's header"""
    levels = args.reliability if args.reliability is not None else getattr(args, "keyed_reliability", None)
    if levels is None and getattr(args, "align_reliability", None) is not None:
        return f"soft, {args.align_reliability} reliability levels over {_alignment_count(args)} alignments"
    if levels is None and getattr(args, "align_window_reliability", None) is not None:
        return f"soft, {args.align_window_reliability} reliability levels per window bit over {_alignment_count(args)} alignments"
    if levels is None and getattr(args, "window_reliability", None) is not None:
        return f"soft, {args.window_reliability} reliability levels per window bit"
    return "hard" if args.hard else "soft" if levels is None else f"soft, {levels} reliability levels"


def _report(job, outcomes, args, registry, synthetic: bool, set_lines: Sequence[str] = ()) -> None:
    from . import extract as X
    from datetime import datetime
    M = args.message_length
    with open(os.path.join(job.path, "trace.txt"), "a") as out:
        bar = "=" * 40
        keyed = [("keys", registry.n_keys)] if args.per_record_keys else []
        fields = [("Time", datetime.now().strftime("%Y-%m-%d %H:%M:%S")), ("key_hex", "per record" if keyed else args.key_hex),
                  ("nonce_hex", "per record" if keyed else args.nonce_hex), ("registry", args.registry),
                  ("users", len(registry)), *keyed, ("message_length", M), ("statistic", _statistic_name(args)), ("fpr", args.fpr),
                  ("num_inference_steps", args.num_inference_steps), ("scheduler", args.scheduler)]
        if getattr(args, "align", "none") != "none":
            fields += [("align", args.align), ("align_shift", args.align_shift), ("alignments", _alignment_count(args))]
        if getattr(args, "pool", None) is not None:
            fields += [("pool", args.pool)] + ([("pool_reliability", args.pool_reliability)] if args.pool_reliability is not None else [])
        out.write(f"{bar}Batch Info{bar}\n" + "".join(f"{k},{v}\n" for k, v in fields) + f"{bar}Batch Start{bar}\n")
        if synthetic:
            out.write(f"{X.SYNTHETIC_MARKER},'{args.model_id}' is not a local checkpoint: the attributions below are not meaningful\n")
        for f, r in zip(job.files, outcomes):
            line = format_line(f if isinstance(r, Exception) else os.path.basename(f), r, M)
            print(line)
            out.write(line + "\n")
        for line in set_lines:                           # --pool: one line per set, after the per-image lines
            print(line)
            out.write(line + "\n")
        out.write(bar + "Batch End" + bar + "\n")


def main(argv=None):
    args = build_parser().parse_args(list(sys.argv[1:] if argv is None else argv))
    from . import extract as X
    if args.per_record_keys:
        registry = KeyedRegistry.from_file(args.registry)
        if args.message_length not in (None, registry.message_bits):
            raise ValueError(f"--message_length {args.message_length}: with --per_record_keys the length is the registry's own ({registry.message_bits})")
        args.message_length = registry.message_bits
        registry.packed()
    else:
        args.key = bytes.fromhex(args.key_hex)
        args.nonce = bytes.fromhex(args.nonce_hex) if args.nonce_hex != "" else bytes.fromhex(args.key_hex[16:48])
        registry = Registry.from_file(args.registry, args.key, args.nonce)
        if args.message_length is None:
            args.message_length = registry.message_bits
        registry.packed(args.message_length)             # a message_length the registry cannot be tiled to fails here, before any model loads
    synthetic = X._no_checkpoint(args.model_id)
    with X._strictness(args, synthetic):
        if args.images_directory_path != "":
            script = X._plan(args)
            jobs = [j for kind, j in script if kind == "job"]
            if any(j.files for j in jobs):
                X.load_models(args.model_id, allow_synthetic=X._synthetic_allowed(args))      # fail before touching any result file
            pool = _PoolStore(args, registry) if args.pool is not None else None
            with_files = [x for kind, x in script if kind == "job" and x.files]
            for kind, x in script:
                if kind == "banner":
                    print("=" * 20 + x + "=" * 20)
                elif x.files:
                    outcomes = _trace_files(x.files, args, registry, store=pool)
                    named = []
                    if args.pool == "subdirs":
                        named = [(os.path.basename(os.path.normpath(x.path)), x.files)]
                    elif args.pool == "all" and x is with_files[-1]:     # every traced image of the run: the line follows the last directory's images
                        named = [("all", [f for j in with_files for f in j.files])]
                    lines = [format_set_line(name, r) for name, r in pool.trace(named)] if named else []
                    _report(x, outcomes, args, registry, synthetic, lines)
        elif args.single_image_path != "":
            if synthetic:
                X.load_models(args.model_id, allow_synthetic=X._synthetic_allowed(args))
                print(f"{X.SYNTHETIC_MARKER}: '{args.model_id}' is not a local checkpoint, the attribution below is not meaningful", file=sys.stderr)
            pool = _PoolStore(args, registry) if args.pool is not None else None
            r = _trace_files([args.single_image_path], args, registry, store=pool)[0]
            print(format_line(args.single_image_path if isinstance(r, Exception) else os.path.basename(args.single_image_path), r, args.message_length))
            if pool is not None:                         # a set of one: the image's own pooled bound
                for name, s in pool.trace([("all", [args.single_image_path])]):
                    print(format_set_line(name, s))
        else:
            print("Please set the argument 'images_directory_path' or 'single_image_path'")


if __name__ == "__main__":
    main()
