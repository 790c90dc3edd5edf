"""Blind detection: is this image watermarked under one of my keys, and what does it say -- without a registry of messages.

`trace` matches an image against messages that were registered when they were issued; `extract` needs the message to say anything about
its result.  A deployment that rotates keys (per day, per customer, per model) has a list of keys, not a registry: the messages are
timestamps, request ids and hashes nobody stored.  This module holds that list (`Keyring`), the search (`detect_latents`: one
`codec.quant_pack` launch, one `codec.key_search_topk` launch over the keyring, one `codec.extract_records` launch that votes every image
under its own best key) and the exact null distribution of the statistic (`log10_p_blind`), plus a front end
(`python -m gswm_amd.detect`) on `trace`'s image -> latent -> inversion path.

The statistic.  An image has n_bits quantised bits h, a keyring row u is a (key, nonce) pair, M = 8 msg_bytes, V = n_bits / M copies:
    d      = h ^ keystream(u)
    c_t    = #{ j < n_bits : j mod M == t, d_j = 1 }
    S[b,u] = sum_t |2 c_t - V|
S is the score `codec.trace_keyed_topk` would give the image's own majority-voted message under that key (a tie adds 0 either way): the
maximum of the registry score over all 2^M messages.

Null model (the paper's, as in `trace`): an image that is independent of the key decrypts to fair coins.  Then the c_t are independent
Bin(V, 1/2) and S is the sum of M independent copies of |2 Bin(V, 1/2) - V|: an exact law with no free parameter (`log10_p_blind`).
Over a keyring of K keys the reported value is the Bonferroni bound `trace.log10_p_any`; a key is named iff that is <= log10(fpr).

Reliability levels (`detect_latents(..., reliability=L)`, `--reliability L`; l = 1): element j votes with its level w_j in 0..L (`codec.level_pack`),
X_t = sum_{j mod M == t} w_j (2 d_j - 1) and S = sum_t |X_t| (`codec.key_search_soft_topk`).  Given the levels the X_t of a key-independent image are
independent weighted Rademacher sums: `log10_p_blind_soft` computes their exact pmfs and bounds the tail of S by Chernoff -- an upper bound, not the tail.

Both at once (`detect_latents_aligned_soft`, `--align ... --align_reliability L`; l = 1): the level-weighted statistic over every (key, alignment) pair
(`align.search_keys_soft`), the Chernoff bound given the image's levels under THAT alignment, Bonferroni over K A.  `detect_latents(reliability=, align=)` still
refuses the combination; the new names leave every existing path as it was.

Reliability levels at l = 2 and 4 (`detect_latents_soft_l`, `--window_reliability L --l 2|4`): every cipher BIT of an element votes with a level, its element's
distance from the nearest quantiser boundary that would flip it (`codec.level_pack_l`); the search kernel and the Chernoff bound are the ones above over the n l
bits.  Not with `--align`.
"""
from __future__ import annotations

import math
import os
import sys
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple, Union

import numpy as np

from . import codec
from . import soft as S
from . import trace as T

EXACT_MAX_BITS = 65536          # lattices up to here get the exact null tail, larger ones the Chernoff bound
_LN10 = math.log(10.0)
_TILTS = 128                    # exponential tilts per (M, V), spaced evenly in the mean they move the statistic to


# ===================================================================================================================== statistics
def _log_pmf_term(V: int) -> Tuple[np.ndarray, np.ndarray]:
    """One message position under the null: the values a of |2 Bin(V, 1/2) - V| (V, V - 2, ... down to V mod 2, ascending) and
    log P[a] = log C(V, (V + a) / 2) + [a > 0] log 2 - V log 2."""
    a = np.arange(V % 2, V + 1, 2, dtype=np.int64)
    lp = np.array([math.log(math.comb(V, (V + int(x)) // 2)) + (math.log(2.0) if x > 0 else 0.0) for x in a]) - V * math.log(2.0)
    return a, lp


def _tilted(a: np.ndarray, lp: np.ndarray, theta: float) -> Tuple[np.ndarray, float, float]:
    """The term's pmf tilted by e^(theta a): (q, log Z, mean of q), log-sum-exp throughout"""
    w = lp + theta * a
    top = float(w.max())
    e = np.exp(w - top)
    z = float(e.sum())
    q = e / z
    return q, top + math.log(z), float((q * a).sum())


def _theta_for_mean(a: np.ndarray, lp: np.ndarray, mean: float) -> float:
    """theta >= 0 at which the tilted term has this mean (between the null mean and V, exclusive): bisection, the mean grows with theta"""
    lo, hi = 0.0, 1.0
    while _tilted(a, lp, hi)[2] < mean:
        lo, hi = hi, 2.0 * hi
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if _tilted(a, lp, mid)[2] < mean:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


class _NullLaw:
    """The null law of S for one (M, V), as a family of exponentially tilted M-fold convolutions computed on demand.

    Tilt i moves the mean of a term to mu_i = mu_0 + (V - mu_0) i / _TILTS (mu_0 the null mean, theta_0 = 0).  Its pmf q_i = p e^(theta a) / Z
    is convolved M times in float64 -- positive terms only, no cancellation -- and
        P[S >= s] = Z^M e^(-theta s) sum_{x >= s} Q_i(x) e^(-theta (x - s))
    holds for every tilt; a query uses the tilt whose mean is the largest one <= s, so the terms that matter sit in the upper tail of Q_i within
    one grid step of its mean and never underflow (at the top tilt the event "no term below V", probability >= e^(-M V / 256))."""

    def __init__(self, M: int, V: int):
        self.M, self.V = M, V
        self.a, self.lp = _log_pmf_term(V)
        self.x_min = M * (V % 2)                                     # the support of S is x_min, x_min + 2, .., M V
        self.mu0 = float((np.exp(self.lp) * self.a).sum())
        self._tilt: Dict[int, Tuple[float, float, np.ndarray]] = {}

    def _get(self, i: int) -> Tuple[float, float, np.ndarray]:
        t = self._tilt.get(i)
        if t is None:
            theta = 0.0 if i == 0 else _theta_for_mean(self.a, self.lp, self.mu0 + (self.V - self.mu0) * i / _TILTS)
            q, log_z, _ = _tilted(self.a, self.lp, theta)
            Q = np.ones(1)
            for _ in range(self.M):                                 # index j of Q <-> the value x_min-so-far + 2 j
                Q = np.convolve(Q, q)
            # R[j] = sum_{j' >= j} Q[j'] e^(-2 theta (j' - j)), from the top down: positive terms
            R = np.empty_like(Q)
            decay, run = math.exp(-2.0 * theta), 0.0
            for j in range(Q.size - 1, -1, -1):
                run = Q[j] + decay * run
                R[j] = run
            t = self._tilt[i] = (theta, self.M * log_z, R)
        return t

    def log10_tail(self, s: int) -> float:
        if s <= self.x_min:
            return 0.0
        j = (s - self.x_min + 1) // 2                               # the smallest support point >= s
        x = self.x_min + 2 * j
        span = self.V - self.mu0
        i = 0 if span <= 0 else min(_TILTS - 1, max(0, int((x / self.M - self.mu0) / span * _TILTS)))
        theta, m_log_z, R = self._get(i)
        return min(0.0, (m_log_z - theta * x + math.log(R[j])) / _LN10)


_LAWS: Dict[Tuple[int, int], _NullLaw] = {}


def _chernoff_log10(s: int, M: int, V: int) -> float:
    """log10 of inf_{theta >= 0} E[e^(theta S)] e^(-theta s), S the sum of M terms |2 Bin(V, 1/2) - V|"""
    a, lp = _log_pmf_term(V)
    mu0 = float((np.exp(lp) * a).sum())
    if s <= M * mu0:
        return 0.0
    if s >= M * V:
        return M * float(lp[-1]) / _LN10                             # theta -> infinity: P[every term = V], the exact value at the top
    theta = _theta_for_mean(a, lp, s / M)
    return min(0.0, (M * _tilted(a, lp, theta)[1] - theta * s) / _LN10)


def log10_p_blind(stat: int, M: int, V: int) -> float:
    """log10 P[S >= stat] for S = sum of M independent |2 Bin(V, 1/2) - V|: the blind statistic of an image that is independent of the
    key, M message bits with V copies each.  Finite for every stat in 0 .. M V (0.0 at and below the smallest value S can take).

    M V <= 65536: the EXACT tail to float64 rounding, by M-fold convolution of positive terms.  It does not underflow for strong detections
    because the pmf is exponentially tilted before the convolution (a grid of 128 tilts per (M, V), computed on first use and cached; the
    tilt is undone in logarithms).
    M V > 65536: the CHERNOFF BOUND inf_theta E[e^(theta S)] e^(-theta stat) from the folded binomial's moment generating function -- an
    upper bound of the tail, not the tail (at stat = M V it is the exact value)."""
    stat, M, V = int(stat), int(M), int(V)
    if M < 1 or V < 1:
        raise ValueError("M and V must be positive")
    if not 0 <= stat <= M * V:
        raise ValueError(f"stat {stat} is outside 0..{M * V}")
    if M * V > EXACT_MAX_BITS:
        return _chernoff_log10(stat, M, V)
    law = _LAWS.get((M, V))
    if law is None:
        law = _LAWS[(M, V)] = _NullLaw(M, V)
    return law.log10_tail(stat)


class _SoftNullLaw:
    """The null law of the level-weighted statistic of ONE image, given its levels: the exact pmf of every |X_t| and the Chernoff bound of their sum.

    levels [n] ints in 0..15, element j votes on message position j mod M.  Under a key the image is independent of, the decrypted bits are fair coins
    independent of the levels, so X_t = sum_j w_j e_j (e_j = +-1) over the V copies of position t, independently over t.  With Y_t = sum_j w_j d_j
    (d_j in {0, 1}) X_t = 2 Y_t - W_t, and the pmf of Y_t is the dynamic programme p <- (p + p shifted by w_j) / 2 over the copies, run for all M positions at
    once on an [M, max W_t + 1] array: V steps.  Up to V = 1000 in probabilities (the smallest, 2^-V, is a normal float64 and every sum is of positive terms),
    beyond that the same recursion in logarithms."""

    LINEAR_MAX_COPIES = 1000

    def __init__(self, levels, M: int):
        lv = np.asarray(levels)
        M = int(M)
        if lv.ndim != 1 or lv.size < 1 or lv.dtype.kind not in "iu":
            raise ValueError("levels must be a one-dimensional integer array")
        if M < 1 or lv.size % M:
            raise ValueError(f"{lv.size} levels are not whole copies of {M} message positions")
        lv = lv.astype(np.int64)
        if lv.min() < 0 or lv.max() > codec.SOFT_MAX_LEVELS:
            raise ValueError(f"levels must be in 0..{codec.SOFT_MAX_LEVELS}")
        w = lv.reshape(-1, M)                                        # [V, M]
        self.M, self.V = M, w.shape[0]
        self.W = w.sum(axis=0)                                       # [M]
        self.total = int(self.W.sum())
        size = int(self.W.max()) + 1
        y = np.arange(size, dtype=np.int64)
        linear = self.V <= self.LINEAR_MAX_COPIES
        p = np.zeros((M, size)) if linear else np.full((M, size), -np.inf)
        p[:, 0] = 1.0 if linear else 0.0
        for i in range(self.V):
            src = y[None, :] - w[i][:, None]
            moved = np.take_along_axis(p, np.maximum(src, 0), axis=1)
            if linear:
                p = 0.5 * (p + np.where(src >= 0, moved, 0.0))
            else:
                p = np.logaddexp(p, np.where(src >= 0, moved, -np.inf)) - math.log(2.0)
        with np.errstate(divide="ignore"):
            self.lp = np.log(p) if linear else p                     # [M, size] log P[Y_t = y]; -inf past W_t and where no pattern lands
        self.a = np.abs(2 * y[None, :] - self.W[:, None]).astype(np.float64)     # |X_t| at Y_t = y
        rows = np.arange(M)
        top = np.logaddexp(self.lp[rows, 0], self.lp[rows, self.W])   # P[|X_t| = W_t] = P[Y = 0] + P[Y = W_t]
        self.log_top = float(np.where(self.W > 0, top, 0.0).sum())   # (W_t = 0: the position is 0 with certainty)
        self.mean0 = self._tilted(0.0)[1]

    def _tilted(self, theta: float) -> Tuple[float, float]:
        """(sum_t log E e^(theta |X_t|), sum_t the mean of |X_t| under that tilt), log-sum-exp"""
        x = self.lp + theta * self.a
        top = x.max(axis=1)
        e = np.exp(x - top[:, None])
        z = e.sum(axis=1)
        return float((top + np.log(z)).sum()), float(((e * self.a).sum(axis=1) / z).sum())

    def log10_bound(self, s: int) -> float:
        s = int(s)
        if not 0 <= s <= self.total:
            raise ValueError(f"stat {s} is outside 0..{self.total}")
        if s <= self.mean0:
            return 0.0
        if s >= self.total:
            return self.log_top / _LN10                              # theta -> infinity: every position at its extreme, the exact value at the top
        lo, hi = 0.0, 1.0                                            # the tilted mean grows with theta from E[S] to sum W: bisection
        while self._tilted(hi)[1] < s:
            lo, hi = hi, 2.0 * hi
        for _ in range(100):
            mid = 0.5 * (lo + hi)
            if mid <= lo or mid >= hi:
                break
            if self._tilted(mid)[1] < s:
                lo = mid
            else:
                hi = mid
        theta = 0.5 * (lo + hi)
        return min(0.0, (self._tilted(theta)[0] - theta * s) / _LN10)


def log10_p_blind_soft(stat: int, levels, M: int) -> float:
    """An UPPER BOUND of log10 P[S >= stat] for the level-weighted blind statistic S = sum_t |X_t| (`codec.key_search_soft_topk`) of an image that is
    independent of the key, given the image's levels: `levels` int [n] in 0..15, element j on message position j mod M.

    Conditionally on the levels the X_t are independent weighted Rademacher sums; their pmfs are exact (integer dynamic programming, `_SoftNullLaw`), the
    tail of their sum is bounded by Chernoff: min_theta [sum_t log E e^(theta |X_t|) - theta stat] / ln 10, in log-sum-exp.  0.0 at and below E[S]; at
    stat = sum_t W_t the exact value prod_t P[|X_t| = W_t]; finite everywhere; ValueError outside 0 .. sum_t W_t.  It is a bound, NOT the tail: for unit
    levels, where the exact tail is known (`log10_p_blind`), the same bound is 1.1 to 1.5 decades weaker than it at 4096-element lattices with 64-bit
    messages.  The exact tail (a tilted convolution of M non-identical terms) is not computed."""
    return _SoftNullLaw(levels, M).log10_bound(stat)


# ===================================================================================================================== keyring
def _check_key_id(key_id) -> None:
    if not isinstance(key_id, str) or not key_id or any(ch in key_id for ch in "\t\r\n"):
        raise ValueError(f"key id {key_id!r} must be a non-empty string without tabs or line breaks")


class Keyring:
    """Ordered key_id -> (key, nonce) rows with unique ids: the keys a deployment has issued watermarks under"""

    def __init__(self):
        self._ids: List[str] = []
        self._rows: List[Tuple[bytes, bytes]] = []
        self._by_id: Dict[str, int] = {}
        self._device_cache = {}

    def __len__(self) -> int:
        return len(self._ids)

    @property
    def key_ids(self) -> List[str]:
        return list(self._ids)

    def key_at(self, index: int) -> str:
        return self._ids[index]

    def row_at(self, index: int) -> Tuple[bytes, bytes]:
        return self._rows[index]

    def add(self, key_id: str, key: Union[str, bytes], nonce: Union[str, bytes]) -> int:
        """Add (key, nonce) as `key_id`; returns the row index.  key (32 bytes) and nonce (16 bytes) are bytes or hex strings."""
        _check_key_id(key_id)
        try:
            key, nonce = T._as_bytes(key, "key"), T._as_bytes(nonce, "nonce")
        except ValueError:
            raise ValueError(f"key {key_id!r}: key and nonce must be hexadecimal") from None
        if key is None or len(key) != 32:
            raise ValueError(f"key {key_id!r}: the ChaCha20 key must be 32 bytes")
        if nonce is None or len(nonce) != 16:
            raise ValueError(f"key {key_id!r}: the ChaCha20 nonce must be 16 bytes")
        if key_id in self._by_id:
            raise ValueError(f"key id {key_id!r} is already in the keyring")
        self._by_id[key_id] = len(self._ids)
        self._ids.append(key_id)
        self._rows.append((key, nonce))
        self._device_cache.clear()
        return len(self._ids) - 1

    # -- files
    def save(self, path) -> None:
        """one `key_id<TAB>key_hex<TAB>nonce_hex` per line"""
        with open(path, "w") as f:
            for kid, (key, nonce) in zip(self._ids, self._rows):
                f.write(f"{kid}\t{key.hex()}\t{nonce.hex()}\n")

    @classmethod
    def load(cls, path) -> "Keyring":
        ring = cls()
        with open(path) as f:
            for no, line in enumerate(f, 1):
                line = line.rstrip("\r\n")
                if not line:
                    continue
                cols = line.split("\t")
                if len(cols) != 3:
                    raise ValueError(f"{path}:{no}: expected 'key_id<TAB>key_hex<TAB>nonce_hex'")
                try:
                    key, nonce = (bytes.fromhex(c.strip()) for c in cols[1:])
                except ValueError:
                    raise ValueError(f"{path}:{no}: key {cols[0]!r} is not hexadecimal") from None
                try:
                    ring.add(cols[0], key, nonce)
                except ValueError as e:
                    raise ValueError(f"{path}:{no}: {e}") from None
        if not len(ring):
            raise ValueError(f"{path}: no keyring entries")
        return ring

    @classmethod
    def from_info_data(cls, path) -> "Keyring":
        """The distinct (key, nonce) pairs of the log gs_insert appends per issued watermark, in order of first use; ids
        `info:<record number>` of the first record under that pair (numbered as `trace.Registry.from_info_data` numbers them)."""
        ring, seen = cls(), set()
        for number, key, nonce, _ in T._info_data_records(path):
            if key is None or nonce is None:
                raise ValueError(f"{path}: record {number} has no key / nonce")
            pair = (bytes.fromhex(key), bytes.fromhex(nonce))
            if pair not in seen:
                seen.add(pair)
                ring.add(f"info:{number}", *pair)
        if not len(ring):
            raise ValueError(f"{path}: no records")
        return ring

    @classmethod
    def from_keyed_registry(cls, kreg: "T.KeyedRegistry") -> "Keyring":
        """The distinct (key, nonce) pairs of a keyed registry, in order; a pair takes the id of its first record"""
        ring, seen = cls(), set()
        for i in range(len(kreg)):
            key, nonce, _ = kreg.record_at(i)
            if (key, nonce) not in seen:
                seen.add((key, nonce))
                ring.add(kreg.user_at(i), key, nonce)
        if not len(ring):
            raise ValueError("the registry is empty")
        return ring

    # -- device
    def packed(self) -> np.ndarray:
        """uint8 [K, 48]: a row is key[32] | nonce[16] (the key rows of `codec.key_search_topk`)"""
        if not self._ids:
            raise ValueError("the keyring is empty")
        t = self._device_cache.get("host")
        if t is None:
            flat = np.frombuffer(b"".join(k + n for k, n in self._rows), dtype=np.uint8)
            t = self._device_cache["host"] = flat.reshape(len(self._ids), codec.KEYED_RECORD_HEAD).copy()
        return t

    def to_device(self, device="cuda"):
        import torch
        k = str(torch.device(device))
        t = self._device_cache.get(k)
        if t is None:
            t = self._device_cache[k] = torch.from_numpy(self.packed()).to(device)
        return t


# ===================================================================================================================== detection
@dataclass
class KeyCandidate:
    key_id: str
    index: int
    stat: int
    log10_p_any: float          # Bonferroni bound over the keyring (with `align`: over the keyring x the candidate alignments)
    alignment: Optional[Tuple[int, int, int]] = None     # with `align`: this key's best alignment (d, dy, dx) of the image (`align.apply` undoes the attack)


@dataclass
class DetectResult:
    candidates: List[KeyCandidate] = field(default_factory=list)
    key_id: Optional[str] = None        # the best candidate's key id if its bound is <= log10(fpr), else None: none of these keys
    message: Optional[bytes] = None     # the majority-voted message under that key (None when no key is named)
    flags: int = 0                      # GSW_FLAG_* of the image (a saturated or NaN latent: the reference refuses such an image)
    alignment: Optional[Tuple[int, int, int]] = None     # with `align`: the named key's alignment, the one the message was read under (None when no key is named)


def _message_bytes(message_length) -> int:
    m = int(message_length)
    if m < 8 or m % 8 or m > 8 * 256:
        raise ValueError(f"message_length {message_length!r} must be a multiple of 8 in 8..2048 bits")
    return m // 8


def detect_latents(latents, keyring: Keyring, message_length: int, *, k: int = 1, fpr: float = 1e-6, l: int = 1, align=None,
                   reliability: int = 0) -> List[DetectResult]:
    """latents [B, ...] on the device -> one DetectResult per image: the k best keys of the keyring (best first) with their Bonferroni
    bounds, the key that is named at false-positive rate `fpr` per image over the whole keyring (or None) and the message voted under it.

    Three launches: `codec.quant_pack` (the image is quantised once, whatever the number of keys), `codec.key_search_topk` (every key's
    keystream is generated inside it) and `codec.extract_records`, which votes every image under its own best key (its rows are that key
    and nonce with a zero message; `matches` is ignored).  The host receives the B k (index, stat) pairs, the flags and the voted bytes.
    l: cipher bits per lattice element the images were embedded with; the rows then hold n l bits.  Raises IndexError where
    `extract_batch` does (n l is not a multiple of message_length).

    align: a list of candidate alignments (`align.alignments`) for images that may have been mirrored, turned by a quarter or shifted on the
    lattice; latents must then be [B, C, H, W].  The candidates come from `align.search_keys` (one more launch, `codec.rows_align`, in front of
    the search), the Bonferroni factor is K A, every candidate carries its best alignment, and each image is read after `align.apply` of
    its best candidate's alignment.  None: exactly the path above.

    reliability: 0, or the number of reliability levels (1..15) every lattice element votes with: `soft.uniform_thresholds`, one `codec.level_pack`, one
    `codec.key_search_soft_topk` in place of the sign search, and the message of the best key read by one `codec.extract_soft` launch with the same
    thresholds.  `KeyCandidate.stat` is then the level-weighted statistic and the bound under it `log10_p_blind_soft` -- a Chernoff bound given the image's
    levels, which the host reads from the planes already on the device.  One cipher bit per element only (l = 1), and not with `align` yet (ValueError)."""
    reliability = _reliability_levels(reliability)
    if reliability and align is not None:
        raise ValueError("reliability cannot be combined with align yet: the level planes are not carried through the alignment search")
    limit, mb = _rate_and_bytes(fpr, message_length)
    l = codec.check_window(l)
    if reliability and l != 1:
        raise ValueError(f"reliability cannot be combined with l = {l}: reliability levels are defined for one cipher bit per element")
    return _detect(latents, keyring, mb, k, limit, l=l, levels=reliability, aligns=align)[0]


def _reliability_levels(reliability) -> int:
    if isinstance(reliability, bool) or not isinstance(reliability, (int, np.integer)) or not 0 <= int(reliability) <= codec.SOFT_MAX_LEVELS:
        raise ValueError(f"reliability must be 0 (the sign statistic) or a number of levels in 1..{codec.SOFT_MAX_LEVELS}, got {reliability!r}")
    return int(reliability)


def levels_from_planes(planes: np.ndarray) -> np.ndarray:
    """`codec.level_pack`'s planes on the host, uint8 [B, P, n / 8] -> the levels int64 [B, n]"""
    bits = np.unpackbits(planes, axis=2).astype(np.int64)
    return sum(bits[:, p] << p for p in range(planes.shape[1]))


def _rate_and_bytes(fpr, message_length) -> Tuple[float, int]:
    """What every detection checks first, in this order -> (log10 fpr, message bytes)"""
    return T._log10_fpr(fpr), _message_bytes(message_length)


# The four steps of a detection, each in the forms a decoder chooses from.  pack(z, l, levels) -> (packed operand, flags, threshold table or None);
# search(packed, shape, l, keys_dev, mb, table, k) -> (idx, stat, alignment index or None), int32 [B, k] on the device; read(z, rows, mb, l, thr) -> voted bytes;
# law(packed, M, V, shape, table) -> bound(b, a, s), log10 of the null tail of statistic s of image b under alignment index a (None: as it stands).
def _pack_signs(z, l, levels):
    packed, flags = codec.quant_pack(z, l)
    return packed, flags, None


def _pack_levels(z, l, levels):
    thr = S._default_table(z, l, levels)                           # once, on the un-aligned latents: the search, the bound and the vote share it
    packed = codec.level_pack(z, thr) if l == 1 else codec.level_pack_l(z, thr, l)
    return packed, packed.flags, thr


def _search_signs(packed, shape, l, keys_dev, mb, table, k):
    return codec.key_search_topk(packed, packed.shape[1] * 8, keys_dev, mb, k=k) + (None,)


def _search_levels(packed, shape, l, keys_dev, mb, table, k):
    return codec.key_search_soft_topk(packed, packed.signs.shape[1] * 8, keys_dev, mb, k=k) + (None,)


def _search_signs_aligned(packed, shape, l, keys_dev, mb, table, k):
    from . import align as AL
    idx, aidx, stat = AL._search_packed(packed, shape, l, keys_dev, mb, table, k)
    return idx, stat, aidx


def _search_levels_aligned(packed, shape, l, keys_dev, mb, table, k):
    from . import align as AL
    codec._level_rows_align_checks(packed, shape, l)
    idx, aidx, stat = AL._search_level_rows(packed, shape, keys_dev, mb, table, k, l=l)
    return idx, stat, aidx


def _read_signs(z, rows, mb, l, thr):
    return codec.extract_records(z, rows, mb, l=l)[0]


def _read_levels(z, rows, mb, l, thr):
    return (codec.extract_soft(z, rows, mb, thr) if l == 1 else codec.extract_soft_l(z, rows, mb, thr, l)).bits


def _read_scored(z, rows, mb, l, thr):
    """the read of `_read_signs` (thr None) or `_read_levels`, with the votes it was taken from -> (bits, score int32 [B, 8 mb]): what `detect_payloads` decodes"""
    if thr is None:
        bits, _, _, counts = codec.extract_records(z, rows, mb, l=l, return_counts=True)
        return bits, 2 * counts - codec.vote_copies(z.numel() // z.shape[0], 8 * mb, l)
    vote = codec.extract_soft(z, rows, mb, thr) if l == 1 else codec.extract_soft_l(z, rows, mb, thr, l)
    return vote.bits, vote.score


def _law_signs(packed, M, V, shape, table):
    return lambda b, a, s: log10_p_blind(s, M, V)                  # exact, and the same under every alignment: a permutation keeps the copies per position


def _law_levels(packed, M, V, shape, table):
    """One dynamic programme per distinct (image, alignment) among the reported candidates: an alignment moves elements between message positions, so the W_t
    and with them the null law differ from one alignment to the next"""
    import torch
    from . import align as AL
    lv = levels_from_planes(packed.planes.cpu().numpy())           # over the n l cipher bits, bit j on message position j mod M
    laws: Dict[Tuple[int, Optional[int]], _SoftNullLaw] = {}

    def aligned(row, a):                                           # the l levels of an element travel with it: [C, H, W, l] -> l lattices -> back
        cube = torch.from_numpy(row.reshape(tuple(shape) + (-1,))).movedim(-1, 0)
        return AL.apply(cube, a).movedim(0, -1).reshape(-1).numpy()

    def bound(b: int, a: Optional[int], s: int) -> float:
        t = laws.get((b, a))
        if t is None:
            row = lv[b] if a is None else aligned(lv[b], table[a])
            t = laws[(b, a)] = _SoftNullLaw(row, M)
        return t.log10_bound(s)

    return bound


_DECODERS = {  # (level-weighted, with alignments) -> (pack, search, read, law); the next decoder is one more row
    (False, False): (_pack_signs, _search_signs, _read_signs, _law_signs),
    (True, False): (_pack_levels, _search_levels, _read_levels, _law_levels),
    (False, True): (_pack_signs, _search_signs_aligned, _read_signs, _law_signs),
    (True, True): (_pack_levels, _search_levels_aligned, _read_levels, _law_levels),
}


def _detect(latents, keyring: Keyring, mb: int, k: int, limit: float, *, l: int, levels: int, aligns, scores: bool = False):
    """The one flow behind `detect_latents`, `detect_latents_soft_l`, `detect_latents_aligned_soft` and `detect_latents_aligned_soft_l`, after the checks that are each entry's own: pack the
    images, search the keyring, read every image under its best key, bound every reported statistic, build the candidate lists
    -> (results, the best candidate's alignment index int [B] or None, the bytes voted under the best key uint8 [B, mb]).

    levels: 0 -- the sign statistic; 1..15 -- the level-weighted statistic.  aligns: None, or the candidate alignments: the search then runs over every
    (key, alignment) pair and the image is read with its best alignment applied.  `_DECODERS` holds the four steps of each combination.
    scores: also return, as a fourth entry, the votes the read was taken from (int32 [B, 8 mb] on the device; `detect_payloads`)."""
    import torch
    from . import align as AL
    pack, search, read, law = _DECODERS[(bool(levels), aligns is not None)]
    M = 8 * mb
    k = int(k)
    if not 1 <= k <= 8:
        raise ValueError("k must be in 1..8")
    keys_host = keyring.packed()                                   # (an empty keyring fails here)
    if aligns is not None and latents.dim() != 4:
        raise ValueError(f"align needs latents [B, C, H, W], got {tuple(latents.shape)}")
    z = latents.contiguous()
    B, shape = z.shape[0], tuple(z.shape[1:])
    table = None if aligns is None else AL._as_list(aligns, shape[1], shape[2])
    V = codec.vote_copies(z.numel() // max(B, 1), M, l)            # (a lattice the message does not tile fails here, as extract_batch would)
    keys_dev = keyring.to_device(z.device) if z.is_cuda else torch.from_numpy(keys_host)
    packed, flags, thr = pack(z, l, levels)
    idx, stat, aidx = search(packed, shape, l, keys_dev, mb, table, k)
    rows = torch.zeros((B, codec.keyed_record_stride(mb)), dtype=torch.uint8, device=z.device)
    rows[:, :codec.KEYED_RECORD_HEAD] = keys_dev[idx[:, 0].long()]      # every image under its own best key, a zero message: `matches` is not read
    score = None
    if aidx is None and scores:
        bits, score = _read_scored(z, rows, mb, l, thr)
        idx_h, stat_h = T._pairs_to_host(idx, stat)
        aidx_h = None
    elif aidx is None:
        bits = read(z, rows, mb, l, thr)
        idx_h, stat_h = T._pairs_to_host(idx, stat)
        aidx_h = None
    else:                                                          # the read needs the best alignment on the host first
        idx_h, aidx_h, stat_h = torch.stack([idx, aidx, stat]).cpu().numpy()
        bits = read(AL.unalign(z, table, aidx_h[:, 0]), rows, mb, l, thr)
    flags_h, bits_h = flags.cpu().numpy(), bits.cpu().numpy()
    pairs = len(keyring) * (1 if table is None else len(table))    # Bonferroni: over the keys, or over the (key, alignment) pairs
    bound = law(packed, M, V, shape, table)

    def candidate(b, j, i, s):
        a = None if aidx_h is None else int(aidx_h[b, j])
        return KeyCandidate(keyring.key_at(i), i, s, T.log10_p_any(bound(b, a, s), pairs), None if a is None else table[a])

    out = T._candidate_lists(idx_h, stat_h, flags_h, limit, candidate,
                             lambda b, c, named: DetectResult(c, c[0].key_id if named else None, bits_h[b].tobytes() if named else None, int(flags_h[b]),
                                                              c[0].alignment if named else None),
                             refuse=False)
    best = None if aidx_h is None else aidx_h[:, 0]
    return (out, best, bits_h, score) if scores else (out, best, bits_h)


def detect_latents_soft_l(latents, keyring: Keyring, message_length: int, l: int, *, levels: int = 15, k: int = 1, fpr: float = 1e-6) -> List[DetectResult]:
    """`detect_latents(reliability=levels)` for multi-bit windows (l = 2 or 4): every one of the n l cipher bits of an
    image votes with a level 0..levels, the distance of its element from the nearest quantiser boundary at which that bit would have come out
    differently.  `soft.window_thresholds`, one `codec.level_pack_l`, the unchanged `codec.key_search_soft_topk` with n_bits = n l, and the
    message of the best key read by one `codec.extract_soft_l` launch with the same thresholds.  `KeyCandidate.stat` is the level-weighted
    statistic; the bound under it is `log10_p_blind_soft` on the n l per-bit levels read back from the planes (given the levels, the decrypted
    bits of a key-independent image are independent fair coins, per cipher bit), Bonferroni over the keyring.  n l (1 + P) may not exceed
    1 048 576, P the bit length of `levels`: the search refuses beyond (ValueError).  l = 1 is refused: that is `detect_latents(reliability=)`."""
    limit, mb = _rate_and_bytes(fpr, message_length)
    l = codec.check_window(l)
    if l == 1:
        raise ValueError("l = 1 has no window bits: the level-weighted key search at l = 1 is detect_latents(reliability=) (--reliability)")
    levels = _reliability_levels(levels)
    if not levels:
        raise ValueError(f"levels must be a number of levels in 1..{codec.SOFT_MAX_LEVELS}, got 0")
    return _detect(latents, keyring, mb, k, limit, l=l, levels=levels, aligns=None)[0]


def detect_payloads(latents, keyring: Keyring, message_length: int, *, ecc: str = "conv", k: int = 1, fpr: float = 1e-6, l: int = 1, reliability: int = 0,
                    window_reliability: int = 0, list_size: int = 1):
    """Blind detection of images whose messages are error-corrected payloads (`ecc.encode`) -> (results, reads):
    `results` is what `detect_latents` (sign statistic, or `reliability=L` at l = 1) or `detect_latents_soft_l` (`window_reliability=L` at l = 2, 4)
    returns, unchanged -- `DetectResult.message` stays the majority-voted CODED message -- and reads[b] is the `ecc.EccRead` of image b (one entry in each
    of its lists) when a key is named, else None.  The votes of every image under its own best key -- the read's score, or 2 counts - copies of the sign
    read -- go through ONE `codec.viterbi_decode` launch for the whole batch.  Alignments are not wired yet: `ecc` with `align` is the next step.
    list_size = 2, 4 or 8: the list read -- the launch is `codec.viterbi_list_decode`'s and reads[b] an `ecc.EccListRead`;
    list_size = 1 is today's launch and today's `EccRead`.  ecc="conv23" / "conv34": the punctured codes, same reads."""
    from . import ecc as E
    if E.check_code(ecc) is None:
        raise ValueError('detect_payloads needs ecc="conv": without a code this is detect_latents')
    list_size = E.check_list_size(list_size)
    limit, mb = _rate_and_bytes(fpr, message_length)
    E.check_length(8 * mb)
    l = codec.check_window(l)
    reliability, window_reliability = _reliability_levels(reliability), _reliability_levels(window_reliability)
    if reliability and window_reliability:
        raise ValueError("reliability (l = 1) and window_reliability (l = 2, 4) cannot be combined")
    if reliability and l != 1:
        raise ValueError(f"reliability cannot be combined with l = {l}: at l = 2 and 4 the levels are window_reliability")
    if window_reliability and l == 1:
        raise ValueError("window_reliability needs l = 2 or 4: at l = 1 the levels are reliability")
    results, _, _, score = _detect(latents, keyring, mb, k, limit, l=l, levels=reliability or window_reliability, aligns=None, scores=True)
    read = E.read_any(score.contiguous(), list_size, ecc)
    return results, [read.image(b) if r.key_id is not None else None for b, r in enumerate(results)]


class _PayloadOutcome:
    """what the command line carries per image with --ecc: the unchanged DetectResult and the text appended to its line"""

    def __init__(self, result: DetectResult, text: str):
        self.result, self.text = result, text


def _line(name: str, r) -> str:
    return format_line(name, r.result) + r.text if isinstance(r, _PayloadOutcome) else format_line(name, r)


def _aligned_soft(latents, keyring: Keyring, message_length: int, aligns, levels: int, k: int, fpr: float, l: int = 1):
    """`detect_latents_aligned_soft` and, with l = 2 or 4, `detect_latents_aligned_soft_l` -> (results, the best candidate's alignment index int [B], the bytes
    voted under it uint8 [B, msg_bytes])"""
    limit, mb = _rate_and_bytes(fpr, message_length)
    levels = _reliability_levels(levels)
    if not levels:
        raise ValueError(f"levels must be in 1..{codec.SOFT_MAX_LEVELS}: a search without levels is detect_latents(align=...)")
    return _detect(latents, keyring, mb, k, limit, l=l, levels=levels, aligns=aligns)


def detect_latents_aligned_soft(latents, keyring: Keyring, message_length: int, aligns, *, levels: int = 15, k: int = 1,
                                fpr: float = 1e-6) -> List[DetectResult]:
    """`detect_latents(align=...)` ranked by `levels` reliability levels (1..15; l = 1): the alignment search with every lattice element
    weighted by its level.  latents [B, C, H, W] on the device, aligns from `align.alignments`.

    `soft.uniform_thresholds` once on the un-aligned latents, one `codec.level_pack`, `align.search_keys_soft`'s search (per chunk of images one
    `codec.level_rows_align` and one `codec.key_search_soft_topk`), and the message of the best key read by one `codec.extract_soft` launch on the
    latents with their best alignment applied, under the SAME threshold table.  `KeyCandidate.stat` is the level-weighted statistic and
    `alignment` that key's best alignment.  The bound is `log10_p_blind_soft` given the image's levels UNDER THAT ALIGNMENT -- an alignment moves
    elements between message positions, so the W_t and with them the null law differ from one alignment to the next; the host permutes the levels
    it read from the planes and runs one dynamic programme per distinct (image, alignment) among the reported candidates -- then Bonferroni over
    the K A (key, alignment) pairs: under a key the image is independent of, the bits of any fixed permutation are fair coins independent of
    the levels, so the bound holds for every pair and the union bound needs nothing else."""
    return _aligned_soft(latents, keyring, message_length, aligns, levels, k, fpr)[0]


def detect_latents_aligned_soft_l(latents, keyring: Keyring, message_length: int, aligns, l: int, *, levels: int = 15, k: int = 1,
                                  fpr: float = 1e-6) -> List[DetectResult]:
    """`detect_latents_aligned_soft` for multi-bit windows (l = 2 or 4): the alignment search with every one of the n l cipher bits
    weighted by its level of `codec.extract_soft_l`.  latents [B, C, H, W] on the device, aligns from `align.alignments`.

    `soft.window_thresholds` once on the un-aligned latents, one `codec.level_pack_l`, `align.search_keys_soft_l`'s search (per chunk of images one
    `codec.level_rows_align_l` and the unchanged `codec.key_search_soft_topk` with n_bits = n l), and the message of the best key read by one
    `codec.extract_soft_l` launch on the latents with their best alignment applied, under the SAME table.  The bound is `log10_p_blind_soft` given the n l levels
    UNDER THAT ALIGNMENT -- the host permutes the levels it read from the planes in groups of l, as the kernel does -- then Bonferroni over the K A pairs.
    n l (1 + P) may not exceed 1 048 576.  l = 1 is refused: that is `detect_latents_aligned_soft`."""
    l = codec._multi_bit_window(l, "detect_latents_aligned_soft")
    return _aligned_soft(latents, keyring, message_length, aligns, levels, k, fpr, l)[0]


# ===================================================================================================================== front end
def format_line(name: str, result) -> str:
    """One line of detect.txt / stdout"""
    if isinstance(result, Exception):
        return f"Error processing {name}: {result}"
    if not result.candidates:
        return f"{name}, key: none, log10 p, 0.0"
    c = result.candidates[0]
    text = f"{name}, key: {result.key_id if result.key_id is not None else 'none'}, log10 p, {c.log10_p_any:.3f}"
    text += f", message: {result.message.hex() if result.message is not None else 'none'}"
    for o in result.candidates[1:]:
        text += f", next: {o.key_id} ({o.log10_p_any:.3f})"
    if result.flags:
        text += f", flags {result.flags}"
    if c.alignment is not None:                                    # only a search with `align` sets it: the best candidate's, named or not
        from . import align as AL
        text += f", alignment: {AL.describe(c.alignment)}"
    return text


def _fpr(text: str) -> float:
    v = float(text)
    if not 0.0 < v <= 1.0:
        raise ValueError("fpr must be in (0, 1]")
    return v


def build_parser():
    import argparse
    p = argparse.ArgumentParser(prog="python -m gswm_amd.detect",
                                description="Name the key of a keyring an image is watermarked under, and read its message, without a registry "
                                            "of messages (single GPU)")
    p.add_argument("--model_id", default="stabilityai/stable-diffusion-2-1-base")
    p.add_argument("--images_directory_path", default="", help="The path of directory containing images to process")
    p.add_argument("--single_image_path", default="")
    p.add_argument("--keyring", required=True, help="keyring file: 'key_id<TAB>key_hex<TAB>nonce_hex' lines, or the info_data.txt log gs_insert "
                                                     "appends (told apart by the first line; of a log, the distinct key / nonce pairs are used)")
    p.add_argument("--message_length", type=int, default=256, help="Length of the message in bits (a multiple of 8, at most 2048)")
    p.add_argument("--fpr", type=_fpr, default=1e-6, help="false-positive rate per image, over the whole keyring (Bonferroni), in (0, 1]")
    p.add_argument("--top", type=int, default=1, choices=range(1, 9), metavar="K", help="candidate keys reported per image (1..8)")
    p.add_argument("--l", type=int, default=1, choices=codec.WINDOWS, help="cipher bits per lattice element the images were embedded with")
    p.add_argument("--reliability", type=int, default=0, choices=range(0, 16), metavar="L",
                   help="rank the keys by level-weighted margins: every lattice element votes with one of L (1..15) reliability levels taken from its "
                        "magnitude, the p-value is a Chernoff bound given the levels (--l 1, not with --align); 0: the sign statistic")
    p.add_argument("--align", default="none", choices=("none", "flips", "d4"),
                   help="also try every alignment of the lattice in this group: flips (half turn and the two mirrors) or d4 (all eight orientations); "
                        "the Bonferroni factor grows by the number of candidates")
    p.add_argument("--align_shift", type=int, default=0, metavar="R", help="with --align: also every lattice shift in [-R, R]^2 (8 R pixels)")
    p.add_argument("--align_reliability", type=int, default=0, choices=range(0, 16), metavar="L",
                   help="with --align: rank every (key, alignment) pair by level-weighted margins, L (1..15) reliability levels per lattice element; the "
                        "p-value is a Chernoff bound given the levels under the alignment (--l 1, not with --reliability); 0: the sign statistic")
    p.add_argument("--window_reliability", type=int, default=0, choices=range(0, 16), metavar="L",
                   help="with --l 2 or 4: rank the keys by level-weighted margins, every cipher bit of a lattice element votes with one of L (1..15) "
                        "levels taken from its distance to the quantiser boundaries that would flip it; the p-value is a Chernoff bound given the levels "
                        "(not with --align, --reliability or --align_reliability); 0: the sign statistic")
    p.add_argument("--align_window_reliability", type=int, default=0, choices=range(0, 16), metavar="L",
                   help="with --align and --l 2 or 4: rank every (key, alignment) pair by level-weighted margins, every cipher bit of a lattice element votes "
                        "with one of L (1..15) levels taken from its distance to the quantiser boundaries that would flip it; the p-value is a Chernoff bound "
                        "given the levels under the alignment (not with --reliability, --align_reliability or --window_reliability); 0: the sign statistic")
    p.add_argument("--num_inference_steps", default=30, type=int, help="Number of inference steps for the model")
    p.add_argument("--scheduler", default="DDIM", help="Choose a scheduler between 'DPMs' and 'DDIM' to inverse the image")
    p.add_argument("--is_traverse_subdirectories", default=0, help="Whether to traverse subdirectories recursively")
    p.add_argument("--width", type=int, default=1024, help="Width of the input image")
    p.add_argument("--height", type=int, default=1024, help="Height of the input image")
    p.add_argument("--allow_synthetic_weights", action="store_true", help="run without a checkpoint (pipeline tests / benchmarks only)")
    p.add_argument("--batch_size", type=int, default=16, help="images per device batch")
    p.add_argument("--strict_kernels", type=int, choices=[0, 1], default=None,
                   help="1: raise when a GPU half-precision call would leave the hand-written kernels instead of warning (default: 1)")
    p.add_argument("--ecc", default=None, choices=("conv", "conv23", "conv34"),
                   help="the messages are error-corrected payloads (issue --ecc conv): for a named key the votes are decoded by one Viterbi launch per batch and "
                        "the line gains 'payload <hex> crc ok|FAILED, corrected <flips> of <M>' (with the sign statistic, --reliability or "
                        "--window_reliability; not with --align, --align_shift, --align_reliability or --align_window_reliability yet)")
    p.add_argument("--ecc_list", type=int, default=1, choices=(1, 2, 4, 8),
                   help="with --ecc conv: the list read -- the decoder keeps this many best paths and the CRC picks among them; the line gains "
                        "', list rank <r> of <L>[, <n> candidates pass]'.  1 (default): the plain read and today's text.  Nothing issued changes; a false "
                        "'crc ok' on an unmarked image becomes at most L times as likely (L 2^-18 at 256 bits)")
    return p


def ecc_refusal(args) -> Optional[str]:
    """--ecc next to an alignment flag: refused by name (the decode composes with the alignment search; wiring it is not part of this step)"""
    if getattr(args, "ecc", None) is None:
        if int(getattr(args, "ecc_list", 1) or 1) > 1:
            return "--ecc_list above 1 needs --ecc conv: the list read is a read of error-corrected payloads"
        return None
    for flag, on in (("--align", getattr(args, "align", "none") != "none"), ("--align_shift", bool(getattr(args, "align_shift", 0))),
                     ("--align_reliability", bool(getattr(args, "align_reliability", 0))),
                     ("--align_window_reliability", bool(getattr(args, "align_window_reliability", 0)))):
        if on:
            return f"--ecc cannot be combined with {flag} yet: the payload read is not wired through the alignment search"
    return None


def load_keyring(path) -> Keyring:
    """gs_insert's log or the three-column format, told apart by the first line"""
    return Keyring.from_info_data(path) if T.detect_format(path) == "info_data" else Keyring.load(path)


def _detect_files(files, args, keyring) -> list:
    """files -> outcomes in order (DetectResult or the exception that file raised): `trace`'s decode / invert / batch path with this
    module's search in place of the registry search"""
    def batch(latents):
        cands = None
        if getattr(args, "ecc", None) is not None:
            from . import ecc as E
            results, reads = detect_payloads(latents, keyring, args.message_length, ecc=args.ecc, k=args.top, fpr=args.fpr, l=args.l,
                                             reliability=getattr(args, "reliability", 0), window_reliability=getattr(args, "window_reliability", 0),
                                             list_size=int(getattr(args, "ecc_list", 1) or 1))
            return [_PayloadOutcome(r, "" if e is None else ", " + E.format_any(e, 0, int(args.message_length), int(getattr(args, "ecc_list", 1) or 1), args.ecc))
                    for r, e in zip(results, reads)]
        if getattr(args, "align", "none") != "none":
            from . import align as AL
            cands = AL.alignments(args.align, int(args.align_shift), latents.shape[-2], latents.shape[-1])
            if getattr(args, "align_window_reliability", 0):
                return detect_latents_aligned_soft_l(latents, keyring, args.message_length, cands, args.l, levels=args.align_window_reliability, k=args.top,
                                                     fpr=args.fpr)
            if getattr(args, "align_reliability", 0):
                return detect_latents_aligned_soft(latents, keyring, args.message_length, cands, levels=args.align_reliability, k=args.top, fpr=args.fpr)
        if getattr(args, "window_reliability", 0):
            return detect_latents_soft_l(latents, keyring, args.message_length, args.l, levels=args.window_reliability, k=args.top, fpr=args.fpr)
        return detect_latents(latents, keyring, args.message_length, k=args.top, fpr=args.fpr, l=args.l, align=cands, reliability=getattr(args, "reliability", 0))

    return T._trace_files(files, args, keyring, trace_batch=batch)


def _report(job, outcomes, args, keyring, synthetic: bool) -> None:
    from . import extract as X
    from datetime import datetime
    with open(os.path.join(job.path, "detect.txt"), "a") as out:
        bar = "=" * 40
        fields = [("Time", datetime.now().strftime("%Y-%m-%d %H:%M:%S")), ("keyring", args.keyring), ("keys", len(keyring)),
                  ("message_length", args.message_length), ("l", args.l), ("fpr", args.fpr),
                  ("num_inference_steps", args.num_inference_steps), ("scheduler", args.scheduler)]
        if getattr(args, "align", "none") != "none":
            fields += [("align", args.align), ("align_shift", args.align_shift)]
        if getattr(args, "reliability", 0):
            fields += [("reliability", args.reliability)]
        if getattr(args, "align_reliability", 0):
            fields += [("align_reliability", args.align_reliability)]
        if getattr(args, "window_reliability", 0):
            fields += [("window_reliability", args.window_reliability)]
        if getattr(args, "align_window_reliability", 0):
            fields += [("align_window_reliability", args.align_window_reliability)]
        if getattr(args, "ecc", None) is not None:
            fields += [("ecc", args.ecc)]
            if int(getattr(args, "ecc_list", 1) or 1) > 1:
                fields += [("ecc_list", args.ecc_list)]
        out.write(f"{bar}Batch Info{bar}\n" + "".join(f"{k},{v}\n" for k, v in fields) + f"{bar}Batch Start{bar}\n")
        if synthetic:
            out.write(f"{X.SYNTHETIC_MARKER},'{args.model_id}' is not a local checkpoint: the detections below are not meaningful\n")
        for f, r in zip(job.files, outcomes):
            line = _line(f if isinstance(r, Exception) else os.path.basename(f), r)
            print(line)
            out.write(line + "\n")
        out.write(bar + "Batch End" + bar + "\n")


def main(argv=None):
    args = build_parser().parse_args(list(sys.argv[1:] if argv is None else argv))
    from . import extract as X
    _message_bytes(args.message_length)                            # fails before any model loads
    if ecc_refusal(args):
        raise SystemExit(ecc_refusal(args))
    if args.ecc is not None:
        from . import ecc as E
        E.check_length(args.message_length)
    if args.align_shift < 0 or (args.align == "none" and args.align_shift):
        raise SystemExit("--align_shift is a non-negative number of lattice steps and needs --align flips or --align d4")
    if args.reliability and (args.l != 1 or args.align != "none"):
        raise SystemExit("--reliability needs --l 1 and cannot be combined with --align yet")
    if args.align_reliability and (args.align == "none" or args.l != 1 or args.reliability):
        raise SystemExit("--align_reliability needs --align flips or --align d4 and --l 1, and cannot be combined with --reliability")
    if args.window_reliability and (args.l == 1 or args.align != "none" or args.reliability or args.align_reliability):
        raise SystemExit("--window_reliability needs --l 2 or --l 4 and cannot be combined with --align, --reliability or --align_reliability")
    if args.align_window_reliability:
        if args.align == "none":
            raise SystemExit("--align_window_reliability needs --align flips or --align d4 (without alignments: --window_reliability)")
        if args.l == 1:
            raise SystemExit("--align_window_reliability needs --l 2 or --l 4: at --l 1 the level-weighted alignment search is --align_reliability")
        if args.reliability or args.align_reliability or args.window_reliability:
            raise SystemExit("--align_window_reliability cannot be combined with --reliability, --align_reliability or --window_reliability")
    keyring = load_keyring(args.keyring)
    keyring.packed()
    synthetic = X._no_checkpoint(args.model_id)
    with X._strictness(args, synthetic):
        if args.images_directory_path != "":
            script = X._plan(args)
            jobs = [j for kind, j in script if kind == "job"]
            if any(j.files for j in jobs):
                X.load_models(args.model_id, allow_synthetic=X._synthetic_allowed(args))      # fail before touching any result file
            for kind, x in script:
                if kind == "banner":
                    print("=" * 20 + x + "=" * 20)
                elif x.files:
                    _report(x, _detect_files(x.files, args, keyring), args, keyring, synthetic)
        elif args.single_image_path != "":
            if synthetic:
                X.load_models(args.model_id, allow_synthetic=X._synthetic_allowed(args))
                print(f"{X.SYNTHETIC_MARKER}: '{args.model_id}' is not a local checkpoint, the detection below is not meaningful", file=sys.stderr)
            r = _detect_files([args.single_image_path], args, keyring)[0]
            print(_line(args.single_image_path if isinstance(r, Exception) else os.path.basename(args.single_image_path), r))
        else:
            print("Please set the argument 'images_directory_path' or 'single_image_path'")


if __name__ == "__main__":
    main()
