"""Error-corrected payloads: the M-bit message is a codeword of the rate-1/2, constraint-length-7 convolutional code (generators
0o171, 0o133, zero tail) over payload | CRC-16/CCITT-FALSE | pad, its code bits spread over the message by a multiplicative interleaver.  `encode` runs on
the host (a few hundred bit operations); `read` decodes the soft votes of a batch in one launch (`codec.viterbi_decode`, gsw_viterbi_decode) -- there is no
CPU decoder here.  The coded message is a message like any other: embed, registries, trace and the searches take it as it is.
`read_list` is the same read with a list: the decoder keeps the 2, 4 or 8 best paths and the CRC picks among them
(`codec.viterbi_list_decode`, gsw_viterbi_list_decode); what is issued does not change.
Punctured codes: `code="conv23"` / `"conv34"` puncture the same mother code to rates 2/3 and 3/4 -- 18 and 21 payload bytes in a
256-bit message against 13 -- and go through the same two reads (gsw_viterbi_decode_rate, gsw_viterbi_list_decode_rate); `code="conv"` is everything above,
unchanged."""
from __future__ import annotations

import math
from typing import List, NamedTuple

import numpy as np
import torch

from . import codec

G0, G1 = 0o171, 0o133
TAIL = 6
MIN_LENGTH, MAX_LENGTH = 64, 8192
CODES = ("conv", "conv23", "conv34")
# a code's puncture pattern: per phase of its period, which of (c0, c1) a step keeps, in this order (c0: 0o171, c1: 0o133; the DVB / 802.11 patterns)
PATTERNS = {"conv": ((0, 1),), "conv23": ((0, 1), (1,)), "conv34": ((0, 1), (1,), (0,))}


def check_code(ecc):
    """`ecc=` / `--ecc`: None or one of `CODES`"""
    if ecc is not None and (not isinstance(ecc, str) or ecc not in CODES):
        raise ValueError(f"ecc must be None or one of {CODES}, got {ecc!r}")
    return ecc


def code_rate(code) -> int:
    """a code's index in `CODES`: the `rate` of the C entry points (0, 1, 2 for 1/2, 2/3, 3/4)"""
    if not isinstance(code, str) or code not in CODES:
        raise ValueError(f"ecc: the code must be one of {CODES}, got {code!r}")
    return CODES.index(code)


def kept_bits(steps: int, code="conv") -> int:
    """N(t): the code bits the first `steps` trellis steps keep"""
    pattern = PATTERNS[CODES[code_rate(code)]]
    return sum(len(q) for q in pattern) * (steps // len(pattern)) + sum(len(q) for q in pattern[:steps % len(pattern)])


def trellis_steps(message_length, code="conv") -> int:
    """T: the largest multiple of 8 with N(T) <= M"""
    M = check_length(message_length)
    T = M // 8 * 8
    while kept_bits(T, code) > M:
        T -= 8
    return T


def check_length(message_length) -> int:
    M = message_length
    if isinstance(M, bool) or not isinstance(M, (int, np.integer)) or M % 16 or not MIN_LENGTH <= M <= MAX_LENGTH:
        raise ValueError(f"ecc: message_length must be a multiple of 16 in {MIN_LENGTH}..{MAX_LENGTH}, got {M!r}")
    return int(M)


def info_bits(message_length, code="conv") -> int:
    return trellis_steps(message_length, code) - TAIL


def capacity(message_length, code="conv") -> int:
    """payload bytes a message of `message_length` bits carries: (I - 16) // 8 with I = T - 6 (13, 18, 21 at M = 256 under conv, conv23, conv34)"""
    return (info_bits(message_length, code) - 16) // 8


def interleaver_step(message_length) -> int:
    """S: code bit i sits at message position (i S) mod M -- the smallest odd integer >= (isqrt(M) | 1) coprime to M"""
    M = check_length(message_length)
    S = math.isqrt(M) | 1
    while math.gcd(S, M) != 1:
        S += 2
    return S


def crc16(data: bytes) -> int:
    """CRC-16/CCITT-FALSE: polynomial 0x1021, init 0xFFFF, no reflection, no final xor"""
    crc = 0xFFFF
    for byte in bytes(data):
        crc ^= byte << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    return crc


def check_payload(payload, message_length, code="conv") -> bytes:
    if not isinstance(payload, (bytes, bytearray)):
        raise ValueError(f"ecc: a payload is bytes, got {type(payload).__name__}")
    cap = capacity(message_length, code)
    if len(payload) != cap:
        raise ValueError(f"ecc: a payload of {len(payload)} bytes; a message of {message_length} bits carries exactly {cap}")
    return bytes(payload)


def encode(payload: bytes, message_length: int, code="conv") -> bytes:
    """payload (exactly `capacity(message_length, code)` bytes) -> the coded message of message_length / 8 bytes; under a punctured code the kept bits
    take positions (j S) mod M in step order, then pattern order, and the spare positions carry 0"""
    payload = check_payload(payload, message_length, code)
    M, I = int(message_length), info_bits(message_length, code)
    pattern = PATTERNS[code]
    c = crc16(payload)
    word = np.unpackbits(np.frombuffer(payload + bytes([c >> 8, c & 0xFF]), dtype=np.uint8))
    u = np.concatenate([word, np.zeros(I - word.size + TAIL, dtype=np.uint8)])
    S, s = interleaver_step(M), 0
    msg = np.zeros(M, dtype=np.uint8)
    j = 0
    for t, bit in enumerate(u.tolist()):
        r = (bit << 6) | s
        for which in pattern[t % len(pattern)]:
            msg[j * S % M] = bin(r & (G1 if which else G0)).count("1") & 1
            j += 1
        s = r >> 1
    return np.packbits(msg).tobytes()


def pad_payload(payload, message_length: int, code="conv") -> bytes:
    """the CLI's convenience: text or bytes, cut or zero-padded to the capacity (as `codec.pad_message` does for messages; nothing random)"""
    raw = payload.encode() if isinstance(payload, str) else bytes(payload)
    cap = capacity(message_length, code)
    return raw[:cap] + b"\0" * max(0, cap - len(raw))


class EccRead(NamedTuple):
    """What `read` returns for a batch of B images"""
    payload: List[bytes]     # B payloads of `capacity(M)` bytes
    ok: List[bool]           # the CRC matches and the pad bits are zero
    flips: List[int]         # positions where the corrected message disagrees with score > 0
    metric: List[int]        # the winning path's correlation
    message: torch.Tensor    # uint8 [B, M / 8] on score's device: the corrected message, for `bit_matches` and the registries

    def image(self, b: int) -> "EccRead":
        return EccRead([self.payload[b]], [self.ok[b]], [self.flips[b]], [self.metric[b]], self.message[b:b + 1])


def read(score: torch.Tensor, code="conv") -> EccRead:
    """Decode soft votes score int32 [B, M] (positive = bit 1: `SoftVote.score`, `RobustVote.score`, or 2 counts - copies of
    `extract_batch(..., return_counts=True)`) in one launch; one device-to-host copy brings the small results over."""
    d = codec.viterbi_decode(score, code=code)
    M = score.shape[1]
    pb = capacity(M, code)
    info = d.info.cpu().numpy()
    small = torch.stack([d.ok, d.flips, d.metric]).cpu().numpy()
    return EccRead([info[b, :pb].tobytes() for b in range(info.shape[0])], [bool(v) for v in small[0]], [int(v) for v in small[1]], [int(v) for v in small[2]],
                   d.message)


LIST_SIZES = codec.VITERBI_LIST_SIZES


def check_list_size(list_size) -> int:
    """`list_size=` / `ecc_list=` / `--ecc_list`: 1 (the plain read), 2, 4 or 8"""
    if isinstance(list_size, bool) or not isinstance(list_size, (int, np.integer)) or int(list_size) not in LIST_SIZES:
        raise ValueError(f"ecc: the list size must be one of {LIST_SIZES}, got {list_size!r}")
    return int(list_size)


class EccListRead(NamedTuple):
    """What `read_list` returns for a batch of B images: `EccRead`'s fields for the SELECTED path, then which path that was"""
    payload: List[bytes]
    ok: List[bool]
    flips: List[int]
    metric: List[int]
    message: torch.Tensor    # uint8 [B, M / 8] on score's device
    rank: List[int]          # the rank of the selected path among the L best: the lowest whose CRC holds, 0 when none does
    n_ok: List[int]          # how many of the L paths pass the CRC; above 1 the CRC alone did not single the payload out

    def image(self, b: int) -> "EccListRead":
        return EccListRead([self.payload[b]], [self.ok[b]], [self.flips[b]], [self.metric[b]], self.message[b:b + 1], [self.rank[b]], [self.n_ok[b]])


def list_read_from_decode(d, message_length: int, code="conv") -> EccListRead:
    """the host side of `read_list`: the seven arrays of a list decode (device tensors or NumPy arrays) -> `EccListRead`"""
    host = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    pb = capacity(message_length, code)
    info = host(d.info)
    ints = lambda t: [int(v) for v in host(t)]
    return EccListRead([info[b, :pb].tobytes() for b in range(info.shape[0])], [bool(v) for v in host(d.ok)], ints(d.flips), ints(d.metric), d.message,
                       ints(d.rank), ints(d.n_ok))


def read_list(score: torch.Tensor, list_size: int, code="conv") -> EccListRead:
    """`read` with a list: the decoder keeps the `list_size` best paths and returns the best-ranked one whose CRC holds, in one
    launch (`codec.viterbi_list_decode`).  What was issued does not change; a row that carries no payload gets ok with probability at most
    list_size 2^-18 instead of 2^-18."""
    list_size = check_list_size(list_size)
    code_rate(code)
    if isinstance(score, torch.Tensor) and score.dim() == 2:
        check_length(score.shape[1])                                # payloads are defined for 64..8192 bits, whatever longer rows the kernel serves
    d = codec.viterbi_list_decode(score, list_size, code=code)
    small = torch.stack([d.ok, d.flips, d.metric, d.rank, d.n_ok]).cpu().numpy()    # one device-to-host copy for the five small results
    return list_read_from_decode(codec.ViterbiListDecode(d.info, d.message, small[2], small[1], small[0], small[3], small[4]), score.shape[1], code)


def read_any(score: torch.Tensor, list_size: int = 1, code="conv"):
    """`read` at list size 1 (today's launch and today's `EccRead`), `read_list` above"""
    return read(score, code) if check_list_size(list_size) == 1 else read_list(score, list_size, code)


def format_read_list(r: EccListRead, b: int, message_length: int, list_size: int, code="conv") -> str:
    """`format_read`'s text plus which of the `list_size` paths was selected, and how many pass when more than one does"""
    text = f"{format_read(r, b, message_length, code)}, list rank {r.rank[b]} of {list_size}"
    return text + (f", {r.n_ok[b]} candidates pass" if r.n_ok[b] > 1 else "")


def format_any(r, b: int, message_length: int, list_size: int = 1, code="conv") -> str:
    return format_read_list(r, b, message_length, list_size, code) if isinstance(r, EccListRead) else format_read(r, b, message_length, code)


def score_from_counts(counts: torch.Tensor, copies: int) -> torch.Tensor:
    """the plain vote as a score: 2 counts - copies (int32 [B, M])"""
    return (2 * counts.to(torch.int32) - int(copies)).contiguous()


def format_read(r: EccRead, b: int, message_length: int, code="conv") -> str:
    """the text the command-line tools append for image b: the flips are counted over the N code positions (N = M under "conv")"""
    n = message_length if code == "conv" else kept_bits(trellis_steps(message_length, code), code)
    return f"payload {r.payload[b].hex()} crc {'ok' if r.ok[b] else 'FAILED'}, corrected {r.flips[b]} of {n}"
