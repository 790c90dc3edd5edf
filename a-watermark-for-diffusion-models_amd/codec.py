"""Batch-first device API of the Gaussian-Shading codec: thin, stream-ordered wrappers over the C ABI.

Everything here runs on the current HIP device through libgswm.so; tensors are only used for device memory and
stream plumbing (`data_ptr()`, `torch.cuda.current_stream()`).  There is no CPU path.

Reference rows: E1-E6 -> `embed_batch`, X3-X5 -> `extract_batch`, X6 -> `bit_matches`,
X2/G1 elementwise step -> `ddim_step*`.
"""
from __future__ import annotations

import os
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as N
from .quant_table import THRESHOLDS

_DTYPES = {torch.float32: N.GSW_F32, torch.float16: N.GSW_F16, torch.bfloat16: N.GSW_BF16, torch.float64: N.GSW_F64}


def _stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def _need_gpu(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on a HIP device (got {t.device}); the watermark hot path has no CPU fallback")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if t.data_ptr() % 16:
        raise ValueError(f"{name} must be 16-byte aligned (got a view at an odd storage offset; .clone() it)")


def _same_device(t: torch.Tensor, ref: torch.Tensor, name: str):
    if t.device != ref.device:
        raise RuntimeError(f"{name} lives on {t.device}, expected {ref.device}")


def _like(t: torch.Tensor, ref: torch.Tensor, name: str, numel: Optional[int] = None):
    """A companion operand whose raw pointer crosses the C ABI next to `ref`: same device and dtype, contiguous, aligned, expected size.
    (A dtype mismatch would be read as the wrong bytes, a short tensor is an out-of-bounds device read: both are silent otherwise.)"""
    _need_gpu(t, name)
    _same_device(t, ref, name)
    if t.dtype != ref.dtype:
        raise ValueError(f"{name} is {t.dtype}, expected {ref.dtype}")
    if numel is not None and t.numel() != numel:
        raise ValueError(f"{name} has {t.numel()} elements, expected {numel}")


def _dt(t: torch.dtype) -> int:
    try:
        return _DTYPES[t]
    except KeyError:
        raise ValueError(f"unsupported dtype {t}") from None


def _check_key_nonce(key: bytes, nonce: bytes):
    # `cryptography` raises ValueError for wrong sizes (gs_insert.py:45)
    if len(key) != 32:
        raise ValueError("ChaCha20 key must be 32 bytes (256 bits)")
    if len(nonce) != 16:
        raise ValueError("ChaCha20 nonce must be 16 bytes (128 bits)")


WINDOWS = (1, 2, 4)             # supported --l: cipher bits per lattice element (windows that never straddle a byte)


def check_window(l) -> int:
    """The window size `l` as an int, or ValueError: 1, 2 and 4 are supported ("Multi-bit windows")."""
    if isinstance(l, bool) or not isinstance(l, (int, np.integer)) or int(l) not in WINDOWS:
        raise ValueError(f"l must be one of {WINDOWS} (cipher bits per lattice element), got {l!r}")
    return int(l)


def quant_thresholds(l: int) -> np.ndarray:
    """The 2**l - 1 float64 decision thresholds of y = int(norm.cdf(float64(z)) * 2**l): y == (z >= thresholds).sum().  The table the
    kernels are compiled with: tools/gen_quant_thresholds.py writes quant_table.py and csrc/quant_thresholds.inc from one bisection."""
    return np.array(THRESHOLDS[check_window(l)], dtype=np.float64)


# ------------------------------------------------------------------------------------------------ E1: host-side prep
def pad_message(message: str, msg_bytes: int = 32) -> bytes:
    """gs_insert.py:9-20 / nodes.py:68-76: UTF-8, zero-pad or truncate to msg_bytes; empty -> os.urandom."""
    if message:
        b = str(message).encode()
        return b + b"\x00" * (msg_bytes - len(b)) if len(b) < msg_bytes else b[:msg_bytes]
    return os.urandom(msg_bytes)


def resolve_key_nonce(key_hex: str, nonce_hex: str) -> Tuple[bytes, bytes]:
    """gs_insert.py:27-42: both given; key only -> nonce = key bytes 8..23; neither -> random."""
    if key_hex and nonce_hex:
        return bytes.fromhex(key_hex), bytes.fromhex(nonce_hex)
    if key_hex and not nonce_hex:
        return bytes.fromhex(key_hex), bytes.fromhex(key_hex[16:48])
    return os.urandom(32), os.urandom(16)


def choose_watermark_length(total_blocks_needed: int) -> int:
    """nodes.py:26-49."""
    for bits in (1024, 512, 256, 128, 64):
        if total_blocks_needed >= bits * 32:
            return bits
    return 32


# ------------------------------------------------------------------------------------------------ E2
def keystream(key: bytes, nonce: bytes, nbytes: int, device="cuda") -> torch.Tensor:
    """ChaCha20 keystream bytes (OpenSSL 16-byte nonce layout) as a uint8 device tensor."""
    _check_key_nonce(key, nonce)
    out = torch.empty(nbytes, dtype=torch.uint8, device=device)
    with torch.cuda.device(out.device):
        N.check(N.lib().gsw_keystream(key, nonce, out.data_ptr(), nbytes, _stream_ptr()))
    return out


# ------------------------------------------------------------------------------------------------ E3-E6
def _embed_operands(out: Optional[torch.Tensor], u: Optional[torch.Tensor], batch: int, shape: Sequence[int], n: int, dtype: torch.dtype, device,
                    ref: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[int]]:
    """The `out` / `u` operands of an embed -> (out, allocated when None, and u's pointer or None); ref: a tensor both must share the device of"""
    if out is None:
        out = torch.empty((batch, *shape), dtype=dtype, device=device)
    elif out.numel() != batch * n:
        raise ValueError("out has the wrong size")
    _need_gpu(out, "out")
    if ref is not None:
        _same_device(out, ref, "out")
    if u is None:
        return out, None
    _need_gpu(u, "u")
    if ref is not None:
        _same_device(u, ref, "u")
    if u.dtype != torch.float64 or u.numel() != batch * n:
        raise ValueError("u must be float64 with batch*n_elems entries")
    return out, u.data_ptr()


def embed_batch(key: bytes, nonce: bytes, k: bytes, batch: int, shape: Sequence[int], *, u: Optional[torch.Tensor] = None,
                seed: int = 0, image_index0: int = 0, dtype: torch.dtype = torch.float32, fast: bool = False,
                device="cuda", out: Optional[torch.Tensor] = None, l: int = 1) -> torch.Tensor:
    """Watermarked initial latents Z_s_T, shape [batch, *shape] (shape = (4, H/8, W/8)).

    u: optional float64 device tensor [batch, prod(shape)] of uniforms (the reference's np.random.uniform draws) for
       bit-parity with gs_insert.py:62-64; None -> in-kernel Philox4x32-7 keyed by (seed, image_index0 + b, element).
    fast: fp32 inverse-CDF core (|dz| <= 1e-5) instead of Cephes fp64.
    l: cipher bits per element (1, 2 or 4): z = ndtri((u + y) / 2**l) with y the element's l-bit window of the message repeated over
       n * l bits; for l > 1 the stored value is the nearest one of `dtype` that still quantises to y.
    """
    _check_key_nonce(key, nonce)
    l = check_window(l)
    n = 1
    for s in shape:
        n *= int(s)
    out, u_ptr = _embed_operands(out, u, batch, shape, n, dtype, device)
    mode = N.GSW_EMBED_FAST_F32 if fast else N.GSW_EMBED_EXACT_F64
    with torch.cuda.device(out.device):
        if l == 1:
            N.check(N.lib().gsw_embed(key, nonce, k, len(k), u_ptr, seed & (2**64 - 1), image_index0, out.data_ptr(), _dt(out.dtype),
                                      batch, n, mode, _stream_ptr()))
        else:
            N.check(N.lib().gsw_embed_l(key, nonce, k, len(k), u_ptr, seed & (2**64 - 1), image_index0, out.data_ptr(), _dt(out.dtype),
                                        batch, n, mode, l, _stream_ptr()))
    return out


def philox_uniform(seed: int, image_index0: int, batch: int, n_elems: int, device="cuda") -> torch.Tensor:
    """The u stream the embed kernel draws when no `u` is supplied ([batch, n_elems] float64)."""
    out = torch.empty((batch, n_elems), dtype=torch.float64, device=device)
    with torch.cuda.device(out.device):
        N.check(N.lib().gsw_philox_uniform(seed & (2**64 - 1), image_index0, out.data_ptr(), batch, n_elems, _stream_ptr()))
    return out


def mt19937_seed(seed: int) -> np.ndarray:
    """NumPy's legacy integer seeding (RandomState(seed) / np.random.seed(seed)): the 624 key words; pos starts at 624."""
    if not 0 <= int(seed) <= 0xFFFFFFFF:
        raise ValueError("Seed must be between 0 and 2**32 - 1")
    key = np.empty(624, dtype=np.uint32)
    N.lib().gsw_mt19937_seed(int(seed), key.ctypes.data)
    return key


def mt19937_uniform(n: int, rng=None, *, device="cuda") -> torch.Tensor:
    """n draws of `rng.uniform(0, 1)` (== legacy `random_sample`) generated ON THE DEVICE from the generator's current state:
    returns float64 [n] on the device and advances `rng` (a np.random.RandomState, or None for NumPy's global generator) exactly as
    the n host draws would -- gs_insert.py:62 / nodes.py:114-117 without shipping the uniforms over PCIe."""
    target = np.random if rng is None else rng
    state = target.get_state()
    if state[0] != "MT19937":
        raise ValueError("only the legacy MT19937 generator is supported")
    key = np.ascontiguousarray(state[1], dtype=np.uint32)
    out = torch.empty(int(n), dtype=torch.float64, device=device)
    st = torch.empty(625, dtype=torch.int32, device=device)
    with torch.cuda.device(out.device):
        N.check(N.lib().gsw_mt19937_uniform(key.ctypes.data, int(state[2]), out.data_ptr(), int(n), st.data_ptr(), _stream_ptr()))
    new = st.cpu().numpy().view(np.uint32)
    target.set_state(("MT19937", new[:624].copy(), int(new[624]), state[3], state[4]))
    return out


# ------------------------------------------------------------------------------------------------ X3-X5
def _vote_outputs(B: int, M: int, device, return_counts: bool):
    """What a vote writes -> (bits uint8 [B, ceil(M / 8)], flags int32 [B], counts int32 [B, M] or None)"""
    bits = torch.empty((B, (M + 7) // 8), dtype=torch.uint8, device=device)
    flags = torch.empty((B,), dtype=torch.int32, device=device)
    counts = torch.empty((B, M), dtype=torch.int32, device=device) if return_counts else None
    return bits, flags, counts


def extract_batch(z: torch.Tensor, key: bytes, nonce: bytes, message_length: int, *, return_counts: bool = False, l: int = 1):
    """Recover the message from latents z [B, ...] (any of fp16/bf16/fp32/fp64); l: cipher bits per element (1, 2 or 4), the
    lattice then holds n * l bits and each message bit gets n * l / message_length votes.

    Returns (bits uint8 [B, ceil(M/8)] MSB-first, flags int32 [B]) (+ counts int32 [B, M] '1'-votes).
    flags != 0 marks images for which the reference raises ValueError (saturated cdf / NaN), extract.py:84-86.
    Raises IndexError when the reference would (padded bit count not a multiple of message_length).
    """
    _check_key_nonce(key, nonce)
    l = check_window(l)
    _need_gpu(z, "z")
    B = z.shape[0]
    n = z.numel() // max(B, 1)
    M = int(message_length)
    bits, flags, counts = _vote_outputs(B, M, z.device, return_counts)
    with torch.cuda.device(z.device):
        if l == 1:
            N.check(N.lib().gsw_extract(z.data_ptr(), _dt(z.dtype), key, nonce, M, bits.data_ptr(),
                                        counts.data_ptr() if return_counts else None, flags.data_ptr(), B, n, _stream_ptr()))
        else:
            N.check(N.lib().gsw_extract_l(z.data_ptr(), _dt(z.dtype), key, nonce, M, bits.data_ptr(),
                                          counts.data_ptr() if return_counts else None, flags.data_ptr(), B, n, l, _stream_ptr()))
    return (bits, flags, counts) if return_counts else (bits, flags)


def bit_matches(bits: torch.Tensor, message_length: int, ref_msg: bytes, ref_bits: Optional[int] = None) -> torch.Tensor:
    """Per-image count of bits equal to ref_msg over min(message_length, ref_bits) positions (extract.py:103-110)."""
    _need_gpu(bits, "bits")
    B = bits.shape[0]
    out = torch.empty((B,), dtype=torch.int32, device=bits.device)
    rb = 8 * len(ref_msg) if ref_bits is None else ref_bits
    with torch.cuda.device(bits.device):
        N.check(N.lib().gsw_bit_matches(bits.data_ptr(), int(message_length), ref_msg, rb, out.data_ptr(), B, _stream_ptr()))
    return out


def bits_to_str(bits_row) -> str:
    """uint8 bytes (MSB-first) -> '0'/'1' string, the reference's return type (extract.py:101)."""
    return "".join(format(int(b), "08b") for b in bits_row)


# ------------------------------------------------------------------------------------------------ tracing (registry search)
def vote_copies(n_elems: int, message_length: int, l: int = 1) -> int:
    """Votes per message bit: the lattice padded to whole bytes (extract.py:88-92) splits into this many message_length-wide segments.
    Raises IndexError where `extract_batch` does (the padded bit count is not a multiple of message_length, extract.py:98).
    l: cipher bits per element; for l > 1 the lattice holds n_elems * l bits, which must fill whole bytes (ValueError otherwise)."""
    n, m = int(n_elems), int(message_length)
    l = check_window(l)
    if n <= 0 or m <= 0:
        raise ValueError("n_elems and message_length must be positive")
    if l > 1 and (n * l) % 8:
        raise ValueError(f"a lattice of {n} elements at l = {l} does not fill whole bytes")
    padded = (n * l + 7) // 8 * 8
    if padded % m:
        raise IndexError("string index out of range")
    return padded // m


def trace_topk(counts: torch.Tensor, copies: int, registry_bits: torch.Tensor, k: int = 1, soft: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k registry rows that best match each image's votes: (idx int32 [B, k], score int32 [B, k]), best first, ties towards the
    lower row; past the registry's end idx = -1 and score = INT32_MIN.

    counts: int32 [B, M] '1'-vote counts (`extract_batch(..., return_counts=True)`), copies: votes per bit (`vote_copies`),
    registry_bits: uint8 [U, M/8] messages packed MSB first (`trace.Registry.to_device`).
    score = sum_t (2 r[t] - 1) w[t] with w = 2 c - copies (soft) or the majority bit as +-1 (hard: score = 2 agree - M)."""
    _need_gpu(counts, "counts")
    _need_gpu(registry_bits, "registry_bits")
    if counts.dtype != torch.int32 or counts.dim() != 2:
        raise ValueError("counts must be int32 [B, M]")
    if registry_bits.dtype != torch.uint8 or registry_bits.dim() != 2:
        raise ValueError("registry_bits must be uint8 [U, M/8]")
    _same_device(registry_bits, counts, "registry_bits")
    B, M = counts.shape
    U = registry_bits.shape[0]
    if registry_bits.shape[1] * 8 != M:
        raise ValueError(f"registry rows hold {registry_bits.shape[1] * 8} bits, counts {M}")
    k = int(k)
    lib = N.lib()
    ws_bytes = lib.gsw_trace_workspace_bytes(B, U, k)
    if ws_bytes == 0:
        raise ValueError(f"libgswm: bad argument (B={B}, users={U}, k={k}: need B >= 1, 1 <= users < 2**31, 1 <= k <= 8)")
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=counts.device)
    idx = torch.empty((B, k), dtype=torch.int32, device=counts.device)
    score = torch.empty((B, k), dtype=torch.int32, device=counts.device)
    with torch.cuda.device(counts.device):
        N.check(lib.gsw_trace_topk(counts.data_ptr(), B, M, int(copies), N.GSW_TRACE_SOFT if soft else N.GSW_TRACE_HARD,
                                   registry_bits.data_ptr(), U, k, idx.data_ptr(), score.data_ptr(), ws.data_ptr(), _stream_ptr()))
    return idx, score


# ------------------------------------------------------------------------------------------------ tracing (records with their own keys)
KEYED_RECORD_HEAD = 48          # key[32] | nonce16[16], then the message
ROW_MAX_BITS = 1048576          # lattice bits of one image in the kernels that stage an image's row in LDS (csrc/gswm_record.h)


def keyed_record_stride(msg_bytes: int) -> int:
    """Bytes per row of a keyed registry: key | nonce | message, padded to a multiple of 16."""
    return (KEYED_RECORD_HEAD + int(msg_bytes) + 15) // 16 * 16


def _msg_bytes_arg(msg_bytes) -> int:
    """msg_bytes as an int, or ValueError"""
    if isinstance(msg_bytes, bool) or not isinstance(msg_bytes, (int, np.integer)) or not 1 <= int(msg_bytes) <= N.GSW_MSG_INLINE_MAX:
        raise ValueError(f"msg_bytes {msg_bytes!r} is outside 1..{N.GSW_MSG_INLINE_MAX}")
    return int(msg_bytes)


def _record_layout(stride: int, msg_bytes) -> int:
    """msg_bytes of a records operand with rows of `stride` bytes, as an int, or ValueError"""
    msg_bytes = _msg_bytes_arg(msg_bytes)
    if stride < KEYED_RECORD_HEAD + msg_bytes or stride % 16:
        raise ValueError(f"record rows of {stride} bytes cannot hold key | nonce | {msg_bytes}-byte message at a multiple of 16")
    return msg_bytes


def _key_layout(stride: int, msg_bytes) -> int:
    """... of a keys operand: a key row is a record's head, the bytes past it are ignored"""
    msg_bytes = _msg_bytes_arg(msg_bytes)
    if stride < KEYED_RECORD_HEAD or stride % 16:
        raise ValueError(f"key rows of {stride} bytes cannot hold key | nonce at a multiple of 16")
    return msg_bytes


def _search_operands(signs, n_bits, rows, msg_bytes, k, *, rows_name="records", rows_shape="[U, stride]", layout=_record_layout, prefix="", extras=()):
    """The checks the searches over packed sign rows share -> (B, U, stride, n_bits, msg_bytes, k).  rows: the records or keys; layout: their stride rule
    (`_record_layout` takes msg_bytes through int() first, as these searches always did; `_key_layout` as it is); extras: (tensor, name, check(B)) of further
    per-image operands, checked between the sign rows and `rows`."""
    _need_gpu(signs, prefix + "signs")
    for t, name, _ in extras:
        _need_gpu(t, name)
    _need_gpu(rows, rows_name)
    if signs.dtype != torch.uint8 or signs.dim() != 2:
        raise ValueError(f"{prefix}signs must be uint8 [B, n_bits / 8]")
    B = signs.shape[0]
    for _, _, check in extras:
        check(B)
    if rows.dtype != torch.uint8 or rows.dim() != 2:
        raise ValueError(f"{rows_name} must be uint8 {rows_shape}")
    for t, name in [e[:2] for e in extras] + [(rows, rows_name)]:
        _same_device(t, signs, name)
    n_bits = int(n_bits)
    if layout is _record_layout:
        msg_bytes = int(msg_bytes)
    k = int(k)
    if signs.shape[1] * 8 != n_bits:
        raise ValueError(f"sign rows hold {signs.shape[1] * 8} bits, n_bits is {n_bits}")
    return B, rows.shape[0], rows.shape[1], n_bits, layout(rows.shape[1], msg_bytes), k


def _search_outputs(workspace_bytes, B: int, U: int, k: int, what: str, device):
    """The workspace query of a search and its allocations -> (ws int64, idx int32 [B, k], score int32 [B, k])"""
    ws_bytes = workspace_bytes(B, U, k)
    if ws_bytes == 0:
        raise ValueError(f"libgswm: bad argument (B={B}, {what}={U}, k={k}: need B >= 1, 1 <= {what} < 2**31, 1 <= k <= 8)")
    return (torch.empty(ws_bytes // 8, dtype=torch.int64, device=device), torch.empty((B, k), dtype=torch.int32, device=device),
            torch.empty((B, k), dtype=torch.int32, device=device))


def sign_pack(z: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """X3 alone: the quantised sign bits of latents z [B, ...] (fp16/bf16/fp32/fp64), packed MSB first, before any decryption:
    (signs uint8 [B, n/8], flags int32 [B]); flags as `extract_batch` (a saturated element packs as 1, a NaN as 0).
    n must be a multiple of 8."""
    _need_gpu(z, "z")
    B = z.shape[0]
    n = z.numel() // max(B, 1)
    if n < 8 or n % 8:
        raise ValueError(f"sign_pack needs a lattice of a multiple of 8 elements per image (got {n})")
    signs = torch.empty((B, n // 8), dtype=torch.uint8, device=z.device)
    flags = torch.empty((B,), dtype=torch.int32, device=z.device)
    with torch.cuda.device(z.device):
        N.check(N.lib().gsw_sign_pack(z.data_ptr(), _dt(z.dtype), signs.data_ptr(), flags.data_ptr(), B, n, _stream_ptr()))
    return signs, flags


def quant_pack(z: torch.Tensor, l: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The l-bit form of `sign_pack`: y = int(norm.cdf(float64(z)) * 2**l) per element of latents z [B, ...], l bits each, MSB first:
    (packed uint8 [B, n * l / 8], flags int32 [B]); a saturated element packs as all ones, a NaN as zeros.  The operand of
    `trace_keyed_topk` with n_bits = n * l.  l == 1 is `sign_pack`."""
    l = check_window(l)
    if l == 1:
        return sign_pack(z)
    _need_gpu(z, "z")
    B = z.shape[0]
    n = z.numel() // max(B, 1)
    if n < 1 or (n * l) % 8:
        raise ValueError(f"quant_pack needs a lattice whose {l}-bit windows fill whole bytes (got {n} elements per image)")
    packed = torch.empty((B, n * l // 8), dtype=torch.uint8, device=z.device)
    flags = torch.empty((B,), dtype=torch.int32, device=z.device)
    with torch.cuda.device(z.device):
        N.check(N.lib().gsw_quant_pack(z.data_ptr(), _dt(z.dtype), packed.data_ptr(), flags.data_ptr(), B, n, l, _stream_ptr()))
    return packed, flags


def trace_keyed_topk(signs: torch.Tensor, n_bits: int, records: torch.Tensor, msg_bytes: int, k: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k records whose codeword best matches each image's sign bits: (idx int32 [B, k], score int32 [B, k]), best first, ties
    towards the lower row; past the registry's end idx = -1 and score = INT32_MIN.

    signs: uint8 [B, n_bits / 8] (`sign_pack`), records: uint8 [U, stride] rows key[32] | nonce[16] | message[msg_bytes]
    (`trace.KeyedRegistry.to_device`; stride >= 48 + msg_bytes, a multiple of 16).  The codeword of a record is what `embed_batch`
    plants for its key, nonce and message; score = n_bits - 2 popcount(signs ^ codeword).  Raises IndexError when n_bits is not a
    multiple of 8 msg_bytes (as `extract_batch` does for such a message length)."""
    B, U, stride, n_bits, msg_bytes, k = _search_operands(signs, n_bits, records, msg_bytes, k)
    lib = N.lib()
    ws, idx, score = _search_outputs(lib.gsw_trace_keyed_workspace_bytes, B, U, k, "records", signs.device)
    with torch.cuda.device(signs.device):
        N.check(lib.gsw_trace_keyed_topk(signs.data_ptr(), B, n_bits, records.data_ptr(), stride, msg_bytes, U, k,
                                         idx.data_ptr(), score.data_ptr(), ws.data_ptr(), _stream_ptr()))
    return idx, score


# ------------------------------------------------------------------------------------------------ blind key search (no message)
def key_search_topk(signs: torch.Tensor, n_bits: int, keys: torch.Tensor, msg_bytes: int, k: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k keys of a keyring under which each image looks most like a watermarked one, whatever the message: (idx int32 [B, k], stat
    int32 [B, k]), best first, ties towards the lower row; past the keyring's end idx = -1 and stat = INT32_MIN.

    signs: uint8 [B, n_bits / 8] (`sign_pack` / `quant_pack`), keys: uint8 [K, stride] rows key[32] | nonce[16], bytes past 48 ignored
    (`detect.Keyring.to_device`, or `trace.KeyedRegistry.to_device` as it is; stride >= 48, a multiple of 16).  With d the image's bits
    decrypted under a key and c_t the ones among the n_bits / (8 msg_bytes) copies of message position t, stat = sum_t |2 c_t - copies|:
    `trace_keyed_topk`'s score of the image's own majority-voted message (`detect.log10_p_blind` is its exact null tail).  One search
    launch (gsw_key_search_topk).  Raises IndexError when n_bits is not a multiple of 8 msg_bytes."""
    B, K, stride, n_bits, msg_bytes, k = _search_operands(signs, n_bits, keys, msg_bytes, k, rows_name="keys", rows_shape="[K, stride]", layout=_key_layout)
    lib = N.lib()
    ws, idx, stat = _search_outputs(lib.gsw_key_search_workspace_bytes, B, K, k, "keys", signs.device)
    with torch.cuda.device(signs.device):
        N.check(lib.gsw_key_search_topk(signs.data_ptr(), B, n_bits, keys.data_ptr(), stride, msg_bytes, K, k,
                                        idx.data_ptr(), stat.data_ptr(), ws.data_ptr(), _stream_ptr()))
    return idx, stat


# ------------------------------------------------------------------------------------------------ alignment search (flips, quarter turns, lattice shifts)
def align_table(aligns, shape: Sequence[int]) -> np.ndarray:
    """A list of alignments (d, dy, dx) for a [C, H, W] lattice as the int32 [A, 3] host table `rows_align` uploads, or ValueError: the list is
    empty or not [A, 3] integers, a d is outside 0..7, or an odd d (an odd number of quarter turns) meets H != W."""
    C_, H, W = _lattice_shape(shape)
    if isinstance(aligns, torch.Tensor):
        if aligns.dtype != torch.int32:
            raise ValueError(f"aligns must be an int32 [A, 3] tensor, got {aligns.dtype}")
        t = aligns.detach().cpu().numpy()
    else:
        try:
            t = np.asarray(list(aligns), dtype=np.int64)
        except (TypeError, ValueError):
            raise ValueError("aligns must be a list of (d, dy, dx) integer triples") from None
    if t.ndim != 2 or t.shape[1] != 3 or t.shape[0] < 1:
        raise ValueError(f"aligns must hold at least one (d, dy, dx) row, got shape {tuple(t.shape)}")
    if np.abs(t).max() >= 2 ** 31:
        raise ValueError("aligns does not fit int32")
    d = t[:, 0]
    if ((d < 0) | (d > 7)).any():
        raise ValueError(f"alignment d must be in 0..7, got {int(d[(d < 0) | (d > 7)][0])}")
    if H != W and (d & 1).any():
        raise ValueError(f"an odd d (a quarter turn) needs a square lattice, got H = {H}, W = {W}")
    return np.ascontiguousarray(t, dtype=np.int32)


def _lattice_shape(shape) -> Tuple[int, int, int]:
    try:
        C_, H, W = (int(s) for s in shape)
    except (TypeError, ValueError):
        raise ValueError(f"shape must be (C, H, W), got {shape!r}") from None
    if C_ < 1 or H < 1 or W < 1:
        raise ValueError(f"shape must be positive (C, H, W), got {shape!r}")
    return C_, H, W


def _rows_align_launch(packed: torch.Tensor, shape: Tuple[int, int, int], l: int, aligns_dev: torch.Tensor) -> torch.Tensor:
    """`rows_align` after its checks: packed uint8 [B, rowbytes] and an `align_table` on packed's device"""
    B, rowbytes = packed.shape
    A = aligns_dev.shape[0]
    out = torch.empty((B, A, rowbytes), dtype=torch.uint8, device=packed.device)
    with torch.cuda.device(packed.device):
        N.check(N.lib().gsw_rows_align(packed.data_ptr(), B, shape[0], shape[1], shape[2], l, aligns_dev.data_ptr(), A, out.data_ptr(), _stream_ptr()))
    return out


def rows_align(packed: torch.Tensor, shape: Sequence[int], l: int, aligns) -> torch.Tensor:
    """Every candidate alignment of packed quantised rows, in one launch: uint8 [B, A, rowbytes].

    packed: uint8 [B, C H W l / 8] (`sign_pack` / `quant_pack` of latents [B, C, H, W]); shape = (C, H, W); aligns: int32 [A, 3] rows
    (d, dy, dx) on packed's device, or a list of such triples that is uploaded here (`align.alignments`).  Row (b, a) of the result is
    bit for bit `quant_pack(align.apply(z[b], aligns[a]), l)`: the l-bit groups of the row are permuted (gsw_rows_align), nothing is
    quantised again, so every row is an operand of `key_search_topk`.  ValueError for a host tensor, a ragged lattice (C H W l is not a
    multiple of 8), more than 1 048 576 bits, l outside (1, 2, 4), an empty list, a d outside 0..7 and an odd d with H != W -- all before any
    launch.  A device list is copied to the host for that check; `align.search_keys` checks its list once for all its launches."""
    l = check_window(l)
    shape = _lattice_shape(shape)
    if not isinstance(packed, torch.Tensor) or not packed.is_cuda:
        raise ValueError(f"packed must live on a HIP device (got {getattr(packed, 'device', type(packed).__name__)}); rows_align has no CPU path")
    _need_gpu(packed, "packed")
    n_bits = shape[0] * shape[1] * shape[2] * l
    if n_bits % 8:
        raise ValueError(f"a lattice of {shape} at l = {l} holds {n_bits} bits: not whole bytes")
    if n_bits > ROW_MAX_BITS:
        raise ValueError(f"a lattice of {shape} at l = {l} holds {n_bits} bits, more than {ROW_MAX_BITS}")
    if packed.dtype != torch.uint8 or packed.dim() != 2 or packed.shape[0] < 1 or packed.shape[1] * 8 != n_bits:
        raise ValueError(f"packed must be uint8 [B, {n_bits // 8}] with B >= 1 for a lattice of {shape} at l = {l}, got {packed.dtype} {tuple(packed.shape)}")
    table = align_table(aligns, shape)
    if isinstance(aligns, torch.Tensor):
        _need_gpu(aligns, "aligns")
        _same_device(aligns, packed, "aligns")
        if aligns.dim() != 2:
            raise ValueError("aligns must be int32 [A, 3]")
        aligns_dev = aligns
    else:
        aligns_dev = torch.from_numpy(table).to(packed.device)
    return _rows_align_launch(packed, shape, l, aligns_dev)


COUNTS_ALIGN_MAX_BITS = 524288  # lattice bits of one image in `counts_align`: the row AND its keystream are staged in LDS (csrc/gswm_counts_align_plan.h)


def _counts_align_launch(packed: torch.Tensor, shape: Tuple[int, int, int], l: int, aligns_dev: torch.Tensor, key: bytes, nonce: bytes, msg_bits: int) -> torch.Tensor:
    """`counts_align` after its checks: packed uint8 [B, rowbytes], an `align_table` on packed's device, a checked key and nonce and a message length the lattice tiles"""
    B = packed.shape[0]
    A = aligns_dev.shape[0]
    counts = torch.empty((B, A, int(msg_bits)), dtype=torch.int32, device=packed.device)
    with torch.cuda.device(packed.device):
        N.check(N.lib().gsw_counts_align(packed.data_ptr(), B, shape[0], shape[1], shape[2], l, aligns_dev.data_ptr(), A, key, nonce, int(msg_bits),
                                         counts.data_ptr(), _stream_ptr()))
    return counts


def _counts_align_message(shape: Tuple[int, int, int], l: int, msg_bits) -> int:
    """msg_bits as `counts_align` takes it for a [C, H, W] lattice at l bits per element, or the refusal: ValueError (the 524 288-bit limit, a length outside
    8..2048 or not whole bytes), IndexError where `vote_copies` raises it"""
    if isinstance(msg_bits, bool) or not isinstance(msg_bits, (int, np.integer)) or not 8 <= int(msg_bits) <= 2048 or int(msg_bits) % 8:
        raise ValueError(f"msg_bits {msg_bits!r} must be a multiple of 8 in 8..2048")
    n_bits = shape[0] * shape[1] * shape[2] * l
    if n_bits > COUNTS_ALIGN_MAX_BITS:
        raise ValueError(f"a lattice of {shape} at l = {l} holds {n_bits} bits, more than the {COUNTS_ALIGN_MAX_BITS} that counts_align stages with their keystream")
    vote_copies(n_bits // l, int(msg_bits), l)
    return int(msg_bits)


def counts_align(packed: torch.Tensor, shape: Sequence[int], l: int, aligns, key: bytes, nonce: bytes, msg_bits: int) -> torch.Tensor:
    """The vote counts of every candidate alignment of packed quantised rows under one key, in one launch: int32 [B, A, msg_bits].

    packed, shape, l and aligns as `rows_align` takes them (a device table or a list that is uploaded here).  Row (b, a) of the result is bit
    for bit the counts of `extract_batch(align.apply(z[b], aligns[a]), key, nonce, msg_bits, return_counts=True, l=l)`: the '1' votes of every
    message position among the decrypted bits of `rows_align`'s row (b, a) (gsw_counts_align) -- the aligned rows themselves are never
    written.  Viewed as [B A, msg_bits] the result is the operand of `trace_topk`.  `rows_align`'s refusals with its messages, then ValueError
    for a lattice of more than 524 288 bits (the row and its keystream are both staged) and a msg_bits outside 8..2048 or not a multiple of 8,
    IndexError("string index out of range") where `vote_copies` raises it -- all before any launch."""
    _check_key_nonce(key, nonce)
    l = check_window(l)
    shape = _lattice_shape(shape)
    if not isinstance(packed, torch.Tensor) or not packed.is_cuda:
        raise ValueError(f"packed must live on a HIP device (got {getattr(packed, 'device', type(packed).__name__)}); counts_align has no CPU path")
    _need_gpu(packed, "packed")
    n_bits = shape[0] * shape[1] * shape[2] * l
    if n_bits % 8:
        raise ValueError(f"a lattice of {shape} at l = {l} holds {n_bits} bits: not whole bytes")
    msg_bits = _counts_align_message(shape, l, msg_bits)
    if packed.dtype != torch.uint8 or packed.dim() != 2 or packed.shape[0] < 1 or packed.shape[1] * 8 != n_bits:
        raise ValueError(f"packed must be uint8 [B, {n_bits // 8}] with B >= 1 for a lattice of {shape} at l = {l}, got {packed.dtype} {tuple(packed.shape)}")
    table = align_table(aligns, shape)
    if isinstance(aligns, torch.Tensor):
        _need_gpu(aligns, "aligns")
        _same_device(aligns, packed, "aligns")
        if aligns.dim() != 2:
            raise ValueError("aligns must be int32 [A, 3]")
        aligns_dev = aligns
    else:
        aligns_dev = torch.from_numpy(table).to(packed.device)
    return _counts_align_launch(packed, shape, l, aligns_dev, key, nonce, msg_bits)


# ------------------------------------------------------------------------------------------------ issuing (one record per image)
def _records_operand(records: torch.Tensor, msg_bytes: int) -> Tuple[int, int, int]:
    """The checks `embed_records` and `extract_records` share -> (B, stride, msg_bytes)"""
    _need_gpu(records, "records")
    if records.dtype != torch.uint8 or records.dim() != 2:
        raise ValueError("records must be uint8 [B, stride] (`trace.KeyedRegistry.packed` rows)")
    B, stride = records.shape[0], records.shape[1]
    if B < 1:
        raise ValueError("records holds no row")
    return B, stride, _record_layout(stride, msg_bytes)


def embed_records(records: torch.Tensor, msg_bytes: int, shape: Sequence[int], *, u: Optional[torch.Tensor] = None, seed: int = 0,
                  image_index0: int = 0, dtype: torch.dtype = torch.float32, fast: bool = False, out: Optional[torch.Tensor] = None,
                  l: int = 1) -> torch.Tensor:
    """Watermarked initial latents [B, *shape], image b under its OWN record, in one launch.

    records: uint8 [B, stride] on the device, a row is key[32] | nonce16[16] | message[msg_bytes] (`trace.KeyedRegistry.packed` rows as
    they are; stride >= 48 + msg_bytes, a multiple of 16).  Row b of the result is bit for bit
    `embed_batch(key_b, nonce_b, msg_b, 1, shape, u=u[b:b+1], seed=seed, image_index0=image_index0 + b, dtype=dtype, fast=fast, l=l)`;
    u, seed, fast, out and l as there."""
    B, stride, msg_bytes = _records_operand(records, msg_bytes)
    l = check_window(l)
    n = 1
    for s in shape:
        n *= int(s)
    if n < 4 or n % 4:
        raise ValueError(f"the lattice must hold a positive multiple of 4 elements per image (got {n})")
    out, u_ptr = _embed_operands(out, u, B, shape, n, dtype, records.device, ref=records)
    mode = N.GSW_EMBED_FAST_F32 if fast else N.GSW_EMBED_EXACT_F64
    with torch.cuda.device(out.device):
        N.check(N.lib().gsw_embed_keyed(records.data_ptr(), stride, msg_bytes, u_ptr, seed & (2**64 - 1), image_index0, out.data_ptr(),
                                        _dt(out.dtype), B, n, mode, l, _stream_ptr()))
    return out


def extract_records(z: torch.Tensor, records: torch.Tensor, msg_bytes: int, *, l: int = 1, return_counts: bool = False):
    """Recover and verify the message of every image under its OWN record, in one launch.

    z: latents [B, ...] (fp16 / bf16 / fp32 / fp64), records: as `embed_records`, one row per image.  Returns (bits uint8 [B, msg_bytes]
    MSB first, flags int32 [B], matches int32 [B]) (+ counts int32 [B, 8 msg_bytes]): bits, flags and counts of row b are those of
    `extract_batch(z[b:b+1], key_b, nonce_b, 8 * msg_bytes, l=l)`, matches[b] is how many of the recovered bits equal record b's
    message.  The n * l bits of an image must fill whole bytes and number at most 1 048 576 (ValueError otherwise); raises IndexError
    where `extract_batch` does (n * l is not a multiple of 8 msg_bytes)."""
    B, stride, msg_bytes = _records_operand(records, msg_bytes)
    l = check_window(l)
    _need_gpu(z, "z")
    _same_device(records, z, "records")
    if z.dim() < 2 or z.shape[0] != B:
        raise ValueError(f"z holds {z.shape[0] if z.dim() else 0} images, records {B} rows")
    dt = _dt(z.dtype)
    n = z.numel() // B
    if n < 1 or (n * l) % 8 or n * l > ROW_MAX_BITS:
        raise ValueError(f"a lattice of {n} elements at l = {l} must fill whole bytes and hold at most {ROW_MAX_BITS} bits")
    bits, flags, counts = _vote_outputs(B, 8 * msg_bytes, z.device, return_counts)
    matches = torch.empty((B,), dtype=torch.int32, device=z.device)
    with torch.cuda.device(z.device):
        N.check(N.lib().gsw_extract_keyed(z.data_ptr(), dt, records.data_ptr(), stride, msg_bytes, bits.data_ptr(),
                                          counts.data_ptr() if return_counts else None, flags.data_ptr(), matches.data_ptr(), B, n, l,
                                          _stream_ptr()))
    return (bits, flags, matches, counts) if return_counts else (bits, flags, matches)


# ------------------------------------------------------------------------------------------------ soft-decision vote and level rows (reliability levels; l = 1, 2, 4)
SOFT_MAX_LEVELS = 15


class SoftVote(NamedTuple):
    """What `extract_soft` returns, all on z's device"""
    bits: torch.Tensor      # uint8 [B, msg_bytes], MSB first, bit t = (score > 0)
    flags: torch.Tensor     # int32 [B], GSW_FLAG_*
    matches: torch.Tensor   # int32 [B], recovered bits equal to the record's message
    score: torch.Tensor     # int32 [B, 8 msg_bytes], sum of level (2 p - 1) over the copies of a message bit
    wsum: torch.Tensor      # int32 [B, 8 msg_bytes], the same sum of level alone
    wsq: torch.Tensor       # int32 [B], sum of level^2 over the image


class LevelRows(NamedTuple):
    """What `level_pack` returns, all on z's device: the operands of `trace_keyed_soft_topk`"""
    signs: torch.Tensor     # uint8 [B, n/8], `sign_pack`'s row
    planes: torch.Tensor    # uint8 [B, P, n/8], plane k = bit k of the levels, packed MSB first; P = bit length of `levels`
    wsum: torch.Tensor      # int32 [B], sum of level over the image
    wsq: torch.Tensor       # int32 [B], sum of level^2 over the image
    flags: torch.Tensor     # int32 [B], GSW_FLAG_*, as `sign_pack`


def level_planes(levels: int) -> int:
    """P: how many bit planes hold levels 0..`levels` (the bit length of `levels`, 1..4)"""
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not 1 <= int(levels) <= SOFT_MAX_LEVELS:
        raise ValueError(f"levels must be an int in 1..{SOFT_MAX_LEVELS}, got {levels!r}")
    return int(levels).bit_length()


def _level_table(thresholds: torch.Tensor, z: torch.Tensor, B: int, l: int) -> Tuple[int, int]:
    """The checks the votes and the packers share on the threshold table -> (levels, the stride between the images' tables in floats, 0 for one table for all).
    l = 1: [levels] or [B, levels]; l = 2, 4: a row per window bit, [l, levels] or [B, l, levels]."""
    _need_gpu(thresholds, "thresholds")
    _same_device(thresholds, z, "thresholds")
    own = thresholds.dim() - (2 if l > 1 else 1)                    # 0: one table for all, 1: a table per image
    if (thresholds.dtype != torch.float32 or own not in (0, 1) or (l > 1 and thresholds.shape[-2] != l) or (own == 1 and thresholds.shape[0] != B)):
        rows = "levels" if l == 1 else f"{l}, levels"
        raise ValueError(f"thresholds must be float32 [{rows}] or [{B}, {rows}]")
    levels = thresholds.shape[-1]
    if not 1 <= levels <= SOFT_MAX_LEVELS:
        raise ValueError(f"thresholds holds {levels} levels, supported are 1..{SOFT_MAX_LEVELS}")
    return levels, own * l * levels


def _soft_vote(z: torch.Tensor, records: torch.Tensor, msg_bytes: int, thresholds: torch.Tensor, l: int) -> SoftVote:
    """`extract_soft` (l = 1) and `extract_soft_l` (l = 2, 4): the operand checks, the outputs and the launch"""
    B, stride, msg_bytes = _records_operand(records, msg_bytes)
    _need_gpu(z, "z")
    _same_device(records, z, "records")
    if z.dim() < 2 or z.shape[0] != B:
        raise ValueError(f"z holds {z.shape[0] if z.dim() else 0} images, records {B} rows")
    levels, thr_stride = _level_table(thresholds, z, B, l)
    dt = _dt(z.dtype)
    n = z.numel() // B
    if n < 1 or n % 8 or n * l > ROW_MAX_BITS:
        raise ValueError(f"a lattice of {n} elements must fill whole bytes and hold at most {ROW_MAX_BITS} bits" if l == 1 else
                         f"a lattice of {n} elements at l = {l} must be a multiple of 8 elements and hold at most {ROW_MAX_BITS} bits")
    M, dev = 8 * msg_bytes, z.device                                # (z.device builds an object per read)
    bits = torch.empty((B, msg_bytes), dtype=torch.uint8, device=dev)
    flags = torch.empty((B,), dtype=torch.int32, device=dev)
    matches = torch.empty((B,), dtype=torch.int32, device=dev)
    score = torch.empty((B, M), dtype=torch.int32, device=dev)
    wsum = torch.empty((B, M), dtype=torch.int32, device=dev)
    wsq = torch.empty((B,), dtype=torch.int32, device=dev)
    window = () if l == 1 else (l,)                                 # gsw_extract_soft_l takes l after levels, gsw_extract_soft has no such argument
    with torch.cuda.device(dev):
        launch = N.lib().gsw_extract_soft if l == 1 else N.lib().gsw_extract_soft_l
        N.check(launch(z.data_ptr(), dt, records.data_ptr(), stride, msg_bytes, thresholds.data_ptr(), thr_stride, levels, *window, bits.data_ptr(),
                       score.data_ptr(), wsum.data_ptr(), wsq.data_ptr(), flags.data_ptr(), matches.data_ptr(), B, n, _stream_ptr()))
    return SoftVote(bits, flags, matches, score, wsum, wsq)


def _level_rows(z: torch.Tensor, thresholds: torch.Tensor, l: int) -> LevelRows:
    """`level_pack` (l = 1) and `level_pack_l` (l = 2, 4): the operand checks, the outputs and the launch"""
    _need_gpu(z, "z")
    if z.dim() < 2 or z.shape[0] < 1:
        raise ValueError("z must be [B, ...] with at least one image")
    B = z.shape[0]
    levels, thr_stride = _level_table(thresholds, z, B, l)
    dt = _dt(z.dtype)
    n = z.numel() // B
    if n < 8 or n % 8 or n * l > ROW_MAX_BITS:
        raise ValueError(f"level_pack needs a lattice of a multiple of 8 elements per image, at most {ROW_MAX_BITS} (got {n})" if l == 1 else
                         f"level_pack_l needs a lattice of a multiple of 8 elements per image and at most {ROW_MAX_BITS} bits (got {n} at l = {l})")
    P = level_planes(levels)
    nbytes, dev = n * l // 8, z.device
    signs = torch.empty((B, nbytes), dtype=torch.uint8, device=dev)
    planes = torch.empty((B, P, nbytes), dtype=torch.uint8, device=dev)
    wsum = torch.empty((B,), dtype=torch.int32, device=dev)
    wsq = torch.empty((B,), dtype=torch.int32, device=dev)
    flags = torch.empty((B,), dtype=torch.int32, device=dev)
    window = () if l == 1 else (l,)
    with torch.cuda.device(dev):
        launch = N.lib().gsw_level_pack if l == 1 else N.lib().gsw_level_pack_l
        N.check(launch(z.data_ptr(), dt, thresholds.data_ptr(), thr_stride, levels, *window, signs.data_ptr(), planes.data_ptr(), wsum.data_ptr(),
                       wsq.data_ptr(), flags.data_ptr(), B, n, _stream_ptr()))
    return LevelRows(signs, planes, wsum, wsq, flags)


def extract_soft(z: torch.Tensor, records: torch.Tensor, msg_bytes: int, thresholds: torch.Tensor) -> SoftVote:
    """The soft-decision vote of every image under its OWN record, in one launch (gsw_extract_soft, l = 1): element j votes for its
    decrypted bit with the integer weight level_j = #{ i : |z_j| >= thresholds[b][i] }.

    z: latents [B, ...] (fp16 / bf16 / fp32 / fp64), records: as `extract_records`, thresholds: float32 [levels] (one table for all images)
    or [B, levels] on z's device, levels in 1..15 (`soft.uniform_thresholds`, `soft.llr_thresholds`).  The comparison is exact in every
    dtype (fp32 after an exact widening; fp64 against the thresholds widened to fp64); a NaN has level 0.  With thresholds = [0] on
    NaN-free images the bits are `extract_records`' bits and score = 2 counts - copies.  Lattice limits and IndexError as `extract_records`."""
    return _soft_vote(z, records, msg_bytes, thresholds, 1)


def level_pack(z: torch.Tensor, thresholds: torch.Tensor) -> LevelRows:
    """Quantise and pack latents z [B, ...] (fp16/bf16/fp32/fp64) once for the level-weighted keyed search, in one launch (gsw_level_pack):
    the sign row of `sign_pack` bit for bit, the reliability level of every element -- `extract_soft`'s level_j = #{ i : |z_j| >=
    thresholds[b][i] }, same exact comparison, NaN -> 0 -- as P bit planes, and the image's sum of levels and of squared levels.
    thresholds: float32 [levels] or [B, levels] on z's device, levels in 1..15.  n must be a multiple of 8 and at most 1 048 576."""
    return _level_rows(z, thresholds, 1)


def _multi_bit_window(l, twin: str) -> int:
    """l as 2 or 4; l = 1 is refused with a pointer to the l = 1 function"""
    l = check_window(l)
    if l == 1:
        raise ValueError(f"l = 1 has one cipher bit per element and no window bits: use `{twin}`")
    return l


def extract_soft_l(z: torch.Tensor, records: torch.Tensor, msg_bytes: int, thresholds: torch.Tensor, l: int) -> SoftVote:
    """The soft-decision vote at l = 2 or 4, every image under its OWN record, in one launch (gsw_extract_soft_l): each of the n l cipher
    bits of an image votes for its decrypted value with an integer level, the distance of its element from the nearest quantiser boundary
    at which that bit would have come out differently.

    Element e holds z and the window y = (z >= quant_thresholds(l)).sum(); window bit w (0 = MSB of y, cipher position e l + w) has the
    value s = 2**(l-1-w) in y, a = (y // s) s and c = a + s are the flip boundaries around z, and
    level(e, w) = #{ i : (a == 0 or Z >= T_a + t_i) and (c == 2**l or Z <= T_c - t_i) }, t_i = thresholds[b][w][i], Z = z in float64, sums
    and compares in float64 -- exact in every dtype; a NaN has level 0.

    z: latents [B, ...] (fp16 / bf16 / fp32 / fp64), records: as `extract_records`, thresholds: float32 [l, levels] (one table for all
    images) or [B, l, levels] on z's device, levels in 1..15 (`soft.window_thresholds`).  Returns a `SoftVote` whose score and wsum sum over
    the copies of a message bit and whose wsq sums over all n l bits.  With one level at threshold 0 on NaN-free images the bits are
    `extract_records(..., l=l)`'s bits and score = 2 counts - copies.  n must be a multiple of 8 and n l at most 1 048 576 (ValueError);
    IndexError as `extract_records`.  l = 1 is refused: that is `extract_soft`."""
    l = _multi_bit_window(l, "extract_soft")
    return _soft_vote(z, records, msg_bytes, thresholds, l)


def level_pack_l(z: torch.Tensor, thresholds: torch.Tensor, l: int) -> LevelRows:
    """`level_pack` at l = 2 or 4, in one launch (gsw_level_pack_l): the row of `quant_pack(z, l)` bit for bit, `extract_soft_l`'s level of
    every cipher bit as P bit planes over the same n l bits, and the image's sum of levels and of squared levels -- the operands of
    `trace_keyed_soft_topk` and `key_search_soft_topk` with n_bits = n l.  thresholds: float32 [l, levels] or [B, l, levels] on z's device.
    n must be a multiple of 8 and n l at most 1 048 576; the searches refuse n l (1 + P) > 1 048 576.  l = 1 is refused: that is
    `level_pack`."""
    l = _multi_bit_window(l, "level_pack")
    return _level_rows(z, thresholds, l)


def _level_rows_checks(rows: "LevelRows", with_wsum: bool):
    """(planes_check, wsum_check) of a `LevelRows` operand for `_search_operands`' extras"""
    signs, planes, wsum = rows.signs, rows.planes, rows.wsum

    def planes_check(B):
        if planes.dtype != torch.uint8 or planes.dim() != 3 or planes.shape[0] != B or planes.shape[2] != signs.shape[1] or not 1 <= planes.shape[1] <= 4:
            raise ValueError(f"rows.planes must be uint8 [{B}, P, {signs.shape[1]}] with P in 1..4")

    def wsum_check(B):
        if wsum.dtype != torch.int32 or tuple(wsum.shape) != (B,):
            raise ValueError(f"rows.wsum must be int32 [{B}]")

    return ((planes, "rows.planes", planes_check),) + (((wsum, "rows.wsum", wsum_check),) if with_wsum else ())


def trace_keyed_soft_topk(rows: LevelRows, n_bits: int, records: torch.Tensor, msg_bytes: int, k: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """`trace_keyed_topk` ranked by reliability-weighted margins: (idx int32 [B, k], score int32 [B, k]), best first, ties towards the lower
    row; past the registry's end idx = -1 and score = INT32_MIN.

    rows: `level_pack`'s result for the images (signs [B, n_bits / 8], planes [B, P, n_bits / 8], wsum [B]; the number of levels is taken
    as 2**P - 1, which selects the same kernel as any `levels` with P planes), records: as `trace_keyed_topk`.
    score = sum_j level_j (1 - 2 (sign_j ^ codeword_j)) = wsum - 2 sum_k 2**k popcount(plane_k & (signs ^ codeword)); for records that share
    one key it is sum_t (2 r_t - 1) score[t] of `extract_soft`.  One search launch (gsw_trace_keyed_soft_topk); n_bits (1 + P) may not
    exceed 1 048 576 (ValueError).  Raises IndexError when n_bits is not a multiple of 8 msg_bytes."""
    signs, planes, wsum = rows.signs, rows.planes, rows.wsum
    B, U, stride, n_bits, msg_bytes, k = _search_operands(signs, n_bits, records, msg_bytes, k, prefix="rows.", extras=_level_rows_checks(rows, True))
    P = planes.shape[1]
    if n_bits * (1 + P) > ROW_MAX_BITS:
        raise ValueError(f"a lattice of {n_bits} bits with {P} level planes is beyond the search's domain: n_bits (1 + P) <= {ROW_MAX_BITS}")
    lib = N.lib()
    ws, idx, score = _search_outputs(lib.gsw_trace_keyed_workspace_bytes, B, U, k, "records", signs.device)
    with torch.cuda.device(signs.device):
        N.check(lib.gsw_trace_keyed_soft_topk(signs.data_ptr(), planes.data_ptr(), wsum.data_ptr(), (1 << P) - 1, B, n_bits, records.data_ptr(), stride,
                                              msg_bytes, U, k, idx.data_ptr(), score.data_ptr(), ws.data_ptr(), _stream_ptr()))
    return idx, score


# ------------------------------------------------------------------------------------------------ pooled evidence across the images of a set
POOL_MAX_PLANES = 10            # Q: planes of a pooled row, at most (csrc/gswm_pool_plan.h)


class PooledRows(NamedTuple):
    """What `pool_rows` returns, all on the rows' device: the operands of `trace_keyed_pooled_topk`"""
    signs: torch.Tensor     # uint8 [G, n/8], bit j = (S_j < 0)
    planes: torch.Tensor    # uint8 [G, Q, n/8], plane k = bit k of |S_j|, packed MSB first
    wsum: torch.Tensor      # int32 [G], sum_j |S_j|
    wsq: torch.Tensor       # int64 [G], sum_j S_j^2


def pool_planes(P: int, max_set: int) -> int:
    """Q: the bit length of Lmax * max_set, Lmax = 2**P - 1 (1 without planes) -- the planes that hold every pooled level of sets of at most
    `max_set` images; ValueError beyond `POOL_MAX_PLANES`."""
    lmax = (1 << P) - 1 if P else 1
    Q = (lmax * int(max_set)).bit_length()
    if Q > POOL_MAX_PLANES:
        raise ValueError(f"a set of {max_set} images at levels up to {lmax} needs {Q} planes: pool_rows holds at most {POOL_MAX_PLANES} "
                         f"(sets of at most {((1 << POOL_MAX_PLANES) - 1) // lmax} images at these levels)")
    return Q


def _pool_domain(n_bits: int, Q: int, what: str):
    if n_bits * (1 + Q) > ROW_MAX_BITS:
        raise ValueError(f"{what}: a lattice of {n_bits} bits with {Q} pooled planes is beyond the searches' domain: n_bits (1 + Q) <= {ROW_MAX_BITS}")
    if n_bits * ((1 << Q) - 1) >= 2 ** 31:
        raise ValueError(f"{what}: a lattice of {n_bits} bits with {Q} pooled planes is beyond int32 scores: n_bits (2**Q - 1) < 2**31")


def pool_rows(signs: torch.Tensor, planes: Optional[torch.Tensor], set_sizes: Sequence[int]) -> PooledRows:
    """Pool the packed rows of the images of every set into ONE row per set, in one launch (gsw_pool_rows): with lev_bj the level of element j of
    image b (1 without planes) and h_bj its sign bit, S_j = sum over the set of lev_bj (1 - 2 h_bj); the pooled sign bit is S_j < 0, the pooled
    level |S_j| (S_j = 0: sign 0, level 0).  A record's `trace_keyed_topk` / `trace_keyed_soft_topk` scores summed over a set are its
    `trace_keyed_pooled_topk` score on the pooled row: every score is linear in the image.

    signs: uint8 [B, n/8] (`sign_pack`, `quant_pack`, `level_pack`); planes: uint8 [B, P, n/8] with P in 1..4 (`level_pack`), or None for unit levels;
    set_sizes: the sizes of the G sets, whose images are contiguous in that order (sum = B, every size >= 1; the caller gathers).
    Q = `pool_planes(P, max(set_sizes))` planes come back: at most 1023 images per set at unit levels, 68 at 15 levels (ValueError beyond, before
    any launch); n (1 + Q) may not exceed 1 048 576 and n (2**Q - 1) must stay below 2**31."""
    _need_gpu(signs, "signs")
    if signs.dtype != torch.uint8 or signs.dim() != 2 or signs.shape[0] < 1 or signs.shape[1] < 1:
        raise ValueError("signs must be uint8 [B, n_bits / 8] with at least one image")
    B, nbytes = signs.shape
    P = 0
    if planes is not None:
        _need_gpu(planes, "planes")
        _same_device(planes, signs, "planes")
        if planes.dtype != torch.uint8 or planes.dim() != 3 or planes.shape[0] != B or planes.shape[2] != nbytes or not 1 <= planes.shape[1] <= 4:
            raise ValueError(f"planes must be uint8 [{B}, P, {nbytes}] with P in 1..4")
        P = planes.shape[1]
    sizes = [int(s) for s in set_sizes]
    if not sizes or min(sizes) < 1 or sum(sizes) != B:
        raise ValueError(f"set_sizes must be at least one set of at least one image each, {B} images in all (got {sizes[:8]}{'...' if len(sizes) > 8 else ''})")
    G, biggest = len(sizes), max(sizes)
    Q = pool_planes(P, biggest)
    _pool_domain(nbytes * 8, Q, "pool_rows")
    signs = signs.contiguous()
    planes = planes.contiguous() if planes is not None else None
    dev = signs.device
    set_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)).to(dev)
    out = PooledRows(torch.empty((G, nbytes), dtype=torch.uint8, device=dev), torch.empty((G, Q, nbytes), dtype=torch.uint8, device=dev),
                     torch.empty((G,), dtype=torch.int32, device=dev), torch.empty((G,), dtype=torch.int64, device=dev))
    with torch.cuda.device(dev):
        N.check(N.lib().gsw_pool_rows(signs.data_ptr(), planes.data_ptr() if planes is not None else None, P, B, nbytes * 8, set_ptr.data_ptr(), G, biggest, Q,
                                      out.signs.data_ptr(), out.planes.data_ptr(), out.wsum.data_ptr(), out.wsq.data_ptr(), _stream_ptr()))
    return out


def trace_keyed_pooled_topk(rows: PooledRows, n_bits: int, records: torch.Tensor, msg_bytes: int, k: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """`trace_keyed_soft_topk` for pooled rows: (idx int32 [G, k], score int32 [G, k]) per set, best first, ties towards the lower row; past the
    registry's end idx = -1 and score = INT32_MIN.

    rows: `pool_rows`' result (signs [G, n_bits / 8], planes [G, Q, n_bits / 8] with Q in 1..10, wsum [G]), records: as `trace_keyed_topk`.
    score = wsum - 2 sum_k 2**k popcount(plane_k & (signs ^ codeword)): the sum over the set's images of the record's per-image score.  One search
    launch (gsw_trace_keyed_pooled_topk); n_bits (1 + Q) may not exceed 1 048 576 (ValueError).  Raises IndexError when n_bits is not a multiple
    of 8 msg_bytes."""
    signs, planes, wsum = rows.signs, rows.planes, rows.wsum

    def planes_check(G):
        if planes.dtype != torch.uint8 or planes.dim() != 3 or planes.shape[0] != G or planes.shape[2] != signs.shape[1] or not 1 <= planes.shape[1] <= POOL_MAX_PLANES:
            raise ValueError(f"rows.planes must be uint8 [{G}, Q, {signs.shape[1]}] with Q in 1..{POOL_MAX_PLANES}")

    def wsum_check(G):
        if wsum.dtype != torch.int32 or tuple(wsum.shape) != (G,):
            raise ValueError(f"rows.wsum must be int32 [{G}]")

    G, U, stride, n_bits, msg_bytes, k = _search_operands(signs, n_bits, records, msg_bytes, k, prefix="rows.",
                                                          extras=((planes, "rows.planes", planes_check), (wsum, "rows.wsum", wsum_check)))
    Q = planes.shape[1]
    _pool_domain(n_bits, Q, "trace_keyed_pooled_topk")
    lib = N.lib()
    signs, planes = signs.contiguous(), planes.contiguous()
    ws, idx, score = _search_outputs(lib.gsw_trace_keyed_workspace_bytes, G, U, k, "records", signs.device)
    with torch.cuda.device(signs.device):
        N.check(lib.gsw_trace_keyed_pooled_topk(signs.data_ptr(), planes.data_ptr(), wsum.data_ptr(), Q, G, n_bits, records.data_ptr(),
                                                stride, msg_bytes, U, k, idx.data_ptr(), score.data_ptr(), ws.data_ptr(), _stream_ptr()))
    return idx, score


# ------------------------------------------------------------------------------------------------ error-corrected payloads: the Viterbi read of the votes
VITERBI_MIN_BITS, VITERBI_MAX_BITS = 64, 8192   # message bits of a coded message (csrc/gswm_viterbi_plan.h)
VITERBI_CODES = ("conv", "conv23", "conv34")    # rates 1/2, 2/3, 3/4: the index is the C entry points' `rate` (csrc/gswm_viterbi_rate_plan.h)


def viterbi_rate(code) -> int:
    if not isinstance(code, str) or code not in VITERBI_CODES:
        raise ValueError(f"code must be one of {VITERBI_CODES}, got {code!r}")
    return VITERBI_CODES.index(code)


def viterbi_kept_bits(steps: int, code="conv") -> int:
    """N(t): the code bits the first `steps` trellis steps keep -- (rate + 2) (t div P) + (0, 2, 3)[t mod P], P = rate + 1"""
    rate = viterbi_rate(code)
    return (rate + 2) * (steps // (rate + 1)) + (0, 2, 3)[steps % (rate + 1)]


def viterbi_steps(message_bits: int, code="conv") -> int:
    """T: the largest multiple of 8 with N(T) <= M"""
    T = int(message_bits) // 8 * 8
    while T > 0 and viterbi_kept_bits(T, code) > message_bits:
        T -= 8
    return T


class ViterbiDecode(NamedTuple):
    """What `viterbi_decode` returns, all on score's device"""
    info: torch.Tensor      # uint8 [B, T / 8] (M / 16 under "conv"), the I = T - 6 info bits MSB first: payload, CRC-16, 2 pad bits (the rest of the last byte is zero)
    message: torch.Tensor   # uint8 [B, M / 8], the re-encoded, re-interleaved codeword: the corrected message
    metric: torch.Tensor    # int32 [B], the winning path's correlation
    flips: torch.Tensor     # int32 [B], positions where the corrected message disagrees with score > 0
    ok: torch.Tensor        # int32 [B], 1: the CRC matches and the pad bits are zero


def viterbi_decode(score: torch.Tensor, code="conv") -> ViterbiDecode:
    """Decode the soft votes of B images under the rate-1/2, constraint-length-7 convolutional code of `ecc.encode`, in one launch
    (gsw_viterbi_decode, one wavefront per image): the maximum-correlation codeword for every row.

    score: int32 [B, M] on a HIP device, positive = bit 1 (`SoftVote.score`, `RobustVote.score`, 2 counts - copies); rows may be strided (a column
    slice of a wider tensor), elements may not; M a multiple of 16 in 64..8192 (ValueError); sum_t |score[b, t]| < 2**30 is the caller's bound,
    which every vote of this library keeps.  Integer arithmetic: the results equal tests/ecc_reference.py bit for bit.
    code: "conv" is that code and that launch; "conv23" / "conv34" are its punctured forms of rates 2/3 and 3/4 (gsw_viterbi_decode_rate; DESIGN.md
    section 4.31, tests/ecc_rate_reference.py): info has T / 8 bytes, message carries 0 at the M - N spare positions, flips counts the N code positions."""
    rate = viterbi_rate(code)
    if not isinstance(score, torch.Tensor) or score.dim() != 2 or score.dtype != torch.int32:
        raise ValueError("score must be an int32 tensor [B, message bits]")
    B, M = score.shape
    if M % 16 or not VITERBI_MIN_BITS <= M <= VITERBI_MAX_BITS:
        raise ValueError(f"score holds {M} message bits: a coded message has a multiple of 16 bits in {VITERBI_MIN_BITS}..{VITERBI_MAX_BITS}")
    if B < 1:
        raise ValueError("score holds no image")
    if not score.is_cuda:
        raise RuntimeError(f"score must live on a HIP device (got {score.device}); the watermark hot path has no CPU fallback")
    if score.stride(1) != 1 or (B > 1 and score.stride(0) < M):
        raise ValueError("score must have unit stride along the message and rows that do not overlap")
    if score.data_ptr() % 4:
        raise ValueError("score must be 4-byte aligned")
    stride = score.stride(0) if B > 1 else M
    dev = score.device
    out = ViterbiDecode(torch.empty((B, viterbi_steps(M, code) // 8), dtype=torch.uint8, device=dev), torch.empty((B, M // 8), dtype=torch.uint8, device=dev),
                        torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev),
                        torch.empty((B,), dtype=torch.int32, device=dev))
    with torch.cuda.device(dev):
        if rate == 0:
            N.check(N.lib().gsw_viterbi_decode(score.data_ptr(), stride, B, M, out.info.data_ptr(), out.message.data_ptr(), out.metric.data_ptr(),
                                               out.flips.data_ptr(), out.ok.data_ptr(), _stream_ptr()))
        else:
            N.check(N.lib().gsw_viterbi_decode_rate(score.data_ptr(), stride, B, M, rate, out.info.data_ptr(), out.message.data_ptr(),
                                                    out.metric.data_ptr(), out.flips.data_ptr(), out.ok.data_ptr(), _stream_ptr()))
    return out


VITERBI_LIST_SIZES = (1, 2, 4, 8)
VITERBI_LIST_LDS = 160 * 1024                   # one wavefront's LDS slice may take the LDS of a compute unit (csrc/gswm_viterbi_list_plan.h)


def viterbi_list_wave_lds(message_bits: int, list_size: int, code="conv") -> int:
    """bytes of LDS one image's list decode needs: 4 M + 256 L + 9 T L + M + T / 8, rounded up to 16 -- M (5 + 1/16 + 9 L / 2) + 256 L under "conv",
    where T = M / 2"""
    M, L, T = int(message_bits), int(list_size), viterbi_steps(message_bits, code)
    return (4 * M + 256 * L + 9 * T * L + M + T // 8 + 15) // 16 * 16


class ViterbiListDecode(NamedTuple):
    """What `viterbi_list_decode` returns, all on score's device; the first five describe the SELECTED path as `ViterbiDecode` describes its single path"""
    info: torch.Tensor      # uint8 [B, M / 16]
    message: torch.Tensor   # uint8 [B, M / 8]
    metric: torch.Tensor    # int32 [B]
    flips: torch.Tensor     # int32 [B]
    ok: torch.Tensor        # int32 [B]
    rank: torch.Tensor      # int32 [B], the selected rank: the lowest one whose CRC holds, 0 when none does
    n_ok: torch.Tensor      # int32 [B], the number of the L ranks whose CRC holds


def viterbi_list_decode(score: torch.Tensor, list_size: int, code="conv") -> ViterbiListDecode:
    """`viterbi_decode` with a list: every trellis state keeps its `list_size` = L best paths (L in 1, 2, 4, 8), and of the L paths that end in state 0
    the best-ranked one whose CRC holds is returned -- rank 0, the plain decode, when none does.  One launch (gsw_viterbi_list_decode, one wavefront
    per image); at L = 1 the first five tensors equal `viterbi_decode`'s.  DESIGN.md section 4.30 has the merge order and its tie rule.

    score: as `viterbi_decode`.  M a multiple of 16 from 64 up, as large as `viterbi_list_wave_lds(M, L)` <= 163 840 allows: 17 104, 11 600, 7 056,
    3 936 bits at L = 1, 2, 4, 8 (ValueError beyond).  Integer arithmetic: the results equal tests/ecc_list_reference.py bit for bit.
    code: as in `viterbi_decode`; the punctured codes go through gsw_viterbi_list_decode_rate and are bounded by `viterbi_list_wave_lds(M, L, code)`."""
    rate = viterbi_rate(code)
    if isinstance(list_size, bool) or not isinstance(list_size, int) or list_size not in VITERBI_LIST_SIZES:
        raise ValueError(f"list_size must be one of {VITERBI_LIST_SIZES}, got {list_size!r}")
    if not isinstance(score, torch.Tensor) or score.dim() != 2 or score.dtype != torch.int32:
        raise ValueError("score must be an int32 tensor [B, message bits]")
    B, M = score.shape
    if M % 16 or M < VITERBI_MIN_BITS:
        raise ValueError(f"score holds {M} message bits: a coded message has a multiple of 16 bits, {VITERBI_MIN_BITS} at least")
    if viterbi_list_wave_lds(M, list_size, code) > VITERBI_LIST_LDS:
        raise ValueError(f"score holds {M} message bits: at list_size {list_size} one image's survivor records need {viterbi_list_wave_lds(M, list_size, code)} "
                         f"bytes of LDS, more than the {VITERBI_LIST_LDS} of a compute unit")
    if B < 1:
        raise ValueError("score holds no image")
    if not score.is_cuda:
        raise RuntimeError(f"score must live on a HIP device (got {score.device}); the watermark hot path has no CPU fallback")
    if score.stride(1) != 1 or (B > 1 and score.stride(0) < M):
        raise ValueError("score must have unit stride along the message and rows that do not overlap")
    if score.data_ptr() % 4:
        raise ValueError("score must be 4-byte aligned")
    stride = score.stride(0) if B > 1 else M
    dev = score.device
    i32 = lambda: torch.empty((B,), dtype=torch.int32, device=dev)
    out = ViterbiListDecode(torch.empty((B, viterbi_steps(M, code) // 8), dtype=torch.uint8, device=dev),
                            torch.empty((B, M // 8), dtype=torch.uint8, device=dev), i32(), i32(), i32(), i32(), i32())
    with torch.cuda.device(dev):
        if rate == 0:
            N.check(N.lib().gsw_viterbi_list_decode(score.data_ptr(), stride, B, M, list_size, out.info.data_ptr(), out.message.data_ptr(),
                                                    out.metric.data_ptr(), out.flips.data_ptr(), out.ok.data_ptr(), out.rank.data_ptr(),
                                                    out.n_ok.data_ptr(), _stream_ptr()))
        else:
            N.check(N.lib().gsw_viterbi_list_decode_rate(score.data_ptr(), stride, B, M, rate, list_size, out.info.data_ptr(), out.message.data_ptr(),
                                                         out.metric.data_ptr(), out.flips.data_ptr(), out.ok.data_ptr(), out.rank.data_ptr(),
                                                         out.n_ok.data_ptr(), _stream_ptr()))
    return out


# ------------------------------------------------------------------------------------------------ blind key search ranked by reliability levels
def key_search_soft_topk(rows: LevelRows, n_bits: int, keys: torch.Tensor, msg_bytes: int, k: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """`key_search_topk` ranked by reliability levels: (idx int32 [B, k], stat int32 [B, k]), best first, ties towards the lower row; past
    the keyring's end idx = -1 and stat = INT32_MIN.

    rows: `level_pack`'s result for the images (signs [B, n_bits / 8], planes [B, P, n_bits / 8]; wsum is not read), keys: as
    `key_search_topk`.  With d the image's signs decrypted under a key and w_j the element's level from the planes,
    stat = sum_t |sum_{j mod 8 msg_bytes == t} w_j (2 d_j - 1)|: sum_t |score[t]| of `extract_soft` under that key, and with one plane of all
    ones `key_search_topk`'s stat (`detect.log10_p_blind_soft` bounds its null tail).  One search launch (gsw_key_search_soft_topk);
    n_bits (1 + P) may not exceed 1 048 576 (ValueError).  Raises IndexError when n_bits is not a multiple of 8 msg_bytes."""
    signs, planes = rows.signs, rows.planes
    B, K, stride, n_bits, msg_bytes, k = _search_operands(signs, n_bits, keys, msg_bytes, k, rows_name="keys", rows_shape="[K, stride]", layout=_key_layout,
                                                          prefix="rows.", extras=_level_rows_checks(rows, False))
    P = planes.shape[1]
    if n_bits * (1 + P) > ROW_MAX_BITS:
        raise ValueError(f"a lattice of {n_bits} bits with {P} level planes is beyond the search's domain: n_bits (1 + P) <= {ROW_MAX_BITS}")
    lib = N.lib()
    ws, idx, stat = _search_outputs(lib.gsw_key_search_soft_workspace_bytes, B, K, k, "keys", signs.device)
    with torch.cuda.device(signs.device):
        N.check(lib.gsw_key_search_soft_topk(signs.data_ptr(), planes.data_ptr(), P, B, n_bits, keys.data_ptr(), stride, msg_bytes, K, k,
                                             idx.data_ptr(), stat.data_ptr(), ws.data_ptr(), _stream_ptr()))
    return idx, stat


# ------------------------------------------------------------------------------------------------ alignment search ranked by reliability levels
def _level_rows_align_launch(rows: LevelRows, shape: Tuple[int, int, int], aligns_dev: torch.Tensor, l: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """`level_rows_align` (l = 1) and `level_rows_align_l` (l = 2, 4) after their checks -> (signs uint8 [B, A, rowbytes], planes uint8 [B, A, P, rowbytes])"""
    B, rowbytes = rows.signs.shape
    P, A = rows.planes.shape[1], aligns_dev.shape[0]
    signs = torch.empty((B, A, rowbytes), dtype=torch.uint8, device=rows.signs.device)
    planes = torch.empty((B, A, P, rowbytes), dtype=torch.uint8, device=rows.signs.device)
    window = () if l == 1 else (l,)                                 # gsw_level_rows_align_l takes l after P, gsw_level_rows_align has no such argument
    with torch.cuda.device(rows.signs.device):
        launch = N.lib().gsw_level_rows_align if l == 1 else N.lib().gsw_level_rows_align_l
        N.check(launch(rows.signs.data_ptr(), rows.planes.data_ptr(), P, *window, B, shape[0], shape[1], shape[2], aligns_dev.data_ptr(), A,
                       signs.data_ptr(), planes.data_ptr(), _stream_ptr()))
    return signs, planes


def _level_rows_align_checks(rows: LevelRows, shape, l: int = 1) -> Tuple[int, int, int]:
    """The operand checks of `level_rows_align` and, with l = 2 or 4, of `level_rows_align_l` (everything but the list of alignments) -> (C, H, W)"""
    shape = _lattice_shape(shape)
    signs, planes = rows.signs, rows.planes
    _need_gpu(signs, "rows.signs")
    n = shape[0] * shape[1] * shape[2] * l                          # the bits of a row
    at = "" if l == 1 else f" at l = {l}"
    if n % 8:
        raise ValueError(f"a lattice of {shape}{at} holds {n} bits: not whole bytes")
    if signs.dtype != torch.uint8 or signs.dim() != 2 or signs.shape[0] < 1 or signs.shape[1] * 8 != n:
        raise ValueError(f"rows.signs must be uint8 [B, {n // 8}] with B >= 1 for a lattice of {shape}{at}, got {signs.dtype} {tuple(signs.shape)}")
    B = signs.shape[0]
    for t, name, check in _level_rows_checks(rows, True) + ((rows.wsq, "rows.wsq", None), (rows.flags, "rows.flags", None)):
        _need_gpu(t, name)
        _same_device(t, signs, name)
        if check is not None:
            check(B)
        elif t.dtype != torch.int32 or tuple(t.shape) != (B,):
            raise ValueError(f"{name} must be int32 [{B}]")
    P = planes.shape[1]
    if n * (1 + P) > ROW_MAX_BITS:
        raise ValueError(f"a lattice of {n} bits with {P} level planes is beyond the search's domain: n_bits (1 + P) <= {ROW_MAX_BITS}")
    if B > 65535:
        raise ValueError(f"level_rows_align{'' if l == 1 else '_l'} takes at most 65535 images per launch, got {B}")
    return shape


def _aligns_operand(aligns, shape: Tuple[int, int, int], ref: torch.Tensor) -> torch.Tensor:
    """A list of alignments, or a device table, checked by `align_table` -> the int32 [A, 3] table on ref's device"""
    table = align_table(aligns, shape)
    if not isinstance(aligns, torch.Tensor):
        return torch.from_numpy(table).to(ref.device)
    _need_gpu(aligns, "aligns")
    _same_device(aligns, ref, "aligns")
    if aligns.dim() != 2:
        raise ValueError("aligns must be int32 [A, 3]")
    return aligns if aligns.is_contiguous() else aligns.contiguous()


def _aligned_level_rows(rows: LevelRows, signs: torch.Tensor, planes: torch.Tensor) -> LevelRows:
    """[B, A, ...] aligned rows as the `LevelRows` of B A images: wsum, wsq and flags are the image's, repeated (a permutation keeps them)"""
    B, A, rowbytes = signs.shape
    return LevelRows(signs.view(B * A, rowbytes), planes.view(B * A, planes.shape[2], rowbytes), rows.wsum.repeat_interleave(A), rows.wsq.repeat_interleave(A),
                     rows.flags.repeat_interleave(A))


def level_rows_align(rows: LevelRows, shape: Sequence[int], aligns) -> LevelRows:
    """Every candidate alignment of `level_pack`'s rows, in one launch (gsw_level_rows_align): signs uint8 [B A, n/8] and planes uint8
    [B A, P, n/8], row b A + a the rows of image b under aligns[a] -- the operand of `key_search_soft_topk` as it is.

    rows: `level_pack`'s result for latents [B, C, H, W]; shape = (C, H, W); aligns: int32 [A, 3] rows (d, dy, dx) on the rows' device, or a list
    of such triples that is uploaded here (`align.alignments`).  Every row is bit for bit `rows_align` of that input row at l = 1, and the rows of
    (b, a) are `level_pack(align.apply(z[b], aligns[a]), thresholds[b])` for the thresholds the rows were packed with: the kernel computes where
    an element comes from once and moves its sign and its level bits together.  wsum, wsq and flags are those of the image, repeated A times (a
    permutation keeps them).  RuntimeError for host tensors (there is no CPU fallback); ValueError for a ragged lattice, n (1 + P) beyond 1 048 576,
    more than 65 535 images, and the list checks of `rows_align` -- all before any launch."""
    shape = _level_rows_align_checks(rows, shape)
    aligns_dev = _aligns_operand(aligns, shape, rows.signs)
    return _aligned_level_rows(rows, *_level_rows_align_launch(rows, shape, aligns_dev))


def level_rows_align_l(rows: LevelRows, shape: Sequence[int], l: int, aligns) -> LevelRows:
    """`level_rows_align` at l = 2 or 4, in one launch (gsw_level_rows_align_l): every candidate alignment of `level_pack_l`'s rows, signs uint8
    [B A, n l / 8] and planes uint8 [B A, P, n l / 8], row b A + a the rows of image b under aligns[a] -- the operand of `key_search_soft_topk`
    and `trace_keyed_soft_topk` with n_bits = n l as it is.

    rows: `level_pack_l`'s result for latents [B, C, H, W] at that l; shape = (C, H, W); aligns as `level_rows_align` takes them.  Every row is bit
    for bit `rows_align` of that input row at l, and the rows of (b, a) are `level_pack_l(align.apply(z[b], aligns[a]), thresholds[b], l)` for the
    thresholds the rows were packed with: the kernel computes where an ELEMENT comes from once and moves its l window bits and the l level bits of
    every plane together.  wsum, wsq and flags are those of the image, repeated A times.  ValueError for l outside (2, 4) -- l = 1 is
    `level_rows_align` -- then `level_rows_align`'s refusals with n l bits per row: a ragged lattice, n l (1 + P) beyond 1 048 576, more than
    65 535 images, the list checks of `rows_align`; RuntimeError for host tensors -- all before any launch."""
    l = _multi_bit_window(l, "level_rows_align")
    shape = _level_rows_align_checks(rows, shape, l)
    aligns_dev = _aligns_operand(aligns, shape, rows.signs)
    return _aligned_level_rows(rows, *_level_rows_align_launch(rows, shape, aligns_dev, l))


# ------------------------------------------------------------------------------------------------ aligned registry search ranked by reliability levels
LEVEL_COUNTS_ALIGN_LDS_CAP = 131072     # bytes of LDS one image's rows, keystream and reduction region may take (csrc/gswm_counts_align_soft_plan.h)


def level_counts_align_lds_bytes(n_bits: int, P: int, msg_bits: int) -> int:
    """The LDS bytes of one `level_counts_align` workgroup, as csrc/gswm_counts_align_soft_plan.h lays them out: 1 + P rows padded to 16 bytes, the keystream in
    64-byte blocks, and one uint16 per position, lane and kind (score, wsum) of the reduction region"""
    rowbytes = n_bits // 8
    words = msg_bits % 32 == 0
    units = msg_bits // 32 if words else msg_bits // 8
    lanes = 256 // units * units
    return (1 + P) * ((rowbytes + 15) // 16 * 16) + 64 * ((rowbytes + 63) // 64) + 2 * lanes * (64 if words else 16)


def _level_counts_align_launch(rows: LevelRows, shape: Tuple[int, int, int], aligns_dev: torch.Tensor, key: bytes, nonce: bytes, msg_bits: int, bias: int = 0,
                               return_wsum: bool = False, l: int = 1):
    """`level_counts_align` after its checks: rows of a [C, H, W] lattice, an `align_table` on their device, a checked key and nonce, a message length the lattice
    tiles and a bias within `_level_counts_align_limits` -> score int32 [B, A, msg_bits], or (score, wsum)"""
    B, P, A = rows.signs.shape[0], rows.planes.shape[1], aligns_dev.shape[0]
    dev = rows.signs.device
    score = torch.empty((B, A, int(msg_bits)), dtype=torch.int32, device=dev)
    wsum = torch.empty_like(score) if return_wsum else None
    window = () if l == 1 else (l,)                                 # gsw_level_counts_align_l takes l after P
    with torch.cuda.device(dev):
        launch = N.lib().gsw_level_counts_align if l == 1 else N.lib().gsw_level_counts_align_l
        N.check(launch(rows.signs.data_ptr(), rows.planes.data_ptr(), P, *window, B, shape[0], shape[1], shape[2], aligns_dev.data_ptr(), A, key, nonce,
                       int(msg_bits), int(bias), score.data_ptr(), wsum.data_ptr() if return_wsum else None, _stream_ptr()))
    return (score, wsum) if return_wsum else score


def _level_counts_align_limits(shape: Tuple[int, int, int], P: int, msg_bits: int, bias, l: int = 1) -> int:
    """bias as `level_counts_align` (and, with l = 2 or 4, `level_counts_align_l`) takes it for a [C, H, W] lattice with P planes and a checked msg_bits, or
    ValueError: the staged regions pass the LDS cap, or |bias| + 15 copies leaves int32"""
    n = shape[0] * shape[1] * shape[2] * l                          # the bits of a row
    if isinstance(bias, bool) or not isinstance(bias, (int, np.integer)):
        raise ValueError(f"bias must be an int, got {bias!r}")
    lds = level_counts_align_lds_bytes(n, P, msg_bits)
    if lds > LEVEL_COUNTS_ALIGN_LDS_CAP:
        raise ValueError(f"a lattice of {shape}{'' if l == 1 else f' at l = {l}'} with {P} level planes and {msg_bits}-bit messages needs {lds} bytes of LDS in "
                         f"level_counts_align{'' if l == 1 else '_l'}, more than {LEVEL_COUNTS_ALIGN_LDS_CAP}")
    if abs(int(bias)) + SOFT_MAX_LEVELS * (n // msg_bits) >= 2 ** 31:
        raise ValueError(f"bias {bias} plus {SOFT_MAX_LEVELS} x {n // msg_bits} copies does not fit int32")
    return int(bias)


def level_counts_align(rows: LevelRows, shape: Sequence[int], aligns, key: bytes, nonce: bytes, msg_bits: int, *, bias: int = 0, return_wsum: bool = False):
    """The level-weighted vote of every candidate alignment of `level_pack`'s rows under one key, in one launch (gsw_level_counts_align): int32
    [B, A, msg_bits], or the pair (score, wsum) with return_wsum.

    rows, shape and aligns as `level_rows_align` takes them.  score[b, a] - bias and wsum[b, a] are bit for bit the `score` and `wsum` of
    `extract_soft(align.apply(z[b], aligns[a]), ...)` under (key, nonce) with the thresholds the rows were packed with: `counts_align` for level rows.  The
    aligned rows are never written.  With bias = levels * copies the scores, viewed as [B A, msg_bits], are the counts' of `trace.reliability_counts` and go
    to `trace_topk` as they are.  RuntimeError for host tensors (there is no CPU fallback); ValueError for `level_rows_align`'s refusals, a msg_bits outside
    8..2048 or not a multiple of 8, rows, keystream and reduction region beyond 128 KiB of LDS (a 4 x 128 x 128 lattice at 15 levels takes 80 KiB) and a bias
    that would leave int32; IndexError("string index out of range") where `vote_copies` raises it -- all before any launch."""
    _check_key_nonce(key, nonce)
    shape = _level_rows_align_checks(rows, shape)
    msg_bits = _counts_align_message(shape, 1, msg_bits)
    bias = _level_counts_align_limits(shape, rows.planes.shape[1], msg_bits, bias)
    aligns_dev = _aligns_operand(aligns, shape, rows.signs)
    return _level_counts_align_launch(rows, shape, aligns_dev, key, nonce, msg_bits, bias, bool(return_wsum))


def level_counts_align_l_lds_bytes(n_bits: int, P: int, msg_bits: int) -> int:
    """The LDS bytes of one `level_counts_align_l` workgroup for rows of n_bits = n l bits: `level_counts_align_lds_bytes` of such a row
    (csrc/gswm_counts_align_soft_l_plan.h lays the regions out as the l = 1 plan does)"""
    return level_counts_align_lds_bytes(n_bits, P, msg_bits)


def level_counts_align_l(rows: LevelRows, shape: Sequence[int], l: int, aligns, key: bytes, nonce: bytes, msg_bits: int, *, bias: int = 0, return_wsum: bool = False):
    """`level_counts_align` at l = 2 or 4, in one launch (gsw_level_counts_align_l): the level-weighted vote of every candidate alignment of
    `level_pack_l`'s rows under one key, int32 [B, A, msg_bits], or the pair (score, wsum) with return_wsum.

    rows, shape, l and aligns as `level_rows_align_l` takes them.  score[b, a] - bias and wsum[b, a] are bit for bit the `score` and `wsum` of
    `extract_soft_l(align.apply(z[b], aligns[a]), ..., l)` under (key, nonce) with the thresholds the rows were packed with, summed over the n l cipher
    positions.  The aligned rows are never written.  With bias = levels * copies, copies = n l / msg_bits, the scores viewed as [B A, msg_bits] are the
    counts' of `trace.reliability_counts` and go to `trace_topk` as they are.  ValueError for l outside (2, 4) -- l = 1 is `level_counts_align` -- then that
    function's refusals with n l bits per row (128 KiB of LDS hold a 4 x 64 x 64 lattice at l = 4 and 15 levels in 80 KiB) -- all before any launch."""
    _check_key_nonce(key, nonce)
    l = _multi_bit_window(l, "level_counts_align")
    shape = _level_rows_align_checks(rows, shape, l)
    msg_bits = _counts_align_message(shape, l, msg_bits)
    bias = _level_counts_align_limits(shape, rows.planes.shape[1], msg_bits, bias, l)
    aligns_dev = _aligns_operand(aligns, shape, rows.signs)
    return _level_counts_align_launch(rows, shape, aligns_dev, key, nonce, msg_bits, bias, bool(return_wsum), l)


# ------------------------------------------------------------------------------------------------ localising edits (tile map, tile-weighted vote)
TILES =(8, 16, 32)             # supported tile edges, in lattice elements


def _tiled_operands(packed: torch.Tensor, keys: torch.Tensor, msg_bits: int, shape: Sequence[int], l: int, tile: int):
    """The checks `tile_agreement` and `vote_tiled` share -> (B, C, h, w, l, tile, msg_bits, th, tw)"""
    l = check_window(l)
    if isinstance(tile, bool) or not isinstance(tile, (int, np.integer)) or int(tile) not in TILES:
        raise ValueError(f"tile must be one of {TILES} (lattice elements per tile edge), got {tile!r}")
    tile, M = int(tile), int(msg_bits)
    if len(shape) != 3 or any(int(s) < 1 for s in shape):
        raise ValueError(f"shape must be the (C, h, w) of one image's lattice, got {tuple(shape)!r}")
    C, h, w = (int(s) for s in shape)
    if h % tile or w % tile:
        raise ValueError(f"a {h} x {w} lattice is not a whole number of {tile} x {tile} tiles")
    if M < 8 or M % 8:
        raise ValueError(f"msg_bits must be a positive multiple of 8, got {M}")
    _need_gpu(packed, "packed")
    _need_gpu(keys, "keys")
    if packed.dtype != torch.uint8 or packed.dim() != 2:
        raise ValueError("packed must be uint8 [B, n * l / 8] (`quant_pack`)")
    B = packed.shape[0]
    if B < 1:
        raise ValueError("packed holds no image")
    if packed.shape[1] * 8 != C * h * w * l:
        raise ValueError(f"packed rows hold {packed.shape[1] * 8} bits, a {C} x {h} x {w} lattice at l = {l} has {C * h * w * l}")
    if keys.dtype != torch.uint8 or tuple(keys.shape) != (B, KEYED_RECORD_HEAD):
        raise ValueError(f"keys must be uint8 [{B}, {KEYED_RECORD_HEAD}]: key[32] | nonce16[16] per image")
    _same_device(keys, packed, "keys")
    return B, C, h, w, l, tile, M, h // tile, w // tile


def tile_agreement(packed: torch.Tensor, keys: torch.Tensor, messages: torch.Tensor, msg_bits: int, shape: Sequence[int], l: int = 1,
                   tile: int = 8) -> torch.Tensor:
    """Per tile, how many of an image's quantised bits equal the codeword of a message: int32 [B, h / tile, w / tile].

    packed: uint8 [B, n l / 8] (`quant_pack(z, l)`), keys: uint8 [B, 48] rows key[32] | nonce16[16], one PER IMAGE, messages: uint8
    [B, msg_bits / 8] MSB first, shape: the (C, h, w) of the lattice.  Tile (ty, tx) holds the elements of all C channels with
    y // tile == ty and x // tile == tx, n_t = C tile^2 l bits; the codeword is what `embed_batch` plants for that key, nonce and message.
    One launch; the keystreams are generated inside it.  Raises IndexError when n l is not a multiple of msg_bits (as `extract_batch`
    does), ValueError for a tile outside (8, 16, 32), a lattice that is not whole tiles or an l outside (1, 2, 4)."""
    B, C, h, w, l, tile, M, th, tw = _tiled_operands(packed, keys, msg_bits, shape, l, tile)
    _need_gpu(messages, "messages")
    if messages.dtype != torch.uint8 or tuple(messages.shape) != (B, M // 8):
        raise ValueError(f"messages must be uint8 [{B}, {M // 8}]")
    _same_device(messages, packed, "messages")
    agree = torch.empty((B, th, tw), dtype=torch.int32, device=packed.device)
    with torch.cuda.device(packed.device):
        N.check(N.lib().gsw_tile_agree(packed.data_ptr(), B, C, h, w, l, tile, keys.data_ptr(), messages.data_ptr(), M, agree.data_ptr(), _stream_ptr()))
    return agree


def vote_tiled(packed: torch.Tensor, keys: torch.Tensor, weights: torch.Tensor, msg_bits: int, shape: Sequence[int], l: int = 1,
               tile: int = 8) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The majority vote with one weight per tile: (bits uint8 [B, msg_bits / 8] MSB first, score int32 [B, msg_bits], wsum int32 [B, msg_bits]).

    Operands as `tile_agreement`; weights: uint16 [B, h / tile, w / tile].  With p_j the decrypted bit j of the image,
    score[t] = sum over j = t (mod msg_bits) of weight[tile of element j // l] (2 p_j - 1), wsum[t] the same sum of the weights, and
    bit t = score[t] > 0 (a tie, or no weight at all, gives 0).  Unit weights give `extract_batch`'s bits and score = 2 counts - copies.
    Raises IndexError / ValueError as `tile_agreement`."""
    B, C, h, w, l, tile, M, th, tw = _tiled_operands(packed, keys, msg_bits, shape, l, tile)
    _need_gpu(weights, "weights")
    if weights.dtype != torch.uint16 or tuple(weights.shape) != (B, th, tw):
        raise ValueError(f"weights must be uint16 [{B}, {th}, {tw}]")
    _same_device(weights, packed, "weights")
    bits = torch.empty((B, M // 8), dtype=torch.uint8, device=packed.device)
    score = torch.empty((B, M), dtype=torch.int32, device=packed.device)
    wsum = torch.empty((B, M), dtype=torch.int32, device=packed.device)
    with torch.cuda.device(packed.device):
        N.check(N.lib().gsw_vote_tiled(packed.data_ptr(), B, C, h, w, l, tile, keys.data_ptr(), weights.data_ptr(), M, bits.data_ptr(),
                                       score.data_ptr(), wsum.data_ptr(), _stream_ptr()))
    return bits, score, wsum


# ------------------------------------------------------------------------------------------------ robust decode in one launch (tile weights times reliability levels)
ROBUST_MAX_ITERS = 8
ROBUST_LDS_CAP = 131072         # bytes of LDS one image's decode may take (csrc/gswm_tamper_plan.h)


class RobustVote(NamedTuple):
    """What `decode_robust` returns, all on the rows' device: the last round of the decode"""
    bits: torch.Tensor      # uint8 [B, msg_bits / 8], MSB first, bit t = (score > 0)
    score: torch.Tensor     # int32 [B, msg_bits], sum of level weight (2 p - 1) over the copies of a message bit
    wsum: torch.Tensor      # int32 [B, msg_bits], the same sum of level weight alone
    excess: torch.Tensor    # int32 [B, th, tw], level-weighted agreement minus disagreement of a tile with the returned bits
    wsq: torch.Tensor       # int32 [B, th, tw], sum of level^2 over a tile
    weights: torch.Tensor   # int32 [B, th, tw], the tile weights the last vote used (ones when iters = 0)


def robust_lds_bytes(n_bits: int, P: int, tiles: int, msg_bits: int, level_rounds: bool) -> int:
    """The LDS one image's decode takes: the row padded to whole 64-byte blocks, P planes, the int32 tile weights (and the tiles' sums of levels
    and of squared levels when a round votes with the levels), the message bytes padded to a dword -- csrc/gswm_tamper_plan.h's layout"""
    rowbytes = n_bits // 8
    return 64 * ((rowbytes + 63) // 64) + P * rowbytes + 4 * tiles * (3 if level_rounds else 1) + (msg_bits // 8 + 3) // 4 * 4


def _small_int(v, name: str, lo: int, hi: int) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{name} must be an int in {lo}..{hi}, got {v!r}")
    return int(v)


def decode_robust(signs: torch.Tensor, planes: Optional[torch.Tensor], keys: torch.Tensor, msg_bits: int, shape: Sequence[int], l: int = 1, tile: int = 8,
                  iters: int = 2, sign_rounds: int = 0) -> RobustVote:
    """The robust decode of every image under its OWN key in ONE launch (gsw_decode_robust): `iters` + 1 rounds of vote, map and weights, every
    cipher bit voting with its reliability level times the weight of its tile.

    signs: uint8 [B, n l / 8] (`quant_pack` / `level_pack[_l]`), planes: uint8 [B, P, n l / 8] with P in 1..4 (`LevelRows.planes`) or None for
    unit levels, keys: uint8 [B, 48] as `vote_tiled`, shape: the (C, h, w) of the lattice.  With p_j the decrypted bit, lev_j the level the
    planes hold and L_j = 1 in round r < sign_rounds, lev_j after, the weights start at 1 and round r = 0 .. iters computes
    score[t] = sum over j = t (mod msg_bits) of L_j weight[tile of j // l] (2 p_j - 1), wsum[t] the same sum without the sign, bit t = score[t] > 0
    (a tie, or no weight at all, gives 0), excess[tile] = sum over the tile's bits of L_j (+1 where p_j agrees with its message bit, -1 where not),
    wsq[tile] = sum of L_j^2, and the next weights max(0, excess - isqrt(wsq)).  Returns the `RobustVote` of the last round.
    planes = None: bits, score and wsum of `tamper.extract_robust(..., iters=iters)` and excess = 2 agree - n_t.  iters = 0, sign_rounds = 0: the
    vote of `extract_soft[_l]`; iters = 0, sign_rounds = 1: the plain vote.
    Raises IndexError when n l is not a multiple of msg_bits, ValueError for what `vote_tiled` refuses, for P outside 0..4, iters outside 0..8,
    sign_rounds outside (0, 1), n l (1 + P) > 1 048 576, copies Lmax^2 n_t > 2^31 - 1 (Lmax = max(1, 2^P - 1), n_t = C tile^2 l, copies = n l /
    msg_bits: a score would not fit int32) and an LDS footprint above 131 072 bytes; RuntimeError for host tensors (there is no CPU fallback).
    All of it before any launch."""
    iters = _small_int(iters, "iters", 0, ROBUST_MAX_ITERS)
    sign_rounds = _small_int(sign_rounds, "sign_rounds", 0, 1)
    B, C, h, w, l, tile, M, th, tw = _tiled_operands(signs, keys, msg_bits, shape, l, tile)
    P = 0
    if planes is not None:
        _need_gpu(planes, "planes")
        if planes.dtype != torch.uint8 or planes.dim() != 3 or planes.shape[0] != B or planes.shape[2] != signs.shape[1] or not 1 <= planes.shape[1] <= 4:
            raise ValueError(f"planes must be uint8 [{B}, P, {signs.shape[1]}] with P in 1..4 (`level_pack`), or None for unit levels")
        _same_device(planes, signs, "planes")
        P = planes.shape[1]
    nb = C * h * w * l
    if nb > ROW_MAX_BITS or nb * (1 + P) > ROW_MAX_BITS:
        raise ValueError(f"a lattice of {nb} bits with {P} level planes is beyond the decode's domain: n_bits (1 + P) <= {ROW_MAX_BITS}")
    if nb % M:
        raise IndexError("string index out of range")
    lmax, n_t, copies = max(1, (1 << P) - 1), C * tile * tile * l, nb // M
    if copies * lmax * lmax * n_t > 2**31 - 1:
        raise ValueError(f"copies Lmax^2 n_t = {copies} x {lmax}^2 x {n_t} = {copies * lmax * lmax * n_t} does not fit int32: a bit's vote is at most "
                         f"Lmax = max(1, 2^P - 1) times a weight of at most Lmax n_t, n_t = C tile^2 l, summed over copies = n_bits / msg_bits")
    lds = robust_lds_bytes(nb, P, th * tw, M, P > 0 and iters >= sign_rounds)
    if lds > ROBUST_LDS_CAP:
        raise ValueError(f"the decode would take {lds} bytes of LDS (64 ceil(n_bits / 512) + P n_bits / 8 + 4 tiles (3 with levels, else 1) + msg_bits / 8), "
                         f"the cap is {ROBUST_LDS_CAP}")
    dev = signs.device
    bits = torch.empty((B, M // 8), dtype=torch.uint8, device=dev)
    score = torch.empty((B, M), dtype=torch.int32, device=dev)
    wsum = torch.empty((B, M), dtype=torch.int32, device=dev)
    excess = torch.empty((B, th, tw), dtype=torch.int32, device=dev)
    wsq = torch.empty((B, th, tw), dtype=torch.int32, device=dev)
    weights = torch.empty((B, th, tw), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        N.check(N.lib().gsw_decode_robust(signs.data_ptr(), planes.data_ptr() if planes is not None else None, P, B, C, h, w, l, tile, keys.data_ptr(), M, iters,
                                          sign_rounds, bits.data_ptr(), score.data_ptr(), wsum.data_ptr(), excess.data_ptr(), wsq.data_ptr(), weights.data_ptr(),
                                          _stream_ptr()))
    return RobustVote(bits, score, wsum, excess, wsq, weights)


# ------------------------------------------------------------------------------------------------ X2 / G1 elementwise
def ddim_step(x: torch.Tensor, model_out: torch.Tensor, a: float, b: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = a*x + b*model_out (fp32 math, one rounding). out may be x (in place)."""
    _need_gpu(x, "x"); _need_gpu(model_out, "model_out")
    if model_out.dtype != x.dtype or model_out.numel() != x.numel():
        raise ValueError("x / model_out mismatch")
    if out is None:
        out = torch.empty_like(x)
    _like(out, x, "out", x.numel())
    with torch.cuda.device(x.device):
        N.check(N.lib().gsw_ddim_step(x.data_ptr(), model_out.data_ptr(), out.data_ptr(), a, b, _dt(x.dtype), x.numel(), _stream_ptr()))
    return out


def ddim_step_cfg(x: torch.Tensor, e_uncond: torch.Tensor, e_text: torch.Tensor, a: float, b: float, guidance: float,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = a*x + b*(e_uncond + guidance*(e_text - e_uncond))."""
    _need_gpu(x, "x")
    _like(e_uncond, x, "e_uncond", x.numel()); _like(e_text, x, "e_text", x.numel())
    if out is None:
        out = torch.empty_like(x)
    _like(out, x, "out", x.numel())
    with torch.cuda.device(x.device):
        N.check(N.lib().gsw_ddim_step_cfg(x.data_ptr(), e_uncond.data_ptr(), e_text.data_ptr(), out.data_ptr(), a, b, guidance,
                                          _dt(x.dtype), x.numel(), _stream_ptr()))
    return out


def _dpm_step(x, e_uncond, e_text, pq, abc, guidance, m_prev, out, m_out):
    _need_gpu(x, "x")
    _like(e_uncond, x, "e_uncond" if e_text is not None else "model_out", x.numel())
    if e_text is not None:
        _like(e_text, x, "e_text", x.numel())
    (P, Q), (A, B, C) = pq, abc
    if m_prev is None and C != 0.0:
        raise ValueError("dpm_step: a second-order update (C != 0) needs m_prev")
    if m_prev is not None:
        _like(m_prev, x, "m_prev", x.numel())
    if out is None:
        out = torch.empty_like(x)
    if m_out is None:
        m_out = torch.empty_like(x)
    _like(out, x, "out", x.numel()); _like(m_out, x, "m_out", x.numel())
    with torch.cuda.device(x.device):
        N.check(N.lib().gsw_dpm_step(x.data_ptr(), e_uncond.data_ptr(), e_text.data_ptr() if e_text is not None else None,
                                     m_prev.data_ptr() if m_prev is not None else None, out.data_ptr(), m_out.data_ptr(),
                                     P, Q, A, B, C, guidance, _dt(x.dtype), x.numel(), _stream_ptr()))
    return out, m_out


def dpm_step(x: torch.Tensor, e: torch.Tensor, pq: Tuple[float, float], abc: Tuple[float, float, float], m_prev: Optional[torch.Tensor] = None, *,
             out: Optional[torch.Tensor] = None, m_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One DPM-Solver++ multistep scheduler step in one launch: m0 = P x + Q e (the x0 prediction, rounded as `ddim_step(x, e, P, Q)` rounds it),
    x' = A x + B m0 + C m_prev -> (x', m0).  out may be x and m_out may be m_prev (in place); m_prev is not read when C == 0."""
    return _dpm_step(x, e, None, pq, abc, 0.0, m_prev, out, m_out)


def dpm_step_cfg(x: torch.Tensor, e_uncond: torch.Tensor, e_text: torch.Tensor, pq: Tuple[float, float], abc: Tuple[float, float, float], guidance: float,
                 m_prev: Optional[torch.Tensor] = None, *, out: Optional[torch.Tensor] = None, m_out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """`dpm_step` on e = e_uncond + guidance (e_text - e_uncond), the guidance folded into the same launch."""
    return _dpm_step(x, e_uncond, e_text, pq, abc, guidance, m_prev, out, m_out)


def ddim_step_extract(x: torch.Tensor, model_out: torch.Tensor, a: float, b: float, key: bytes, nonce: bytes,
                      message_length: int, *, z_out: Optional[torch.Tensor] = None, return_counts: bool = False):
    """Last inversion step fused with the vote: z = a*x + b*model_out is quantised and voted without a round trip to HBM."""
    _check_key_nonce(key, nonce)
    _need_gpu(x, "x")
    _like(model_out, x, "model_out", x.numel())
    if z_out is not None:
        _like(z_out, x, "z_out", x.numel())
    B = x.shape[0]
    n = x.numel() // max(B, 1)
    M = int(message_length)
    bits, flags, counts = _vote_outputs(B, M, x.device, return_counts)
    with torch.cuda.device(x.device):
        N.check(N.lib().gsw_ddim_step_extract(x.data_ptr(), model_out.data_ptr(), z_out.data_ptr() if z_out is not None else None,
                                              a, b, _dt(x.dtype), key, nonce, M, bits.data_ptr(),
                                              counts.data_ptr() if return_counts else None, flags.data_ptr(), B, n, _stream_ptr()))
    return (bits, flags, counts) if return_counts else (bits, flags)


# ------------------------------------------------------------------------------------------------ eps-model fusions (X2 / G1)
def groupnorm_silu(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float, *, act: bool = True,
                   pre_bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = act(GroupNorm(x + pre_bias[:, :, None, None]) * gamma + beta) for NCHW x in one kernel (2 HBM passes)."""
    _need_gpu(x, "x")
    B, C = x.shape[0], x.shape[1]
    HW = x.numel() // max(B * C, 1)
    if out is None:
        out = torch.empty_like(x)
    _like(out, x, "out", x.numel())
    _like(gamma, x, "gamma", C); _like(beta, x, "beta", C)
    pb = None
    if pre_bias is not None:
        pre_bias = pre_bias.to(x.dtype).contiguous()
        _like(pre_bias, x, "pre_bias", B * C)
        pb = pre_bias.data_ptr()
    with torch.cuda.device(x.device):
        N.check(N.lib().gsw_groupnorm_silu(x.data_ptr(), pb, gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), B, C, HW, groups, eps,
                                           1 if act else 0, _dt(x.dtype), _stream_ptr()))
    return out


def geglu(x: torch.Tensor) -> torch.Tensor:
    """[..., 2*I] -> [..., I]: x[..., :I] * gelu(x[..., I:]) in one pass."""
    _need_gpu(x, "x")
    inner = x.shape[-1] // 2
    rows = x.numel() // (2 * inner)
    out = torch.empty((*x.shape[:-1], inner), dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        N.check(N.lib().gsw_geglu(x.data_ptr(), out.data_ptr(), rows, inner, _dt(x.dtype), _stream_ptr()))
    return out


def add_layernorm(x: torch.Tensor, delta: Optional[torch.Tensor], weight: torch.Tensor, bias: torch.Tensor, eps: float):
    """(x + delta, LayerNorm(x + delta)) in one kernel; delta=None -> (x, LayerNorm(x))."""
    _need_gpu(x, "x")
    C = x.shape[-1]
    rows = x.numel() // C
    _like(weight, x, "weight", C); _like(bias, x, "bias", C)
    y = torch.empty_like(x)
    xnew = x
    dptr = None
    if delta is not None:
        _like(delta, x, "delta", x.numel())
        xnew = torch.empty_like(x)
        dptr = delta.data_ptr()
    with torch.cuda.device(x.device):
        N.check(N.lib().gsw_add_layernorm(x.data_ptr(), dptr, weight.data_ptr(), bias.data_ptr(), xnew.data_ptr() if delta is not None else None,
                                          y.data_ptr(), rows, C, eps, _dt(x.dtype), _stream_ptr()))
    return xnew, y
