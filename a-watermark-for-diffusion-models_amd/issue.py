"""Issuing: a list of requests, each user with their own key, nonce and message -> watermarked initial latents in ONE embed launch,
plus the registry rows that `trace --per_record_keys` later reads.

The reference issues one watermark per run of gs_insert.py; with key and nonce left blank every run draws a fresh pair and appends it
to info_data.txt (gs_insert.py:27-42, 68-74).  A service that batches many users' requests does the same here for the whole batch:

    reqs = [issue.Request("alice", "alice@example"), issue.Request("bob", "bob@example")]
    latents, records = issue.issue_latents(reqs, registry=reg, log_path="info_data.txt")     # [2, 4, 64, 64], uint8 [2, stride]
    images, _, _ = pipe.txt2img(ctx, vae, latents=latents)
    ...
    bits, flags, matches = pipe.verify_records(x0, records, reg.message_bytes)               # each image against its own record

    python -m gswm_amd.issue --requests requests.tsv --registry registry.tsv --info_data info_data.txt --out_dir latents/
"""
from __future__ import annotations

import os
import re
import sys
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np

from . import codec, ecc as _ecc
from .trace import KeyedRegistry, _check_user_id

Record = Tuple[bytes, bytes, bytes]         # key[32], nonce[16], message


class Request:
    """One watermark to issue: `message` for `user_id` under `key` / `nonce` (bytes or hex strings).  Key and nonce left blank are
    drawn fresh for THIS request (what a first run of the reference does, gs_insert.py:40-42); a key without a nonce takes the nonce
    from the key's bytes 8..23 (gs_insert.py:33-36).  A str message is padded as gs_insert pads it (`codec.pad_message`), bytes must
    have the registry's message length."""

    __slots__ = ("user_id", "message", "key", "nonce")

    def __init__(self, user_id: str, message: Union[str, bytes], key: Union[str, bytes, None] = None, nonce: Union[str, bytes, None] = None):
        _check_user_id(user_id)
        if isinstance(message, str):
            if not message:
                raise ValueError(f"user {user_id!r}: an empty message string cannot be issued (pad_message would draw random bytes)")
        elif isinstance(message, (bytes, bytearray)):
            message = bytes(message)
        else:
            raise TypeError(f"user {user_id!r}: message must be str or bytes")
        key_hex, nonce_hex = (self._hex(x, user_id, what) for x, what in ((key, "key"), (nonce, "nonce")))
        if nonce_hex and not key_hex:
            raise ValueError(f"user {user_id!r}: a nonce without a key (leave both blank for a fresh pair)")
        try:
            k, n = codec.resolve_key_nonce(key_hex, nonce_hex)
        except ValueError:
            raise ValueError(f"user {user_id!r}: key and nonce must be hexadecimal") from None
        if len(k) != 32:
            raise ValueError(f"user {user_id!r}: the ChaCha20 key must be 32 bytes (got {len(k)})")
        if len(n) != 16:
            raise ValueError(f"user {user_id!r}: the ChaCha20 nonce must be 16 bytes (got {len(n)})")
        self.user_id, self.message, self.key, self.nonce = user_id, message, k, n

    @staticmethod
    def _hex(x, user_id: str, what: str) -> str:
        if x is None:
            return ""
        if isinstance(x, (bytes, bytearray)):
            return bytes(x).hex()
        if isinstance(x, str):
            return x.strip()
        raise TypeError(f"user {user_id!r}: {what} must be bytes or a hex string")

    def record(self, message_bytes: int) -> Record:
        """(key, nonce, message padded or checked to `message_bytes`)"""
        if isinstance(self.message, str):
            return self.key, self.nonce, codec.pad_message(self.message, message_bytes)
        if len(self.message) != message_bytes:
            raise ValueError(f"user {self.user_id!r}: message has {len(self.message)} bytes, {message_bytes}-byte messages are issued")
        return self.key, self.nonce, self.message

    def __repr__(self) -> str:
        return f"Request({self.user_id!r}, {self.message!r}, key={self.key.hex()}, nonce={self.nonce.hex()})"


def resolve_requests(requests: Sequence[Request], registry: Optional[KeyedRegistry] = None, message_bytes: int = 32) -> List[Record]:
    """The record of every request, in order, after every check that needs no device: message lengths, and against `registry` (and
    among the requests themselves) a user id already bound to another triple or a triple already bound to another user.  Nothing is
    added to the registry here."""
    if not requests:
        raise ValueError("no requests")
    mb = registry.message_bytes if registry is not None else int(message_bytes)
    if not 1 <= mb <= 256:
        raise ValueError("message_bytes must be in 1..256")
    by_id, by_record, out = {}, {}, []
    for r in requests:
        if not isinstance(r, Request):
            raise TypeError(f"expected issue.Request, got {type(r).__name__}")
        rec = r.record(mb)
        bound = registry.record(r.user_id) if registry is not None and r.user_id in registry._by_id else by_id.get(r.user_id)
        if bound is not None and bound != rec:
            raise ValueError(f"user id {r.user_id!r} is already bound to another key, nonce and message")
        owner = registry.user_at(registry._by_record[rec]) if registry is not None and rec in registry._by_record else by_record.get(rec)
        if owner is not None and owner != r.user_id:
            raise ValueError(f"user {r.user_id!r}: this key, nonce and message {rec[2].hex()} are already bound to {owner!r}")
        by_id[r.user_id], by_record[rec] = rec, r.user_id
        out.append(rec)
    return out


def encode_requests(requests: Sequence[Request], message_bytes: int, ecc: Optional[str]) -> List[Request]:
    """With ecc="conv" (or a punctured code, "conv23" / "conv34": more payload bytes, `ecc.capacity(M, ecc)`) the requests' messages are PAYLOADS: every request comes back with its payload encoded to the `message_bytes`-byte coded message
    (`ecc.encode`), which is what the registry, the log and the embed launch then see.  bytes must have exactly `ecc.capacity(8 message_bytes)` bytes, a
    str at most that many once encoded (zero-padded); anything else raises here, before anything runs.  ecc=None: the requests as they are."""
    if _ecc.check_code(ecc) is None:
        return list(requests)
    M = 8 * int(message_bytes)
    cap = _ecc.capacity(M, ecc)
    out = []
    for r in requests:
        if not isinstance(r, Request):
            raise TypeError(f"expected issue.Request, got {type(r).__name__}")
        raw = r.message.encode() if isinstance(r.message, str) else r.message
        if len(raw) > cap or (len(raw) != cap and not isinstance(r.message, str)):
            raise ValueError(f"user {r.user_id!r}: payload has {len(raw)} bytes, {message_bytes}-byte coded messages carry "
                             f"{'at most' if isinstance(r.message, str) else 'exactly'} {cap}")
        q = Request.__new__(Request)
        q.user_id, q.key, q.nonce, q.message = r.user_id, r.key, r.nonce, _ecc.encode(raw + b"\0" * (cap - len(raw)), M, ecc)
        out.append(q)
    return out


def pack_records(records: Sequence[Record], message_bytes: int) -> np.ndarray:
    """uint8 [B, stride] rows key | nonce | message, zero-padded to a multiple of 16 bytes: `KeyedRegistry.packed`'s row format"""
    t = np.zeros((len(records), codec.keyed_record_stride(message_bytes)), dtype=np.uint8)
    flat = np.frombuffer(b"".join(k + n + m for k, n, m in records), dtype=np.uint8)
    t[:, :codec.KEYED_RECORD_HEAD + message_bytes] = flat.reshape(len(records), codec.KEYED_RECORD_HEAD + message_bytes)
    return t


def write_log(log_path, records: Sequence[Record]) -> None:
    """one block of the reference's info_data.txt per image (gs_insert.py:68-74), which `KeyedRegistry.from_info_data` reads back"""
    from .gs_insert import _write_info
    for key, nonce, msg in records:
        _write_info(log_path, key, nonce, msg)


def issue_latents(requests: Sequence[Request], shape: Sequence[int] = (4, 64, 64), *, registry: Optional[KeyedRegistry] = None, log_path=None,
                  seed: Optional[int] = None, image_index0: int = 0, dtype=None, fast: bool = False, l: int = 1, device="cuda", ecc: Optional[str] = None):
    """Watermarked initial latents [B, *shape] for B requests, image b under request b's own record, after ONE embed launch:
    (latents, records) with records the uint8 [B, stride] device rows the launch read (`codec.extract_records` verifies against them).

    seed=None: the B * n uniforms come from NumPy's global MT19937, generated on the device (`codec.mt19937_uniform`): row b is what
    the b-th of B reference calls in a row would get, as `gs_watermark_init_noise_batch`; seed=int: in-kernel Philox by global image
    index image_index0 + b.  registry: every record is added under its user id BEFORE the launch (a clash raises before anything
    runs or changes); log_path: one info_data.txt block per image is appended.  Without a registry 32-byte messages are issued.
    ecc="conv": the requests' messages are payloads (`encode_requests`); registry rows, log blocks and `records` hold the CODED message."""
    import torch
    l = codec.check_window(l)
    mb = registry.message_bytes if registry is not None else 32
    requests = encode_requests(requests, mb, ecc)
    records = resolve_requests(requests, registry)
    n = 1
    for s in shape:
        n *= int(s)
    if registry is not None:
        for r, rec in zip(requests, records):
            if r.user_id not in registry._by_id:
                registry.add(r.user_id, *rec)
    if log_path:
        write_log(log_path, records)
    rows = torch.from_numpy(pack_records(records, mb)).to(device)
    B = len(records)
    u = codec.mt19937_uniform(B * n, device=device).view(B, n) if seed is None else None
    z = codec.embed_records(rows, mb, tuple(int(s) for s in shape), u=u, seed=seed or 0, image_index0=image_index0,
                            dtype=torch.float32 if dtype is None else dtype, fast=fast, l=l)
    return z, rows


# ===================================================================================================================== command line
def read_requests(path) -> List[Request]:
    """`user_id<TAB>message` or `user_id<TAB>message<TAB>key_hex<TAB>nonce_hex` per line (blank lines skipped; key_hex and nonce_hex may
    be empty columns)"""
    out = []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line.strip():
                continue
            cols = line.split("\t")
            if len(cols) not in (2, 4):
                raise ValueError(f"{path}:{no}: expected 'user_id<TAB>message' or 'user_id<TAB>message<TAB>key_hex<TAB>nonce_hex', got {len(cols)} columns")
            try:
                out.append(Request(cols[0], cols[1], *(c.strip() or None for c in cols[2:])))
            except (ValueError, TypeError) as e:
                raise ValueError(f"{path}:{no}: {e}") from None
    if not out:
        raise ValueError(f"{path}: no requests")
    return out


_DTYPES = ("float32", "float16", "float64")


def build_parser():
    import argparse
    p = argparse.ArgumentParser(prog="python -m gswm_amd.issue",
                                description="Issue watermarked initial latents for a file of requests, every user under their own key and nonce, in one "
                                            "embed launch (single GPU; image generation stays in the library: pipeline.txt2img(latents=...))")
    p.add_argument("--requests", required=True, help="'user_id<TAB>message[<TAB>key_hex<TAB>nonce_hex]' per line; blank key and nonce are drawn fresh per request")
    p.add_argument("--registry", required=True, help="four-column registry 'user_id<TAB>key_hex<TAB>nonce_hex<TAB>message_hex' (trace --per_record_keys "
                                                      "reads it): loaded when it exists, extended and saved")
    p.add_argument("--info_data", default=None, metavar="FILE", help="also append the reference's info_data.txt block per image")
    p.add_argument("--out_dir", default=None, metavar="DIR", help="write DIR/<user_id>.npy, the [4, height / 8, width / 8] latent of every request")
    p.add_argument("--message_bytes", type=int, default=32, help="message length of a NEW registry (an existing one keeps its own)")
    p.add_argument("--height", type=int, default=512, help="Height of the image the latents are for")
    p.add_argument("--width", type=int, default=512, help="Width of the image the latents are for")
    p.add_argument("--l", type=int, default=1, choices=codec.WINDOWS, help="cipher bits per lattice element")
    p.add_argument("--seed", type=int, default=None, help="in-kernel Philox stream of this seed (default: NumPy's global MT19937, as the reference draws)")
    p.add_argument("--dtype", default="float32", choices=_DTYPES)
    p.add_argument("--fast", action="store_true", help="fp32 inverse-CDF core (|dz| <= 1e-5)")
    p.add_argument("--ecc", default=None, choices=_ecc.CODES, help="the requests' messages are payloads of ecc.capacity(8 message_bytes) bytes (13 in a 32-byte "
                                                                   "message; 18 with conv23 and 21 with conv34, the punctured codes of rates 2/3 and 3/4): "
                                                                   "the registry and the latents carry their convolutional codeword")
    return p


def latent_file_names(user_ids: Sequence[str]) -> List[str]:
    """<user_id>.npy with everything outside [A-Za-z0-9._-] replaced by '_'; a name that repeats gets .2, .3, .. before the extension"""
    seen, out = {}, []
    for uid in user_ids:
        stem = re.sub(r"[^A-Za-z0-9._-]", "_", uid).lstrip(".") or "_"
        seen[stem] = seen.get(stem, 0) + 1
        out.append(f"{stem}.npy" if seen[stem] == 1 else f"{stem}.{seen[stem]}.npy")
    return out


def main(argv=None):
    args = build_parser().parse_args(list(sys.argv[1:] if argv is None else argv))
    if args.height % 8 or args.width % 8 or args.height < 8 or args.width < 8:
        raise ValueError("--height and --width must be positive multiples of 8")
    requests = read_requests(args.requests)
    registry = KeyedRegistry.load(args.registry) if os.path.exists(args.registry) and os.path.getsize(args.registry) else KeyedRegistry(args.message_bytes)
    requests = encode_requests(requests, registry.message_bytes, args.ecc)      # payloads -> coded messages, before anything else
    resolve_requests(requests, registry)                    # clashes and lengths: before the device is touched or a file written
    import torch
    latents, _ = issue_latents(requests, (4, args.height // 8, args.width // 8), registry=registry, log_path=args.info_data, seed=args.seed,
                               dtype=getattr(torch, args.dtype), fast=args.fast, l=args.l)
    registry.save(args.registry)
    if args.out_dir:
        os.makedirs(args.out_dir, exist_ok=True)
        host = latents.cpu().numpy()
        for name, z in zip(latent_file_names([r.user_id for r in requests]), host):
            np.save(os.path.join(args.out_dir, name), z)
    print(f"issued {len(requests)} latents for {len({r.user_id for r in requests})} users; registry {args.registry} holds {len(registry)} records")


if __name__ == "__main__":
    main()
