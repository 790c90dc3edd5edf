"""The refusal table of the level-weighted decoders (soft vote, level packer, the traces, detections and alignment searches built on them): one call per row,
shared by tools/gen_level_decoder_refusals.py, which records what every call raises into tests/golden/level_decoder_refusals.tsv, and by
tests/test_level_decoder_refusals.py, which replays the calls and compares.  The ORDER in which bad arguments are refused is behaviour: a row with two faults pins
which one wins.

Python rows.  `host`: plain host tensors, everything else valid -- the call must get as far as the device check ("HIP device") and no further.  `device`: the same
host tensors while `no_library(True)` makes every tensor say it lives on the device, so that a call gets past the device check to the checks behind it on a machine
without a device.  Nothing can launch meanwhile: the library is replaced by one that raises `Reached(<symbol>)` for everything but its host-only workspace queries,
so a row whose arguments are all valid records the symbol it would have launched.

C rows.  The four entry points with null or made-up pointers; every row carries at least one fault, so a correct library returns before it touches a pointer.  The
rows with made-up (non-null) pointers are replayed only where there is no device: there a library that lost a check cannot do harm."""
import contextlib

import torch

from gswm_amd import _native as N, align, codec, detect, soft, trace

KEY, NONCE = bytes(range(32)), bytes(range(16))
MB = 4                                      # message bytes: 32 bits, which tile the 256-element lattice below at l = 1, 2 and 4


class Reached(Exception):
    """Every check passed: the call arrived at this symbol of the library"""


class _NoLibrary:
    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        if name.endswith("workspace_bytes"):
            return getattr(self._real, name)
        raise Reached(name)


@contextlib.contextmanager
def no_library(on_device: bool):
    """Replace the library (see the module docstring); on_device: every tensor also claims to live on the device.

    These are patches of the whole process -- `N.lib`, `torch.cuda.device` and, on_device, the `is_cuda` of torch's own Tensor class -- undone on the way out.  They
    leave the code under test as it is (its own `_need_gpu` and `_same_device` run), but while they hold nothing else in this interpreter may use torch or the
    library: the rows are replayed one at a time in the test's own thread, and the suite does not run tests concurrently in one interpreter."""
    real_lib, real_ctx = N.lib, torch.cuda.device
    stub = _NoLibrary(real_lib())
    N.lib = lambda: stub
    torch.cuda.device = lambda d: contextlib.nullcontext()
    if on_device:
        torch.Tensor.is_cuda = property(lambda self: True)
    try:
        yield
    finally:
        if on_device:
            del torch.Tensor.is_cuda
        N.lib, torch.cuda.device = real_lib, real_ctx


def z(B=2, shape=(4, 8, 8), dtype=torch.float32):
    return torch.zeros((B, *shape), dtype=dtype)


def recs(B=2, mb=MB, stride=None, dtype=torch.uint8):
    return torch.zeros((B, codec.keyed_record_stride(mb) if stride is None else stride), dtype=dtype)


def thr(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


def off16(t):
    """the same values at a storage offset that is not 16-byte aligned"""
    flat = torch.zeros(t.numel() + 1, dtype=t.dtype)
    return flat[1:].view(t.shape)


def keyring(n=5):
    ring = detect.Keyring()
    for i in range(n):
        ring.add(f"key{i}", bytes([i]) * 32, bytes([i]) * 16)
    return ring


def registry(n=6, mb=MB):
    reg = trace.KeyedRegistry(mb)
    for i in range(n):
        reg.add(f"user{i}", bytes([i]) * 32, bytes([i]) * 16, bytes([i + 1]) * mb)
    return reg


FLIPS = align.alignments("flips", 1, 8, 8)
CASES = []                                  # (entry, tag, "host" | "device", thunk)


def case(entry, tag, thunk, where="device"):
    CASES.append((entry, tag, where, thunk))


# ---- codec: the vote -------------------------------------------------------------------------------------------------------------------------------------------
def vote_rows(entry, call, table, l):
    """call(z, records, msg_bytes, thresholds); table(*lead) -> a valid table with these leading dimensions"""
    t = lambda levels=3, **kw: table(levels, **kw)
    case(entry, "host", lambda: call(z(), recs(), MB, t()), "host")
    case(entry, "ok", lambda: call(z(), recs(), MB, t()))
    case(entry, "ok_per_image", lambda: call(z(), recs(), MB, t(batch=2)))
    case(entry, "ok_f16_15_levels", lambda: call(z(dtype=torch.float16), recs(), MB, t(15)))
    case(entry, "records_dtype", lambda: call(z(), recs(dtype=torch.int32), MB, t()))
    case(entry, "records_dim", lambda: call(z(), recs()[0], MB, t()))
    case(entry, "records_empty", lambda: call(z(), recs(B=0), MB, t()))
    case(entry, "records_strided", lambda: call(z(), recs(stride=128)[:, :64], MB, t()))
    case(entry, "records_off16", lambda: call(z(), off16(recs()), MB, t()))
    for mb in (0, 257, True, 4.0):
        case(entry, f"msg_bytes_{mb!r}", lambda mb=mb: call(z(), recs(), mb, t()))
    case(entry, "stride_short", lambda: call(z(), recs(stride=48), MB, t()))
    case(entry, "stride_odd", lambda: call(z(), recs(stride=72), MB, t()))
    case(entry, "z_images", lambda: call(z(B=3), recs(), MB, t()))
    case(entry, "z_dim", lambda: call(torch.zeros(2), recs(), MB, t()))
    case(entry, "z_strided", lambda: call(z(shape=(4, 8, 16))[..., :8], recs(), MB, t()))
    case(entry, "z_off16", lambda: call(off16(z()), recs(), MB, t()))
    case(entry, "z_dtype", lambda: call(z(dtype=torch.int32), recs(), MB, t()))
    case(entry, "thr_dtype", lambda: call(z(), recs(), MB, t(dtype=torch.float64)))
    case(entry, "thr_dim_low", lambda: call(z(), recs(), MB, t()[0]))
    case(entry, "thr_dim_high", lambda: call(z(), recs(), MB, t(batch=2)[None]))
    case(entry, "thr_images", lambda: call(z(), recs(), MB, t(batch=3)))
    case(entry, "thr_levels_0", lambda: call(z(), recs(), MB, t(0)))
    case(entry, "thr_levels_16", lambda: call(z(), recs(), MB, t(16)))
    case(entry, "lattice_ragged", lambda: call(z(shape=(4,)), recs(), MB, t()))
    case(entry, "lattice_at_limit", lambda: call(z(shape=(codec.ROW_MAX_BITS // l,), dtype=torch.float16), recs(), MB, t()))
    case(entry, "lattice_past_limit", lambda: call(z(shape=(codec.ROW_MAX_BITS // l + 8,), dtype=torch.float16), recs(), MB, t()))
    case(entry, "two_records_thr", lambda: call(z(), recs(dtype=torch.int32), MB, t(16)))
    case(entry, "two_msg_bytes_z", lambda: call(z(B=3), recs(), 0, t()))
    case(entry, "two_z_thr", lambda: call(z(B=3), recs(), MB, t(dtype=torch.float64)))
    case(entry, "two_thr_dtype", lambda: call(z(dtype=torch.int32), recs(), MB, t(16)))
    case(entry, "two_dtype_lattice", lambda: call(z(shape=(4,), dtype=torch.int32), recs(), MB, t()))
    case(entry, "two_thr_lattice", lambda: call(z(shape=(4,)), recs(), MB, t(0)))


vote_rows("codec.extract_soft", codec.extract_soft, lambda levels, batch=None, dtype=torch.float32: thr(*(() if batch is None else (batch,)), levels, dtype=dtype), 1)
for L in (2, 4):
    vote_rows(f"codec.extract_soft_l/{L}", lambda a, b, c, d, L=L: codec.extract_soft_l(a, b, c, d, L),
              lambda levels, batch=None, dtype=torch.float32, L=L: thr(*(() if batch is None else (batch,)), L, levels, dtype=dtype), L)
for bad in (1, 3, True, 2.0, None):
    case("codec.extract_soft_l", f"l_{bad!r}", lambda bad=bad: codec.extract_soft_l(z(), recs(), MB, thr(2, 3), bad))
case("codec.extract_soft_l", "thr_window", lambda: codec.extract_soft_l(z(), recs(), MB, thr(4, 3), 2))
case("codec.extract_soft_l", "thr_flat", lambda: codec.extract_soft_l(z(), recs(), MB, thr(2, 3), 4))
case("codec.extract_soft_l", "two_l_records", lambda: codec.extract_soft_l(z(), recs(dtype=torch.int32), MB, thr(2, 3), 1))
case("codec.extract_soft_l", "two_l_host", lambda: codec.extract_soft_l(z(), recs(), MB, thr(2, 3), 1), "host")


# ---- codec: the packer -----------------------------------------------------------------------------------------------------------------------------------------
def pack_rows(entry, call, table, l):
    t = lambda levels=3, **kw: table(levels, **kw)
    case(entry, "host", lambda: call(z(), t()), "host")
    case(entry, "ok", lambda: call(z(), t()))
    case(entry, "ok_per_image", lambda: call(z(), t(batch=2)))
    case(entry, "ok_f64_8_levels", lambda: call(z(dtype=torch.float64), t(8)))
    case(entry, "z_dim", lambda: call(torch.zeros(8), t()))
    case(entry, "z_empty", lambda: call(z(B=0), t()))
    case(entry, "z_strided", lambda: call(z(shape=(4, 8, 16))[..., :8], t()))
    case(entry, "z_off16", lambda: call(off16(z()), t()))
    case(entry, "z_dtype", lambda: call(z(dtype=torch.int64), t()))
    case(entry, "thr_dtype", lambda: call(z(), t(dtype=torch.float16)))
    case(entry, "thr_dim_low", lambda: call(z(), t()[0]))
    case(entry, "thr_dim_high", lambda: call(z(), t(batch=2)[None]))
    case(entry, "thr_images", lambda: call(z(), t(batch=1)))
    case(entry, "thr_strided", lambda: call(z(), t(6)[..., ::2]))
    case(entry, "thr_levels_0", lambda: call(z(), t(0)))
    case(entry, "thr_levels_16", lambda: call(z(), t(16)))
    case(entry, "lattice_ragged", lambda: call(z(shape=(12,)), t()))
    case(entry, "lattice_short", lambda: call(z(shape=(4,)), t()))
    case(entry, "lattice_at_limit", lambda: call(z(shape=(codec.ROW_MAX_BITS // l,), dtype=torch.float16), t()))
    case(entry, "lattice_past_limit", lambda: call(z(shape=(codec.ROW_MAX_BITS // l + 8,), dtype=torch.float16), t()))
    case(entry, "two_z_thr", lambda: call(torch.zeros(8), t(16)))
    case(entry, "two_thr_dtype", lambda: call(z(dtype=torch.int64), t(0)))
    case(entry, "two_dtype_lattice", lambda: call(z(shape=(12,), dtype=torch.int64), t()))
    case(entry, "two_thr_lattice", lambda: call(z(shape=(12,)), t(dtype=torch.float16)))


pack_rows("codec.level_pack", codec.level_pack, lambda levels, batch=None, dtype=torch.float32: thr(*(() if batch is None else (batch,)), levels, dtype=dtype), 1)
for L in (2, 4):
    pack_rows(f"codec.level_pack_l/{L}", lambda a, b, L=L: codec.level_pack_l(a, b, L),
              lambda levels, batch=None, dtype=torch.float32, L=L: thr(*(() if batch is None else (batch,)), L, levels, dtype=dtype), L)
for bad in (1, 3, True, 2.0, None):
    case("codec.level_pack_l", f"l_{bad!r}", lambda bad=bad: codec.level_pack_l(z(), thr(2, 3), bad))
case("codec.level_pack_l", "thr_window", lambda: codec.level_pack_l(z(), thr(4, 3), 2))
case("codec.level_pack_l", "two_l_z", lambda: codec.level_pack_l(torch.zeros(8), thr(2, 3), 1))
case("codec.level_pack_l", "two_l_host", lambda: codec.level_pack_l(z(), thr(2, 3), 1), "host")


# ---- soft: one key for the batch -----------------------------------------------------------------------------------------------------------------------------------
def shared_key_rows(entry, call, table):
    """call(latents, key, nonce, message_length, **kw)"""
    case(entry, "host", lambda: call(z(), KEY, NONCE, 32), "host")
    case(entry, "host_table", lambda: call(z(), KEY, NONCE, 32, thresholds=table()), "host")
    case(entry, "ok", lambda: call(z(), KEY, NONCE, 32))
    case(entry, "ok_3_levels", lambda: call(z(), KEY, NONCE, 32, levels=3, clip=1.5))
    case(entry, "ok_table", lambda: call(z(), KEY, NONCE, 32, thresholds=table()))
    for m in (0, 12, 2056, -8):
        case(entry, f"message_length_{m}", lambda m=m: call(z(), KEY, NONCE, m))
    for lv in (0, 16, True, 2.5):
        case(entry, f"levels_{lv!r}", lambda lv=lv: call(z(), KEY, NONCE, 32, levels=lv))
    for c in (0, float("nan"), float("inf"), "wide", True):
        case(entry, f"clip_{c!r}", lambda c=c: call(z(), KEY, NONCE, 32, clip=c))
    case(entry, "z_dim", lambda: call(torch.zeros(256), KEY, NONCE, 32))
    case(entry, "key_short", lambda: call(z(), KEY[:31], NONCE, 32))
    case(entry, "nonce_long", lambda: call(z(), KEY, NONCE + b"x", 32))
    case(entry, "table_levels_16", lambda: call(z(), KEY, NONCE, 32, thresholds=table(16)))
    case(entry, "lattice_ragged", lambda: call(z(shape=(4, 3, 4)), KEY, NONCE, 32))
    case(entry, "two_message_levels", lambda: call(z(), KEY, NONCE, 12, levels=0))
    case(entry, "two_levels_key", lambda: call(z(), KEY[:31], NONCE, 32, levels=0))
    case(entry, "two_key_table", lambda: call(z(), KEY[:31], NONCE, 32, thresholds=table(16)))
    case(entry, "two_message_host", lambda: call(z(), KEY, NONCE, 12), "host")


shared_key_rows("soft.extract_soft", soft.extract_soft, lambda levels=3: thr(levels))
for L in (1, 2, 4):
    shared_key_rows(f"soft.extract_soft_l/{L}", lambda *a, L=L, **kw: soft.extract_soft_l(*a, L, **kw), lambda levels=3, L=L: thr(levels) if L == 1 else thr(L, levels))
for bad in (3, True, "2"):
    case("soft.extract_soft_l", f"l_{bad!r}", lambda bad=bad: soft.extract_soft_l(z(), KEY, NONCE, 32, bad))
case("soft.extract_soft_l", "two_l_message", lambda: soft.extract_soft_l(z(), KEY, NONCE, 12, 3))


# ---- trace: the keyed registry -------------------------------------------------------------------------------------------------------------------------------------
def keyed_trace_rows(entry, call, table, tamper):
    """call(latents, registry, **kw)"""
    case(entry, "host", lambda: call(z(), registry()), "host")
    case(entry, "host_table", lambda: call(z(), registry(), thresholds=table()), "host")
    case(entry, "ok", lambda: call(z(), registry()))
    case(entry, "ok_table_k", lambda: call(z(), registry(), thresholds=table(), k=3, fpr=1.0))
    case(entry, "ok_table_f64", lambda: call(z(), registry(), thresholds=table().double()))
    for f in (0.0, 1.5, -1e-6):
        case(entry, f"fpr_{f}", lambda f=f: call(z(), registry(), fpr=f))
    case(entry, "lattice_ragged", lambda: call(z(shape=(4, 3, 3)), registry()))
    case(entry, "lattice_odd_bytes", lambda: call(z(shape=(4, 3, 4)), registry()))
    for lv in (0, 16, True):
        case(entry, f"levels_{lv!r}", lambda lv=lv: call(z(), registry(), levels=lv))
    case(entry, "clip_0", lambda: call(z(), registry(), clip=0))
    case(entry, "registry_empty", lambda: call(z(), registry(0)))
    case(entry, "table_levels_16", lambda: call(z(), registry(), thresholds=table(16)))
    case(entry, "table_images", lambda: call(z(), registry(), thresholds=torch.stack([table()] * 3)))
    case(entry, "two_fpr_lattice", lambda: call(z(shape=(4, 3, 3)), registry(), fpr=0.0))
    case(entry, "two_lattice_levels", lambda: call(z(shape=(4, 3, 3)), registry(), levels=0))
    case(entry, "two_levels_registry", lambda: call(z(), registry(0), levels=0))
    case(entry, "two_fpr_host", lambda: call(z(), registry(), fpr=0.0), "host")
    if tamper:
        case(entry, "ok_tamper_tile", lambda: call(z(), registry(), tamper_tile=8))


keyed_trace_rows("trace.trace_latents_keyed_soft", trace.trace_latents_keyed_soft, lambda levels=3: thr(levels), True)
for L in (2, 4):
    keyed_trace_rows(f"trace.trace_latents_keyed_soft_l/{L}", lambda a, b, L=L, **kw: trace.trace_latents_keyed_soft_l(a, b, L, **kw),
                     lambda levels=3, L=L: thr(L, levels), False)
for bad in (1, 3, True):
    case("trace.trace_latents_keyed_soft_l", f"l_{bad!r}", lambda bad=bad: trace.trace_latents_keyed_soft_l(z(), registry(), bad))
case("trace.trace_latents_keyed_soft_l", "two_l_fpr", lambda: trace.trace_latents_keyed_soft_l(z(), registry(), 1, fpr=0.0))
case("trace.trace_latents_keyed_soft_l", "two_l3_fpr", lambda: trace.trace_latents_keyed_soft_l(z(), registry(), 3, fpr=0.0))


# ---- detect: the keyring -----------------------------------------------------------------------------------------------------------------------------------------
def detect_rows(entry, call, aligned, window=1):
    """call(latents, keyring, message_length, **kw) with the entry's own mode bound; the rows every detection shares"""
    case(entry, "host", lambda: call(z(), keyring(), 32), "host")
    case(entry, "ok", lambda: call(z(), keyring(), 32))
    case(entry, "ok_k_fpr", lambda: call(z(), keyring(), 32, k=8, fpr=1.0))
    for f in (0.0, 2.0):
        case(entry, f"fpr_{f}", lambda f=f: call(z(), keyring(), 32, fpr=f))
    for m in (0, 12, 2056):
        case(entry, f"message_length_{m}", lambda m=m: call(z(), keyring(), m))
    for k in (0, 9):
        case(entry, f"k_{k}", lambda k=k: call(z(), keyring(), 32, k=k))
    case(entry, "keyring_empty", lambda: call(z(), keyring(0), 32))
    case(entry, "lattice_ragged", lambda: call(z(shape=(4, 3, 3)), keyring(), 32))
    case(entry, "two_fpr_message", lambda: call(z(), keyring(), 12, fpr=0.0))
    case(entry, "two_message_k", lambda: call(z(), keyring(), 12, k=0))
    case(entry, "two_k_keyring", lambda: call(z(), keyring(0), 32, k=0))
    case(entry, "two_keyring_lattice", lambda: call(z(shape=(4, 3, 3)), keyring(0), 32))
    case(entry, "two_k_host", lambda: call(z(), keyring(), 32, k=9), "host")
    if aligned:
        case(entry, "latents_3d", lambda: call(z(shape=(16, 16)), keyring(), 32))
        case(entry, "two_keyring_3d", lambda: call(z(shape=(16, 16)), keyring(0), 32))
        case(entry, "two_3d_lattice", lambda: call(z(shape=(12, 3)), keyring(), 32))


detect_rows("detect.detect_latents", detect.detect_latents, False)
for L in (2, 4):
    detect_rows(f"detect.detect_latents/l{L}", lambda *a, L=L, **kw: detect.detect_latents(*a, l=L, **kw), False)
detect_rows("detect.detect_latents/reliability", lambda *a, **kw: detect.detect_latents(*a, reliability=15, **kw), False)
detect_rows("detect.detect_latents/align", lambda *a, **kw: detect.detect_latents(*a, align=FLIPS, **kw), True)
detect_rows("detect.detect_latents/align_l2", lambda *a, **kw: detect.detect_latents(*a, align=FLIPS, l=2, **kw), True)
for L in (2, 4):
    detect_rows(f"detect.detect_latents_soft_l/{L}", lambda *a, L=L, **kw: detect.detect_latents_soft_l(*a, L, **kw), False)
detect_rows("detect.detect_latents_aligned_soft", lambda *a, **kw: detect.detect_latents_aligned_soft(*a, FLIPS, **kw), True)
for r in (-1, 16, True, 1.5, None):
    case("detect.detect_latents", f"reliability_{r!r}", lambda r=r: detect.detect_latents(z(), keyring(), 32, reliability=r))
case("detect.detect_latents", "reliability_align", lambda: detect.detect_latents(z(), keyring(), 32, reliability=3, align=FLIPS))
case("detect.detect_latents", "reliability_l2", lambda: detect.detect_latents(z(), keyring(), 32, reliability=3, l=2))
case("detect.detect_latents", "l_3", lambda: detect.detect_latents(z(), keyring(), 32, l=3))
case("detect.detect_latents", "align_empty", lambda: detect.detect_latents(z(), keyring(), 32, align=[]))
case("detect.detect_latents", "align_bad_entry", lambda: detect.detect_latents(z(), keyring(), 32, align=[(0, 0, 0), (9, 0, 0)]))
case("detect.detect_latents", "align_l_3", lambda: detect.detect_latents(z(), keyring(), 32, align=FLIPS, l=3))
case("detect.detect_latents", "two_reliability_align_fpr", lambda: detect.detect_latents(z(), keyring(), 32, reliability=3, align=FLIPS, fpr=0.0))
case("detect.detect_latents", "two_bad_reliability_align", lambda: detect.detect_latents(z(), keyring(), 32, reliability=16, align=FLIPS))
case("detect.detect_latents", "two_reliability_message_l2", lambda: detect.detect_latents(z(), keyring(), 12, reliability=3, l=2))
case("detect.detect_latents", "two_reliability_l2_k", lambda: detect.detect_latents(z(), keyring(), 32, reliability=3, l=2, k=0))
case("detect.detect_latents", "two_align_k_empty", lambda: detect.detect_latents(z(), keyring(), 32, align=[], k=0))
case("detect.detect_latents", "two_align_3d_empty", lambda: detect.detect_latents(z(shape=(16, 16)), keyring(), 32, align=[]))
case("detect.detect_latents", "two_align_empty_lattice", lambda: detect.detect_latents(z(shape=(4, 3, 3)), keyring(), 32, align=[]))
for bad in (1, 3, True):
    case("detect.detect_latents_soft_l", f"l_{bad!r}", lambda bad=bad: detect.detect_latents_soft_l(z(), keyring(), 32, bad))
for lv in (0, 16, True, None):
    case("detect.detect_latents_soft_l", f"levels_{lv!r}", lambda lv=lv: detect.detect_latents_soft_l(z(), keyring(), 32, 2, levels=lv))
    case("detect.detect_latents_aligned_soft", f"levels_{lv!r}", lambda lv=lv: detect.detect_latents_aligned_soft(z(), keyring(), 32, FLIPS, levels=lv))
case("detect.detect_latents_soft_l", "two_message_l", lambda: detect.detect_latents_soft_l(z(), keyring(), 12, 1))
case("detect.detect_latents_soft_l", "two_l_levels", lambda: detect.detect_latents_soft_l(z(), keyring(), 32, 1, levels=0))
case("detect.detect_latents_soft_l", "two_levels_k", lambda: detect.detect_latents_soft_l(z(), keyring(), 32, 2, levels=0, k=0))
case("detect.detect_latents_aligned_soft", "aligns_empty", lambda: detect.detect_latents_aligned_soft(z(), keyring(), 32, []))
case("detect.detect_latents_aligned_soft", "aligns_bad_entry", lambda: detect.detect_latents_aligned_soft(z(), keyring(), 32, [(0, 5, 0)]))
case("detect.detect_latents_aligned_soft", "two_message_levels", lambda: detect.detect_latents_aligned_soft(z(), keyring(), 12, FLIPS, levels=0))
case("detect.detect_latents_aligned_soft", "two_levels_k", lambda: detect.detect_latents_aligned_soft(z(), keyring(), 32, FLIPS, levels=0, k=0))
case("detect.detect_latents_aligned_soft", "two_empty_lattice", lambda: detect.detect_latents_aligned_soft(z(shape=(4, 3, 3)), keyring(), 32, []))


# ---- align: the searches and the known-key reader ------------------------------------------------------------------------------------------------------------------
def keys():
    return torch.zeros((5, codec.KEYED_RECORD_HEAD), dtype=torch.uint8)


for entry, call in (("align.search_keys", align.search_keys), ("align.search_keys_soft", align.search_keys_soft)):
    case(entry, "host", lambda call=call: call(z(), keys(), MB, FLIPS), "host")
    case(entry, "ok", lambda call=call: call(z(), keys(), MB, FLIPS))
    case(entry, "latents_3d", lambda call=call: call(z(shape=(16, 16)), keys(), MB, FLIPS))
    case(entry, "aligns_empty", lambda call=call: call(z(), keys(), MB, []))
    case(entry, "aligns_bad_entry", lambda call=call: call(z(), keys(), MB, [(0, 0, 0), (8, 0, 0)]))
    case(entry, "aligns_quarter_turn", lambda call=call: call(z(shape=(4, 8, 16)), keys(), MB, [(1, 0, 0)]))
    case(entry, "two_3d_empty", lambda call=call: call(z(shape=(16, 16)), keys(), MB, []))
    case(entry, "two_empty_host", lambda call=call: call(z(), keys(), MB, []), "host")
for bad in (3, True):
    case("align.search_keys", f"l_{bad!r}", lambda bad=bad: align.search_keys(z(), keys(), MB, FLIPS, l=bad))
case("align.search_keys", "ok_l2", lambda: align.search_keys(z(), keys(), MB, FLIPS, l=2))
case("align.search_keys", "two_l_empty", lambda: align.search_keys(z(), keys(), MB, [], l=3))
for lv in (0, 16, True):
    case("align.search_keys_soft", f"levels_{lv!r}", lambda lv=lv: align.search_keys_soft(z(), keys(), MB, FLIPS, levels=lv))
case("align.search_keys_soft", "ok_table", lambda: align.search_keys_soft(z(), keys(), MB, FLIPS, thresholds=thr(2, 7)))
case("align.search_keys_soft", "table_images", lambda: align.search_keys_soft(z(), keys(), MB, FLIPS, thresholds=thr(3, 7)))
case("align.search_keys_soft", "table_levels_16", lambda: align.search_keys_soft(z(), keys(), MB, FLIPS, thresholds=thr(16)))
case("align.search_keys_soft", "two_empty_levels", lambda: align.search_keys_soft(z(), keys(), MB, [], levels=0))

E = "align.extract_aligned_soft"
case(E, "host", lambda: align.extract_aligned_soft(z(), KEY, NONCE, 32, FLIPS), "host")
case(E, "ok", lambda: align.extract_aligned_soft(z(), KEY, NONCE, 32, FLIPS))
case(E, "ok_3_levels", lambda: align.extract_aligned_soft(z(), KEY, NONCE, 32, FLIPS, levels=3, fpr=1.0))
case(E, "key_short", lambda: align.extract_aligned_soft(z(), KEY[:16], NONCE, 32, FLIPS))
case(E, "nonce_short", lambda: align.extract_aligned_soft(z(), KEY, NONCE[:12], 32, FLIPS))
case(E, "fpr_0", lambda: align.extract_aligned_soft(z(), KEY, NONCE, 32, FLIPS, fpr=0.0))
case(E, "message_length_12", lambda: align.extract_aligned_soft(z(), KEY, NONCE, 12, FLIPS))
case(E, "levels_0", lambda: align.extract_aligned_soft(z(), KEY, NONCE, 32, FLIPS, levels=0))
case(E, "levels_16", lambda: align.extract_aligned_soft(z(), KEY, NONCE, 32, FLIPS, levels=16))
case(E, "latents_3d", lambda: align.extract_aligned_soft(z(shape=(16, 16)), KEY, NONCE, 32, FLIPS))
case(E, "aligns_empty", lambda: align.extract_aligned_soft(z(), KEY, NONCE, 32, []))
case(E, "lattice_ragged", lambda: align.extract_aligned_soft(z(shape=(4, 3, 3)), KEY, NONCE, 32, [(0, 0, 0)]))
case(E, "two_key_fpr", lambda: align.extract_aligned_soft(z(), KEY[:16], NONCE, 32, FLIPS, fpr=0.0))
case(E, "two_fpr_message", lambda: align.extract_aligned_soft(z(), KEY, NONCE, 12, FLIPS, fpr=0.0))
case(E, "two_levels_3d", lambda: align.extract_aligned_soft(z(shape=(16, 16)), KEY, NONCE, 32, FLIPS, levels=0))
case(E, "two_3d_empty", lambda: align.extract_aligned_soft(z(shape=(16, 16)), KEY, NONCE, 32, []))
case(E, "two_key_host", lambda: align.extract_aligned_soft(z(), KEY[:16], NONCE, 32, FLIPS), "host")

assert len({c[:2] for c in CASES}) == len(CASES), "every (entry, tag) names one row"


def outcome(thunk, where) -> tuple:
    """(exception type name, message) of one Python row; ("returned", "") for a call that came back"""
    with no_library(where == "device"):
        try:
            thunk()
        except Exception as e:                      # noqa: BLE001 -- the row records whatever is raised
            return type(e).__name__, " ".join(str(e).split())
    return "returned", ""


# ---- the C entry points --------------------------------------------------------------------------------------------------------------------------------------------
P, ODD = 0x10000, 0x10004                   # made-up pointers: 16-byte aligned, and 4 bytes past that.  Never read: every row below is refused first
VOTE = dict(z=P, dtype=N.GSW_F32, records=P, stride=64, msg_bytes=MB, thr=P, thr_stride=0, levels=3, bits=P, score=P, wsum=P, wsq=P, flags=P, matches=P, B=2, n=256)
PACK = dict(z=P, dtype=N.GSW_F32, thr=P, thr_stride=0, levels=3, signs=P, planes=P, wsum=P, wsq=P, flags=P, B=2, n=256)
POINTERS = {"z", "records", "thr", "bits", "score", "wsum", "wsq", "flags", "matches", "signs", "planes"}
REQUIRED = {True: ("z", "records", "thr", "bits", "flags"), False: ("z", "thr", "signs", "planes", "wsum", "wsq", "flags")}
C_CASES = []                                # (symbol, tag, only without a device, the arguments in the order of include/gswm.h)


def c_case(symbol, tag, l, **kw):
    vote = "extract" in symbol
    args = dict(VOTE if vote else PACK)
    assert not set(kw) - set(args), set(kw) - set(args)
    args.update(kw)
    made_up = all(args[k] for k in REQUIRED[vote])            # no null pointer: only the value checks stand between the row and a launch
    out = []
    for name, v in args.items():
        out.append((v or None) if name in POINTERS else v)
        if name == "levels" and l is not None:
            out.append(l)
    C_CASES.append((symbol, tag, made_up, tuple(out) + (None,)))


def c_rows(symbol, l):
    vote, w = "extract" in symbol, (l or 1)
    at = "" if l is None else f"@l{l}"
    limit = codec.ROW_MAX_BITS // w
    for name in REQUIRED[vote]:
        c_case(symbol, f"null_{name}{at}", l, **{name: 0})
    c_case(symbol, f"null_all{at}", l, **{k: 0 for k in POINTERS if k in (VOTE if vote else PACK)})
    c_case(symbol, f"null_z_ragged{at}", l, z=0, n=12)
    c_case(symbol, f"null_z_past_limit{at}", l, z=0, n=limit + 8)
    c_case(symbol, f"null_thr_levels_16{at}", l, thr=0, levels=16)
    rows = [("B_0", dict(B=0)), ("n_0", dict(n=0)), ("n_negative", dict(n=-8)), ("dtype_low", dict(dtype=N.GSW_F32 - 1)), ("dtype_high", dict(dtype=N.GSW_F64 + 1)),
            ("z_odd", dict(z=ODD)), ("thr_odd", dict(thr=P + 2)), ("levels_0", dict(levels=0)), ("levels_16", dict(levels=16)),
            ("thr_stride_short", dict(thr_stride=w * 3 - 1)), ("thr_stride_negative", dict(thr_stride=-1)),
            ("n_ragged", dict(n=12)), ("n_past_limit", dict(n=limit + 8)), ("n_far_past_limit", dict(n=2 ** 40)),
            ("two_dtype_ragged", dict(dtype=9, n=12)), ("two_levels_past_limit", dict(levels=0, n=limit + 8)), ("two_stride_ragged", dict(thr_stride=1, n=12)),
            ("two_z_odd_ragged", dict(z=ODD, n=12))]
    if vote:
        rows += [("msg_bytes_0", dict(msg_bytes=0)), ("msg_bytes_257", dict(msg_bytes=257, stride=320)), ("stride_short", dict(stride=48)), ("stride_odd", dict(stride=72)),
                 ("stride_huge", dict(stride=2 ** 31)), ("records_odd", dict(records=ODD)),
                 ("message_ragged", dict(n=8, msg_bytes=5)), ("message_ragged_256", dict(msg_bytes=256, stride=304, n=limit - 8)), ("msg_bytes_1_past_limit", dict(msg_bytes=1, n=limit + 8)),
                 ("two_records_levels", dict(stride=48, levels=0)), ("two_records_ragged", dict(msg_bytes=0, n=12)), ("two_ragged_message", dict(n=12, msg_bytes=3)),
                 ("two_past_limit_message", dict(n=limit + 8, msg_bytes=5)), ("two_bits_ragged", dict(bits=0, n=12)), ("two_flags_message", dict(flags=0, n=8, msg_bytes=5))]
    for tag, kw in rows:
        c_case(symbol, tag + at, l, **kw)
    if l == 2:
        for bad in (0, 1, 3, 8, -2):
            c_case(symbol, f"l_{bad}", bad)
            c_case(symbol, f"two_l_{bad}_ragged", bad, n=12)
            c_case(symbol, f"null_z_l_{bad}", bad, z=0)


c_rows("gsw_extract_soft", None)
c_rows("gsw_level_pack", None)
for L in (2, 4):
    c_rows("gsw_extract_soft_l", L)
    c_rows("gsw_level_pack_l", L)
assert len({c[:2] for c in C_CASES}) == len(C_CASES), "every (symbol, tag) names one row"


def c_outcome(symbol, args) -> int:
    return int(getattr(N.lib(), symbol)(*args))
