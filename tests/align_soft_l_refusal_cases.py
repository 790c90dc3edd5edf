"""The refusal table of the reliability levels of multi-bit windows through the alignment searches: one call per row, shared by
tools/gen_align_soft_l_refusals.py, which records what every call raises into tests/golden/align_soft_l_refusals.tsv, and by tests/test_align_soft_l_host.py, which
replays the calls and compares.  The ORDER in which bad arguments are refused is behaviour: a row with two faults pins which one wins.

The rows are replayed as tests/level_refusal_cases.py replays its own (`no_library`, `outcome`, `c_outcome`: `host` rows on plain host tensors, `device` rows
while every tensor claims to live on the device and the library is replaced by one that raises `Reached(<symbol>)`).  The C rows carry at least one fault each, so
a correct library returns before it touches a pointer; rows with made-up pointers are replayed only where there is no device."""
import torch

import level_refusal_cases as L
from gswm_amd import align, codec, detect, trace
from level_refusal_cases import FLIPS, KEY, MB, NONCE, keyring, keys, registry, thr, z

CASES = []                                  # (entry, tag, "host" | "device", thunk)
C_CASES = []                                # (symbol, tag, made-up pointers, arguments in the order of include/gswm.h)


def case(entry, tag, thunk, where="device"):
    CASES.append((entry, tag, where, thunk))


def rows(B=2, shape=(4, 8, 8), l=2, P=2, **replace):
    """host `codec.LevelRows` of zeros for a lattice at l"""
    nb = shape[0] * shape[1] * shape[2] * l // 8
    i32 = lambda: torch.zeros(B, dtype=torch.int32)
    r = codec.LevelRows(torch.zeros((B, nb), dtype=torch.uint8), torch.zeros((B, P, nb), dtype=torch.uint8), i32(), i32(), i32())
    return r._replace(**replace)


def shared_registry(n=6, mb=MB):
    reg = trace.Registry(mb)
    for i in range(n):
        reg.add(f"user{i}", bytes([i + 1]) * mb)
    return reg


S = (4, 8, 8)
# ---- codec: the two launches ---------------------------------------------------------------------------------------------------------------------------------------
for entry, call in (("codec.level_rows_align_l", lambda r, shape, l, aligns, **kw: codec.level_rows_align_l(r, shape, l, aligns)),
                    ("codec.level_counts_align_l", lambda r, shape, l, aligns, M=32, **kw: codec.level_counts_align_l(r, shape, l, aligns, KEY, NONCE, M, **kw))):
    for l in (2, 4):
        case(entry, f"host/{l}", lambda call=call, l=l: call(rows(l=l), S, l, FLIPS), "host")
        case(entry, f"ok/{l}", lambda call=call, l=l: call(rows(l=l), S, l, FLIPS))
        case(entry, f"ok_device_table/{l}", lambda call=call, l=l: call(rows(l=l), S, l, torch.tensor(FLIPS, dtype=torch.int32)))
    for bad in (1, 3, True, 2.0, None):
        case(entry, f"l_{bad!r}", lambda call=call, bad=bad: call(rows(), S, bad, FLIPS))
    case(entry, "shape_2d", lambda call=call: call(rows(), (8, 8), 2, FLIPS))
    case(entry, "shape_zero", lambda call=call: call(rows(), (4, 0, 8), 2, FLIPS))
    case(entry, "lattice_ragged", lambda call=call: call(rows(shape=(1, 1, 8))._replace(signs=torch.zeros((2, 1), dtype=torch.uint8)), (1, 1, 3), 2, [(0, 0, 0)]))
    case(entry, "rows_of_l1", lambda call=call: call(rows(l=1), S, 2, FLIPS))                       # `level_pack`'s rows: half as long as the window's
    case(entry, "rows_of_l4", lambda call=call: call(rows(l=4), S, 2, FLIPS))
    case(entry, "signs_dtype", lambda call=call: call(rows(signs=torch.zeros((2, 64), dtype=torch.int8)), S, 2, FLIPS))
    case(entry, "planes_images", lambda call=call: call(rows(planes=torch.zeros((3, 2, 64), dtype=torch.uint8)), S, 2, FLIPS))
    case(entry, "planes_5", lambda call=call: call(rows(P=5), S, 2, FLIPS))
    case(entry, "wsum_dtype", lambda call=call: call(rows(wsum=torch.zeros(2, dtype=torch.int64)), S, 2, FLIPS))
    case(entry, "flags_shape", lambda call=call: call(rows(flags=torch.zeros(3, dtype=torch.int32)), S, 2, FLIPS))
    case(entry, "past_domain", lambda call=call: call(rows(B=1, shape=(4, 128, 128), l=4, P=4), (4, 128, 128), 4, [(0, 0, 0)], M=256))   # n l (1 + P) = 5 x 2^18
    case(entry, "aligns_empty", lambda call=call: call(rows(), S, 2, []))
    case(entry, "aligns_bad_entry", lambda call=call: call(rows(), S, 2, [(0, 0, 0), (8, 0, 0)]))
    case(entry, "aligns_quarter_turn", lambda call=call: call(rows(shape=(4, 8, 16)), (4, 8, 16), 2, [(1, 0, 0)]))
    case(entry, "aligns_dtype", lambda call=call: call(rows(), S, 2, torch.zeros((3, 3), dtype=torch.int64)))
    case(entry, "two_l_shape", lambda call=call: call(rows(), (8, 8), 1, FLIPS))
    case(entry, "two_shape_aligns", lambda call=call: call(rows(), (8, 8), 2, []))
    case(entry, "two_rows_aligns", lambda call=call: call(rows(l=1), S, 2, []))
    case(entry, "two_l_host", lambda call=call: call(rows(), S, 1, FLIPS), "host")
E = "codec.level_counts_align_l"
cnt = codec.level_counts_align_l
for m in (0, 12, 2056, True):
    case(E, f"msg_bits_{m!r}", lambda m=m: cnt(rows(), S, 2, FLIPS, KEY, NONCE, m))
case(E, "msg_bits_untiled", lambda: cnt(rows(), S, 2, FLIPS, KEY, NONCE, 24))
case(E, "key_short", lambda: cnt(rows(), S, 2, FLIPS, KEY[:31], NONCE, 32))
case(E, "bias_float", lambda: cnt(rows(), S, 2, FLIPS, KEY, NONCE, 32, bias=1.5))
case(E, "bias_past_int32", lambda: cnt(rows(), S, 2, FLIPS, KEY, NONCE, 32, bias=2 ** 31 - 15 * 16))
case(E, "ok_bias_wsum", lambda: cnt(rows(), S, 2, FLIPS, KEY, NONCE, 32, bias=15 * 16, return_wsum=True))
case(E, "past_lds_cap", lambda: cnt(rows(B=1, shape=(4, 128, 132), l=4, P=1), (4, 128, 132), 4, [(0, 0, 0)], KEY, NONCE, 256))
case(E, "two_key_l", lambda: cnt(rows(), S, 1, FLIPS, KEY[:31], NONCE, 32))
case(E, "two_l_msg_bits", lambda: cnt(rows(), S, 3, FLIPS, KEY, NONCE, 12))
case(E, "two_msg_bits_bias", lambda: cnt(rows(), S, 2, FLIPS, KEY, NONCE, 12, bias=1.5))
case(E, "two_bias_aligns", lambda: cnt(rows(), S, 2, [], KEY, NONCE, 32, bias=1.5))


# ---- the searches --------------------------------------------------------------------------------------------------------------------------------------------------
def search_rows(entry, call, table):
    """call(latents, aligns, l, **kw) with the entry's other operands bound; the rows every search shares"""
    for l in (2, 4):
        case(entry, f"host/{l}", lambda l=l: call(z(), FLIPS, l), "host")
        case(entry, f"ok/{l}", lambda l=l: call(z(), FLIPS, l))
        case(entry, f"ok_table/{l}", lambda l=l: call(z(), FLIPS, l, thresholds=table(l)))
    for bad in (1, 3, True):
        case(entry, f"l_{bad!r}", lambda bad=bad: call(z(), FLIPS, bad))
    for lv in (0, 16, True):
        case(entry, f"levels_{lv!r}", lambda lv=lv: call(z(), FLIPS, 2, levels=lv))
    case(entry, "latents_3d", lambda: call(z(shape=(16, 16)), FLIPS, 2))
    case(entry, "aligns_empty", lambda: call(z(), [], 2))
    case(entry, "aligns_bad_entry", lambda: call(z(), [(0, 0, 0), (8, 0, 0)], 2))
    case(entry, "aligns_quarter_turn", lambda: call(z(shape=(4, 8, 16)), [(1, 0, 0)], 2))
    case(entry, "lattice_ragged", lambda: call(z(shape=(4, 3, 3)), [(0, 0, 0)], 2))
    case(entry, "table_window", lambda: call(z(), FLIPS, 2, thresholds=table(4)))
    case(entry, "table_flat", lambda: call(z(), FLIPS, 4, thresholds=thr(7)))
    case(entry, "table_levels_16", lambda: call(z(), FLIPS, 2, thresholds=thr(2, 16)))
    case(entry, "two_l_3d", lambda: call(z(shape=(16, 16)), FLIPS, 1))
    case(entry, "two_3d_empty", lambda: call(z(shape=(16, 16)), [], 2))
    case(entry, "two_empty_levels", lambda: call(z(), [], 2, levels=0))
    case(entry, "two_l_host", lambda: call(z(), FLIPS, 3), "host")


search_rows("align.search_keys_soft_l", lambda zz, al, l, **kw: align.search_keys_soft_l(zz, keys(), MB, al, l, **kw), lambda l, levels=7: thr(l, levels))
search_rows("trace.trace_latents_aligned_soft_l", lambda zz, al, l, **kw: trace.trace_latents_aligned_soft_l(zz, KEY, NONCE, shared_registry(), al, l, **kw),
            lambda l, levels=7: thr(l, levels))
search_rows("trace.trace_latents_keyed_aligned_soft_l", lambda zz, al, l, **kw: trace.trace_latents_keyed_aligned_soft_l(zz, registry(), al, l, **kw),
            lambda l, levels=7: thr(l, levels))
for entry, call in (("trace.trace_latents_aligned_soft_l", lambda **kw: trace.trace_latents_aligned_soft_l(z(), KEY, NONCE, shared_registry(), FLIPS, 2, **kw)),
                    ("trace.trace_latents_keyed_aligned_soft_l", lambda **kw: trace.trace_latents_keyed_aligned_soft_l(z(), registry(), FLIPS, 2, **kw))):
    for f in (0.0, 1.5):
        case(entry, f"fpr_{f}", lambda call=call, f=f: call(fpr=f))
    case(entry, "clip_0", lambda call=call: call(clip=0))
    case(entry, "k_9", lambda call=call: call(k=9))
    case(entry, "ok_tamper_tile", lambda call=call: call(tamper_tile=8))
    case(entry, "two_fpr_levels", lambda call=call: call(fpr=0.0, levels=0))
case("trace.trace_latents_aligned_soft_l", "key_short", lambda: trace.trace_latents_aligned_soft_l(z(), KEY[:31], NONCE, shared_registry(), FLIPS, 2))
case("trace.trace_latents_aligned_soft_l", "message_length_untiled", lambda: trace.trace_latents_aligned_soft_l(z(), KEY, NONCE, shared_registry(mb=3), FLIPS, 2))
case("trace.trace_latents_aligned_soft_l", "two_l_key", lambda: trace.trace_latents_aligned_soft_l(z(), KEY[:31], NONCE, shared_registry(), FLIPS, 1))
case("trace.trace_latents_keyed_aligned_soft_l", "registry_empty", lambda: trace.trace_latents_keyed_aligned_soft_l(z(), registry(0), FLIPS, 2))

D = "detect.detect_latents_aligned_soft_l"
det = lambda zz=None, ring=None, m=32, al=FLIPS, l=2, **kw: detect.detect_latents_aligned_soft_l(z() if zz is None else zz, keyring() if ring is None else ring, m, al, l, **kw)
for l in (2, 4):
    case(D, f"host/{l}", lambda l=l: det(l=l), "host")
    case(D, f"ok/{l}", lambda l=l: det(l=l))
case(D, "ok_k_fpr", lambda: det(k=8, fpr=1.0, levels=3))
for bad in (1, 3, True):
    case(D, f"l_{bad!r}", lambda bad=bad: det(l=bad))
for lv in (0, 16, True, None):
    case(D, f"levels_{lv!r}", lambda lv=lv: det(levels=lv))
for f in (0.0, 2.0):
    case(D, f"fpr_{f}", lambda f=f: det(fpr=f))
for m in (0, 12, 2056):
    case(D, f"message_length_{m}", lambda m=m: det(m=m))
for k in (0, 9):
    case(D, f"k_{k}", lambda k=k: det(k=k))
case(D, "keyring_empty", lambda: det(ring=keyring(0)))
case(D, "latents_3d", lambda: det(zz=z(shape=(16, 16))))
case(D, "aligns_empty", lambda: det(al=[]))
case(D, "aligns_bad_entry", lambda: det(al=[(0, 5, 0), (9, 0, 0)]))
case(D, "lattice_ragged", lambda: det(zz=z(shape=(4, 3, 3)), al=[(0, 0, 0)]))
case(D, "two_l_fpr", lambda: det(l=1, fpr=0.0))
case(D, "two_fpr_message", lambda: det(m=12, fpr=0.0))
case(D, "two_message_levels", lambda: det(m=12, levels=0))
case(D, "two_levels_k", lambda: det(levels=0, k=0))
case(D, "two_keyring_3d", lambda: det(zz=z(shape=(16, 16)), ring=keyring(0)))
case(D, "two_l_host", lambda: det(l=3), "host")

X = "align.extract_aligned_soft_l"
ext = lambda zz=None, key=KEY, nonce=NONCE, m=32, al=FLIPS, l=2, **kw: align.extract_aligned_soft_l(z() if zz is None else zz, key, nonce, m, al, l, **kw)
for l in (2, 4):
    case(X, f"host/{l}", lambda l=l: ext(l=l), "host")
    case(X, f"ok/{l}", lambda l=l: ext(l=l))
for bad in (1, 3, True):
    case(X, f"l_{bad!r}", lambda bad=bad: ext(l=bad))
case(X, "key_short", lambda: ext(key=KEY[:16]))
case(X, "nonce_short", lambda: ext(nonce=NONCE[:12]))
case(X, "fpr_0", lambda: ext(fpr=0.0))
case(X, "message_length_12", lambda: ext(m=12))
case(X, "levels_0", lambda: ext(levels=0))
case(X, "levels_16", lambda: ext(levels=16))
case(X, "latents_3d", lambda: ext(zz=z(shape=(16, 16))))
case(X, "aligns_empty", lambda: ext(al=[]))
case(X, "aligns_bad_entry", lambda: ext(al=[(0, 0, 0), (8, 0, 0)]))
case(X, "lattice_ragged", lambda: ext(zz=z(shape=(4, 3, 3)), al=[(0, 0, 0)]))
case(X, "two_key_l", lambda: ext(key=KEY[:16], l=1))
case(X, "two_l_fpr", lambda: ext(l=3, fpr=0.0))
case(X, "two_levels_3d", lambda: ext(zz=z(shape=(16, 16)), levels=0))
case(X, "two_key_host", lambda: ext(key=KEY[:16]), "host")

assert len({c[:2] for c in CASES}) == len(CASES), "every (entry, tag) names one row"
outcome = L.outcome


# ---- the C entry points --------------------------------------------------------------------------------------------------------------------------------------------
P, ODD = L.P, 0x10002                       # made-up pointers: 16-byte aligned, and 2 bytes past that.  Never read: every row below is refused first
ROWS_ARGS = dict(signs=P, planes=P, P=2, l=2, B=2, C=4, H=8, W=8, aligns=P, A=3, out_signs=P, out_planes=P)
COUNTS_ARGS = dict(signs=P, planes=P, P=2, l=2, B=2, C=4, H=8, W=8, aligns=P, A=3, key=KEY, nonce=NONCE, msg_bits=32, bias=0, score=P, wsum=P)
POINTERS = {"signs", "planes", "aligns", "out_signs", "out_planes", "score", "wsum", "key", "nonce"}


def c_case(symbol, tag, **kw):
    args = dict(ROWS_ARGS if symbol == "gsw_level_rows_align_l" else COUNTS_ARGS)
    assert not set(kw) - set(args), set(kw) - set(args)
    args.update(kw)
    made_up = all(args[k] for k in POINTERS if k in args and k != "wsum")
    C_CASES.append((symbol, tag, made_up, tuple((v or None) if k in POINTERS else v for k, v in args.items()) + (None,)))


for symbol in ("gsw_level_rows_align_l", "gsw_level_counts_align_l"):
    counts = symbol == "gsw_level_counts_align_l"
    for name in ("signs", "planes", "aligns") + (("key", "nonce", "score") if counts else ("out_signs", "out_planes")):
        c_case(symbol, f"null_{name}", **{name: 0})
    c_case(symbol, "null_signs_l_3", signs=0, l=3)
    c_case(symbol, "null_signs_ragged", signs=0, C=1, H=1, W=3)
    c_case(symbol, "null_signs_past_domain", signs=0, C=4, H=128, W=128, l=4, P=4, **(dict(msg_bits=256) if counts else {}))
    for bad in (0, 3, 8, -2):
        c_case(symbol, f"l_{bad}", l=bad)
    for tag, kw in (("P_0", dict(P=0)), ("P_5", dict(P=5)), ("B_0", dict(B=0)), ("C_0", dict(C=0)), ("H_negative", dict(H=-1)), ("W_0", dict(W=0)), ("A_0", dict(A=0)),
                    ("aligns_odd", dict(aligns=ODD)), ("ragged_l2", dict(C=1, H=1, W=3)), ("ragged_l4", dict(C=1, H=1, W=1, l=4)),
                    ("B_65536", dict(B=65536)), ("two_l_ragged", dict(l=3, C=1, H=1, W=3)), ("two_P_past_domain", dict(P=5, C=4, H=256, W=256)),
                    ("huge", dict(C=2147483646, H=2147483644, W=2147483640))):
        c_case(symbol, tag, **kw)
    c_case(symbol, "past_domain_l4", C=4, H=128, W=128, l=4, P=4, **(dict(msg_bits=256) if counts else {}))
    c_case(symbol, "past_domain_l2", C=4, H=128, W=256, l=2, P=4, **(dict(msg_bits=256) if counts else {}))
    if counts:
        for tag, kw in (("msg_bits_0", dict(msg_bits=0)), ("msg_bits_12", dict(msg_bits=12)), ("msg_bits_2056", dict(msg_bits=2056)), ("msg_bits_untiled", dict(msg_bits=24)),
                        ("score_odd", dict(score=ODD)), ("wsum_odd", dict(wsum=ODD)), ("bias_past_int32", dict(bias=2 ** 31 - 15 * 16)),
                        ("past_lds_cap", dict(C=4, H=128, W=132, l=4, P=1, msg_bits=256)), ("two_msg_bits_ragged", dict(msg_bits=12, C=1, H=1, W=3)),
                        ("two_untiled_past_domain", dict(msg_bits=24, C=4, H=256, W=256, P=4))):
            c_case(symbol, tag, **kw)
assert len({c[:2] for c in C_CASES}) == len(C_CASES), "every (symbol, tag) names one row"
c_outcome = L.c_outcome
