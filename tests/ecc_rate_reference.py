"""NumPy restatement of the punctured payload codes: the rate-1/2, constraint-length-7 mother code of `ecc_reference` punctured to
rates 2/3 ("conv23") and 3/4 ("conv34"), its encoder, its maximum-correlation Viterbi decoder and its list decoder.  Integer arithmetic throughout: the device
(`codec.viterbi_decode(code=)`, `codec.viterbi_list_decode(code=)`) and the package's host encoder (`ecc.encode(code=)`) must equal it bit for bit.  Written
from the definition; the CRC, the labels, the interleaver step and the ok rule are imported from the two older restatements, nothing of their decoders is.

The definition.  Step t of the mother code emits (c0, c1), c0 of 0o171 and c1 of 0o133.  A code has a pattern of period P; step t keeps the outputs
PATTERN[code][t mod P], in that order.  N(t) is the number of kept bits of the first t steps.  T is the largest multiple of 8 with N(T) <= M, I = T - 6, the
info word has T / 8 bytes (payload, CRC-16, 2 pad bits, tail).  Kept bit j, in step order and then pattern order, sits at message position (j S) mod M for
j < N = N(T); the M - N spare positions carry 0 when encoded and are never read.  The decoder is section 4.29's (4.30's with a list) with one change: an
output that is not kept contributes nothing to a branch metric.  Here that is said literally: the votes are spread into two columns per step, 0 where an
output is punctured, and the trellis runs on those."""
import numpy as np

import ecc_list_reference as LR
import ecc_reference as R

CODES = ("conv", "conv23", "conv34")
PATTERN = {"conv": ((0, 1),), "conv23": ((0, 1), (1,)), "conv34": ((0, 1), (1,), (0,))}
EMPTY = LR.EMPTY


def kept_bits(code, steps):
    """N(t), in closed form as the issue states it"""
    if code == "conv":
        return 2 * steps
    if code == "conv23":
        return 3 * (steps // 2) + 2 * (steps % 2)
    return 4 * (steps // 3) + (0, 2, 3)[steps % 3]


def sizes(M, code):
    """-> (I info bits, T trellis steps, N kept bits, payload bytes); no upper limit on M (the list read's own bound is its LDS slice)"""
    assert code in CODES and M % 16 == 0 and M >= 64
    T = max(t for t in range(8, M + 1, 8) if kept_bits(code, t) <= M)
    return T - R.TAIL, T, kept_bits(code, T), T // 8 - 3


def capacity(M, code):
    return sizes(M, code)[3]


def layout(M, code, interleave=True):
    """-> (step [N], which [N], pos [N]): kept bit j is output `which` of step `step` and sits at message position `pos`"""
    _, T, N, _ = sizes(M, code)
    pat = PATTERN[code]
    pairs = [(t, w) for t in range(T) for w in pat[t % len(pat)]]
    assert len(pairs) == N
    j = np.arange(N, dtype=np.int64)
    return np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs]), (j * R.interleaver_step(M)) % M if interleave else j


def info_word(payload, M, code):
    I, _, _, pb = sizes(M, code)
    if len(payload) != pb:
        raise ValueError(f"a payload of {len(payload)} bytes; message_length {M} carries exactly {pb} under {code}")
    c = R.crc16(payload)
    bits = np.unpackbits(np.frombuffer(bytes(payload) + bytes([c >> 8, c & 0xFF]), dtype=np.uint8))
    return np.concatenate([bits, np.zeros(I - bits.size, dtype=np.uint8)])


def encode_bits(info, M, code, interleave=True):
    """uint8 [M] message bits of an info word of I bits: the mother code's 2 T bits (`ecc_reference.conv_encode`, the shift register), the kept ones placed"""
    mother = R.conv_encode(np.concatenate([np.asarray(info, dtype=np.uint8), np.zeros(R.TAIL, dtype=np.uint8)])).reshape(-1, 2)
    step, which, pos = layout(M, code, interleave)
    msg = np.zeros(M, dtype=np.uint8)
    msg[pos] = mother[step, which]
    return msg


def encode(payload, M, code, interleave=True):
    return np.packbits(encode_bits(info_word(payload, M, code), M, code, interleave)).tobytes()


def spread(score, code, interleave=True):
    """score int [B, M] -> int64 [B, 2 T]: column 2 t + w holds the vote of output w of step t, 0 where that output is punctured; no interleaver left"""
    score = np.asarray(score)
    B, M = score.shape
    step, which, pos = layout(M, code, interleave)
    row = np.zeros((B, 2 * sizes(M, code)[1]), dtype=np.int64)
    row[:, 2 * step + which] = score[:, pos]
    return row


def _trellis(x, T, I, L):
    """the list trellis of section 4.30 on two vote columns per step, x int64 [B, 2 T] -> (metrics int64 [B, L], inputs uint8 [B, L, T]) of the L paths
    through state 0, best first.  L = 1 is section 4.29's decoder: a state's single entry, the lower predecessor on equal metrics."""
    B = x.shape[0]
    s = np.arange(64)
    p0, u = 2 * (s & 31), s >> 5
    l0, l1 = R._labels()
    sg0, sg1 = 2 * l0 - 1, 2 * l1 - 1
    pm = np.full((B, 64, L), EMPTY, dtype=np.int64)
    pm[:, 0, 0] = 0
    dec = np.zeros((T, B, 64), dtype=np.int64)
    pad = np.full((B, 64, 1), EMPTY, dtype=np.int64)
    for t in range(T):
        bm = (sg0[None, :] * x[:, 2 * t, None] + sg1[None, :] * x[:, 2 * t + 1, None])[:, :, None]
        a, b = pm[:, p0, :], pm[:, p0 + 1, :]
        a = np.concatenate([np.where(a == EMPTY, EMPTY, a + bm), pad], axis=2)
        b = np.concatenate([np.where(b == EMPTY, EMPTY, b - bm), pad], axis=2)
        i = np.zeros((B, 64, 1), dtype=np.int64)
        j = np.zeros((B, 64, 1), dtype=np.int64)
        out = np.empty((B, 64, L), dtype=np.int64)
        bits = np.zeros((B, 64), dtype=np.int64)
        for k in range(L):
            ha, hb = np.take_along_axis(a, i, axis=2), np.take_along_axis(b, j, axis=2)
            tb = hb > ha                                            # strict: on equal metrics the d = 0 entry goes first
            out[:, :, k] = np.where(tb, hb, ha)[:, :, 0]
            bits |= tb[:, :, 0].astype(np.int64) << k
            i, j = i + ~tb, j + tb
        if t >= I:
            out[:, u != 0, :] = EMPTY
        pm, dec[t] = out, bits
    assert (pm[:, 0, :] != EMPTY).all()
    rows = np.arange(B)
    inputs = np.zeros((B, L, T), dtype=np.uint8)
    for r in range(L):
        st, k = np.zeros(B, dtype=np.int64), np.full(B, r, dtype=np.int64)
        for t in range(T - 1, -1, -1):
            rec = dec[t][rows, st]
            d = (rec >> k) & 1
            same1 = LR._POPCOUNT[rec & ((1 << k) - 1)]
            inputs[:, r, t] = st >> 5
            k = np.where(d == 1, same1, k - same1)
            st = 2 * (st & 31) + d
        assert (st == 0).all() and (k == 0).all()
    return pm[:, 0, :], inputs


def decode_list(score, L, code, interleave=True):
    """score int [B, M] -> info uint8 [B, T/8], message uint8 [B, M/8], metric, flips, ok, rank, n_ok int32 [B] of the selected path"""
    score = LR._check(score, L)
    B, M = score.shape
    I, T, N, pb = sizes(M, code)
    metrics, inputs = _trellis(spread(score, code, interleave), T, I, L)
    oks = np.array([[LR._ok(inputs[b, r], pb) for r in range(L)] for b in range(B)], dtype=bool)
    n_ok = oks.sum(axis=1).astype(np.int32)
    rank = np.where(n_ok > 0, oks.argmax(axis=1), 0).astype(np.int32)
    rows = np.arange(B)
    ub = inputs[rows, rank]
    step, which, pos = layout(M, code, interleave)
    msg = np.zeros((B, M), dtype=np.uint8)
    for b in range(B):
        msg[b, pos] = R.conv_encode(ub[b]).reshape(-1, 2)[step, which]       # re-encoded by the shift register, re-punctured, re-interleaved
    flips = (msg[:, pos] != (score[:, pos] > 0)).sum(axis=1).astype(np.int32)   # over the N code positions only
    return {"info": np.packbits(ub, axis=1), "message": np.packbits(msg, axis=1), "metric": metrics[rows, rank].astype(np.int32), "flips": flips,
            "ok": oks[rows, rank].astype(np.int32), "rank": rank, "n_ok": n_ok}


PLAIN = ("info", "message", "metric", "flips", "ok")
NAMES = LR.NAMES


def decode(score, code, interleave=True):
    """the plain read: the list read of one path, its five outputs"""
    d = decode_list(score, 1, code, interleave)
    return {k: d[k] for k in PLAIN}


def payloads(info, M, code):
    pb = capacity(M, code)
    return [np.asarray(info)[b, :pb].tobytes() for b in range(len(info))]


def plain_wave_lds(M, code):
    T = sizes(M, code)[1]
    return (4 * M + 8 * T + T + M + T // 8 + 15) // 16 * 16


def list_wave_lds(M, L, code):
    T = sizes(M, code)[1]
    return (4 * M + 256 * L + 9 * T * L + M + T // 8 + 15) // 16 * 16


def served(M, L, code):
    return code in CODES and L in LR.LIST_SIZES and M % 16 == 0 and M >= 64 and list_wave_lds(M, L, code) <= 160 * 1024


def largest_served(L, code):
    return max(M for M in range(64, 20000, 16) if served(M, L, code))


def format_read(d, b, M, code, L=1):
    """the text of `ecc.format_any`, restated from the issue: `corrected <flips> of <N>`"""
    pb, N = capacity(M, code), sizes(M, code)[2]
    text = f"payload {d['info'][b, :pb].tobytes().hex()} crc {'ok' if d['ok'][b] else 'FAILED'}, corrected {d['flips'][b]} of {N}"
    if L > 1:
        text += f", list rank {d['rank'][b]} of {L}" + (f", {d['n_ok'][b]} candidates pass" if d["n_ok"][b] > 1 else "")
    return text


# ------------------------------------------------------------------------------------------------ the sigma walk (tools/ecc_rate_sigma_walk.py, the end-to-end tests)
# `ecc_reference.WALK` and `walk_setup()` as they are (keys, uniforms, noise, blank latents); a payload draw of its own per code, since the codes carry
# different numbers of bytes.
PAYLOAD_SEED = {"conv": 2026043100, "conv23": 2026043123, "conv34": 2026043134}


def walk_payloads(code):
    rng = np.random.default_rng(PAYLOAD_SEED[code])
    return [rng.bytes(capacity(R.WALK["M"], code)) for _ in range(R.WALK["images"])]


def walk_scores(code, setup=None):
    """-> (setup, payloads, {sigma: score int32 [20, 256]}): the walk's images carrying this code's payloads, their votes at every grid point"""
    W = R.WALK
    setup = setup or R.walk_setup()
    pl = walk_payloads(code)
    z = R.walk_latents(setup, [encode(p, W["M"], code) for p in pl])
    return setup, pl, {s: R.walk_scores(setup, R.held(z, setup["noise"], s), W["M"])[0] for s in W["sigmas"]}


def count_reads(d, sent, M, code):
    """-> (right + ok, wrong + ok)"""
    got = payloads(d["info"], M, code)
    right = sum(1 for b, p in enumerate(sent) if d["ok"][b] and got[b] == p)
    return right, int(d["ok"].sum()) - right


def walk(code, setup=None):
    """-> {L: ([(sigma, right + ok, wrong + ok)], blank ok count)} for the four list sizes"""
    setup, pl, scores = walk_scores(code, setup)
    blank = LR.blank_scores(setup)
    M = R.WALK["M"]
    return {L: ([(s,) + count_reads(decode_list(scores[s], L, code), pl, M, code) for s in R.WALK["sigmas"]], int(decode_list(blank, L, code)["ok"].sum()))
            for L in LR.LIST_SIZES}


def chosen_sigmas(walks):
    """-> (plain, list): the largest grid point at which all 20 read back at L = 1; the largest at which all 20 read back at L = 8 and fewer at L = 1
    (None when no grid point separates them)"""
    n = R.WALK["images"]
    one = {s: r for s, r, _ in walks[1][0]}
    full = [s for s, r in one.items() if r == n]
    sep = [s for s, r, _ in walks[8][0] if r == n and one[s] < n]
    return (max(full) if full else None), (max(sep) if sep else None)


# the recorded outcome: `chosen_sigmas(walk(code))` and the counts right + ok at the list point, asserted by tests/test_ecc_rate_host.py
# No grid point separates L = 8 from L = 1 for either punctured code under these draws (the list adds images only where L = 8 is itself short of 20), so the list
# end-to-end test runs at the L = 1 point.
RATE_WALK = {"conv23": {"sigma": 1.75, "list_sigma": None, "reads": {1: 20, 2: 20, 4: 20, 8: 20}},
             "conv34": {"sigma": 1.75, "list_sigma": None, "reads": {1: 20, 2: 20, 4: 20, 8: 20}}}
