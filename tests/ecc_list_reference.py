"""NumPy and plain-Python restatements of the list read of an error-corrected payload: the parallel list Viterbi decoder that keeps
the L best paths of every trellis state and lets the CRC pick among the L paths through state 0.  Code, interleaver, info word, branch metrics and tail are
`ecc_reference`'s, imported unchanged.  Integer arithmetic throughout: the device (`codec.viterbi_list_decode`) must equal both restatements bit for bit.

TWO independent restatements of one definition:
  `decode_list`        vectorised over images and states; survivor records are the d bit of every output rank, the traceback finds the predecessor's rank as
                       the number of lower output ranks with the same d (a popcount under a mask) -- the device's bookkeeping, restated
  `decode_list_plain`  one image at a time; every entry carries its whole path; the merge is Python's stable sort of the d = 0 entries followed by the d = 1
                       entries -- no records, no traceback, no popcount

The definition.  Every state s keeps a list of at most L (metric, path) entries, best first.  Before step 0 only state 0 has one: metric 0.  Step t forms the
list of s from the entries of 2 (s & 31) + d, d in {0, 1}; d = 0 entries take + bm, d = 1 entries - bm; the two sorted lists are merged and the first L kept:
higher metric first, on equal metrics d = 0 before d = 1, entries of one predecessor in their rank order.  In the last 6 steps only states with s >> 5 == 0
live.  After step T - 1 state 0 holds L paths; ok_r is `ecc_reference`'s ok rule on rank r; the selected rank is the lowest r with ok_r, 0 when none."""
import numpy as np

import ecc_reference as R

LIST_SIZES = (1, 2, 4, 8)
EMPTY = -(2 ** 62)                                                  # an empty slot's metric: below every sum of scores, never added to


def sizes(M):
    """`ecc_reference.sizes` without its upper limit of 8192: the list kernel's own bound is its LDS slice (`served`)"""
    assert M % 16 == 0 and M >= 64
    T = M // 2
    return T - R.TAIL, T, (T - R.TAIL - 16) // 8


def wave_lds(M, L):
    """bytes of one wavefront's LDS slice, restated from the README: M (5 + 1/16 + 9 L / 2) + 256 L, rounded up to 16"""
    raw = 4 * M + 256 * L + 4 * M * L + M * L // 2 + M + M // 16
    return (raw + 15) // 16 * 16


def served(M, L):
    return L in LIST_SIZES and M % 16 == 0 and M >= 64 and wave_lds(M, L) <= 160 * 1024


def largest_served(L):
    return max(M for M in range(64, 20000, 16) if served(M, L))


def _check(score, L):
    score = np.asarray(score)
    assert score.ndim == 2 and np.issubdtype(score.dtype, np.integer) and L in LIST_SIZES
    assert int(np.abs(score.astype(np.int64)).sum(axis=1).max()) < 2 ** 30
    return score


def _ok(bits, pb):
    """`ecc_reference`'s ok rule on the T input bits of a path: the CRC of the payload bytes matches and the last info byte is zero"""
    info = np.packbits(np.asarray(bits, dtype=np.uint8))
    return bool(R.crc16(info[:pb].tobytes()) == (int(info[pb]) << 8 | int(info[pb + 1])) and info[pb + 2] == 0)


def _recode(ub):
    """input bits [B, T] -> code bits [B, 2 T]: delay k of the input meets bit 6 - k of the generators"""
    B, T = ub.shape
    up = np.concatenate([np.zeros((B, R.TAIL), dtype=np.uint8), ub], axis=1)
    c = np.zeros((B, T, 2), dtype=np.uint8)
    for k in range(R.TAIL + 1):
        past = up[:, R.TAIL - k:R.TAIL - k + T]
        if (R.G0 >> (6 - k)) & 1:
            c[:, :, 0] ^= past
        if (R.G1 >> (6 - k)) & 1:
            c[:, :, 1] ^= past
    return c.reshape(B, 2 * T)


_POPCOUNT = np.array([bin(v).count("1") for v in range(256)], dtype=np.int64)


# ------------------------------------------------------------------------------------------------ restatement 1: vectorised, d-bit records, popcount traceback
def decode_list(score, L, interleave=True, all_ranks=False) -> dict:
    """score int [B, M] -> info uint8 [B, M/16], message uint8 [B, M/8], metric, flips, ok, rank, n_ok int32 [B] of the selected path.
    all_ranks: also `metrics` int64 [B, L], `inputs` uint8 [B, L, T] and `oks` bool [B, L] of every rank through state 0"""
    score = _check(score, L)
    B, M = score.shape
    I, T, pb = sizes(M)
    pos = R.positions(M, interleave)
    x = score.astype(np.int64)[:, pos]
    s = np.arange(64)
    p0, u = 2 * (s & 31), s >> 5
    l0, l1 = R._labels()
    sg0, sg1 = 2 * l0 - 1, 2 * l1 - 1
    pm = np.full((B, 64, L), EMPTY, dtype=np.int64)
    pm[:, 0, 0] = 0
    dec = np.zeros((T, B, 64), dtype=np.int64)                      # bit k: output rank k of the state came from d = 1
    for t in range(T):
        bm = (sg0[None, :] * x[:, 2 * t, None] + sg1[None, :] * x[:, 2 * t + 1, None])[:, :, None]
        a, b = pm[:, p0, :], pm[:, p0 + 1, :]
        a = np.where(a == EMPTY, EMPTY, a + bm)
        b = np.where(b == EMPTY, EMPTY, b - bm)
        pad = np.full((B, 64, 1), EMPTY, dtype=np.int64)            # a list read past its end is empty
        a, b = np.concatenate([a, pad], axis=2), np.concatenate([b, pad], axis=2)
        i = np.zeros((B, 64, 1), dtype=np.int64)
        j = np.zeros((B, 64, 1), dtype=np.int64)
        out = np.empty((B, 64, L), dtype=np.int64)
        bits = np.zeros((B, 64), dtype=np.int64)
        for k in range(L):
            ha, hb = np.take_along_axis(a, i, axis=2), np.take_along_axis(b, j, axis=2)
            tb = hb > ha                                            # strict: equal metrics go to d = 0; two empty heads leave an empty slot
            out[:, :, k] = np.where(tb, hb, ha)[:, :, 0]
            bits |= tb[:, :, 0].astype(np.int64) << k
            i, j = i + ~tb, j + tb
        if t >= I:
            out[:, u != 0, :] = EMPTY
        pm, dec[t] = out, bits
    assert (pm[:, 0, :] != EMPTY).all()                             # 2^I >= 2^26 paths end in state 0: its list is full
    rows = np.arange(B)
    inputs = np.zeros((B, L, T), dtype=np.uint8)
    for r in range(L):
        st, k = np.zeros(B, dtype=np.int64), np.full(B, r, dtype=np.int64)
        for t in range(T - 1, -1, -1):
            rec = dec[t][rows, st]
            d = (rec >> k) & 1
            same1 = _POPCOUNT[rec & ((1 << k) - 1)]                 # lower output ranks that came from d = 1
            inputs[:, r, t] = st >> 5
            k = np.where(d == 1, same1, k - same1)
            st = 2 * (st & 31) + d
        assert (st == 0).all() and (k == 0).all()                   # every path starts as the one entry of state 0
    oks = np.array([[_ok(inputs[b, r], pb) for r in range(L)] for b in range(B)], dtype=bool)
    return _outputs(score, pos, pm[:, 0, :], inputs, oks, all_ranks)


def _outputs(score, pos, metrics, inputs, oks, all_ranks):
    B, M = score.shape
    n_ok = oks.sum(axis=1).astype(np.int32)
    rank = np.where(n_ok > 0, oks.argmax(axis=1), 0).astype(np.int32)
    rows = np.arange(B)
    ub = inputs[rows, rank]
    msg = np.zeros((B, M), dtype=np.uint8)
    msg[:, pos] = _recode(ub)
    out = {"info": np.packbits(ub, axis=1), "message": np.packbits(msg, axis=1), "metric": metrics[rows, rank].astype(np.int32),
           "flips": (msg != (score > 0)).sum(axis=1).astype(np.int32), "ok": oks[rows, rank].astype(np.int32), "rank": rank, "n_ok": n_ok}
    if all_ranks:
        out.update(metrics=np.asarray(metrics, dtype=np.int64), inputs=inputs, oks=oks)
    return out


# ------------------------------------------------------------------------------------------------ restatement 2: whole paths, a stable sort
def decode_list_plain(score, L, interleave=True, all_ranks=False) -> dict:
    """the same outputs, from lists of (metric, path) per state; a path is a chain of (earlier path, input) cells, unrolled at the end"""
    score = _check(score, L)
    B, M = score.shape
    I, T, pb = sizes(M)
    S = R.interleaver_step(M)
    par = lambda v: bin(v).count("1") & 1
    metrics, inputs, oks = np.zeros((B, L), dtype=np.int64), np.zeros((B, L, T), dtype=np.uint8), np.zeros((B, L), dtype=bool)
    for b in range(B):
        row = [int(v) for v in score[b]]
        x = [row[(i * S) % M if interleave else i] for i in range(M)]
        lists = [[] for _ in range(64)]
        lists[0] = [(0, None)]
        for t in range(T):
            new = [[] for _ in range(64)]
            for s in range(64):
                inp = s >> 5
                if t >= I and inp:
                    continue
                both = []
                for d in (0, 1):
                    p = 2 * (s & 31) + d
                    r = (inp << 6) | p
                    bm = (2 * par(r & R.G0) - 1) * x[2 * t] + (2 * par(r & R.G1) - 1) * x[2 * t + 1]
                    both += [(m + bm, (path, inp)) for m, path in lists[p]]       # d = 0 entries first, each predecessor's in rank order
                both.sort(key=lambda e: -e[0])                                     # stable: equal metrics keep that order
                new[s] = both[:L]
            lists = new
        assert len(lists[0]) == L
        for r, (m, path) in enumerate(lists[0]):
            bits = []
            while path is not None:
                path, inp = path
                bits.append(inp)
            assert len(bits) == T
            metrics[b, r], inputs[b, r] = m, bits[::-1]
            oks[b, r] = _ok(inputs[b, r], pb)
    return _outputs_plain(score, metrics, inputs, oks, interleave, all_ranks)


def _outputs_plain(score, metrics, inputs, oks, interleave, all_ranks):
    """the selected path's outputs by `ecc_reference`'s own encoder, one image at a time"""
    B, M = score.shape
    I = sizes(M)[0]
    out = {k: [] for k in ("info", "message", "metric", "flips", "ok", "rank", "n_ok")}
    for b in range(B):
        passing = [r for r in range(oks.shape[1]) if oks[b, r]]
        r = passing[0] if passing else 0
        S = R.interleaver_step(M)
        code = R.conv_encode(inputs[b, r])
        msg = np.zeros(M, dtype=np.uint8)
        msg[[(i * S) % M if interleave else i for i in range(M)]] = code
        assert inputs[b, r, I:].sum() == 0                          # the tail
        out["info"].append(np.packbits(inputs[b, r]))
        out["message"].append(np.packbits(msg))
        out["metric"].append(int(metrics[b, r]))
        out["flips"].append(int((msg != (score[b] > 0)).sum()))
        out["ok"].append(int(oks[b, r]))
        out["rank"].append(r)
        out["n_ok"].append(len(passing))
    res = {k: (np.stack(v) if k in ("info", "message") else np.array(v, dtype=np.int32)) for k, v in out.items()}
    if all_ranks:
        res.update(metrics=metrics, inputs=inputs, oks=oks)
    return res


NAMES = ("info", "message", "metric", "flips", "ok", "rank", "n_ok")


def format_read_list(d, b, M, L):
    """the text of `ecc.format_read_list`, restated from the issue"""
    pb = sizes(M)[2]
    text = f"payload {d['info'][b, :pb].tobytes().hex()} crc {'ok' if d['ok'][b] else 'FAILED'}, corrected {d['flips'][b]} of {M}, list rank {d['rank'][b]} of {L}"
    return text + (f", {d['n_ok'][b]} candidates pass" if d["n_ok"][b] > 1 else "")


# ------------------------------------------------------------------------------------------------ the sigma walk (tools/ecc_list_sigma_walk.py, the end-to-end tests)
def blank_scores(setup):
    """score int32 [64, 256]: the votes of the walk's 64 unwatermarked latents under key 0, 15 uniform levels on each one's own RMS"""
    import gs_oracle as O
    import soft_reference as SR
    blank = setup["blank"]
    ks = np.frombuffer(O.chacha20_keystream(setup["keys"][0], setup["nonces"][0], blank.shape[1] // 8), dtype=np.uint8)
    return np.stack([SR.soft_vote(row, ks, R.uniform_thresholds32(row), R.WALK["M"])["score"] for row in blank]).astype(np.int32)


def walk_scores_all():
    """-> (setup, {sigma: score int32 [20, 256]}, blank score int32 [64, 256]): `ecc_reference`'s walk, its coded latents and votes, computed once"""
    W = R.WALK
    setup = R.walk_setup()
    z = R.walk_latents(setup, [R.encode(p, W["M"]) for p in setup["payloads"]])
    scores = {s: R.walk_scores(setup, R.held(z, setup["noise"], s), W["M"])[0] for s in W["sigmas"]}
    return setup, scores, blank_scores(setup)


def count_reads(d, payloads, M):
    """-> (right + ok, wrong + ok) of a decode against the payloads that were sent"""
    got = R.payloads(d["info"], M)
    right = sum(1 for b, p in enumerate(payloads) if d["ok"][b] and got[b] == p)
    return right, int(d["ok"].sum()) - right


def walk_list(L, inputs=None):
    """-> ([(sigma, right + ok, wrong + ok)] over the grid, the number of the 64 blank latents with ok), all at list size L"""
    setup, scores, blank = inputs or walk_scores_all()
    M = R.WALK["M"]
    table = [(s,) + count_reads(decode_list(scores[s], L), setup["payloads"], M) for s in R.WALK["sigmas"]]
    return table, int(decode_list(blank, L)["ok"].sum())


def walk_lists():
    """{L: walk_list(L)} for the four list sizes, on one set of votes"""
    inputs = walk_scores_all()
    return {L: walk_list(L, inputs) for L in LIST_SIZES}


def chosen_sigma(walks):
    """the LARGEST grid point at which all 20 payloads read back at L = 8 and fewer than 20 at L = 1; None when no grid point separates them"""
    n = R.WALK["images"]
    one = {s: r for s, r, _ in walks[1][0]}
    sep = [s for s, r, _ in walks[8][0] if r == n and one[s] < n]
    return max(sep) if sep else None


# the recorded outcome: `chosen_sigma(walk_lists())` and the counts right + ok there, asserted by tests/test_ecc_list_host.py
LIST_WALK = {"sigma": 2.75, "reads": {1: 16, 2: 18, 4: 20, 8: 20}}
