"""Microbenchmark of the blind key search ranked by reliability levels (codec.key_search_soft_topk -> gsw_key_search_soft_topk,
csrc/gswm_keysearch_soft.inc) against the sign search (codec.key_search_topk) in the same run, and against the only route the tree offered
before it: a Python loop over the keys of `soft.extract_soft`'s launch (`codec.extract_soft` on record rows built once per key in advance), one launch per
key, the statistic sum_t |score[t]| still to be formed (the loop is timed WITHOUT that step and without a host round trip, which favours the loop).

Cases: 64 images of 4 x 64 x 64 (16384 lattice bits), 256-bit messages, keyrings of 2^10 and 2^16 keys, 1, 3 and 15 levels (1, 2 and 4 planes).
Every shape is warmed up first, then --reps rounds alternate a timed window of the sign search and of the soft search at each level (device
events around back-to-back calls, a device synchronise at the end of every window) and, at 2^10 keys, a timed window of the loop over all 2^10
keys at 15 levels.  The loop's figure at 2^16 keys is the per-key time multiplied out -- EXTRAPOLATED, marked with '~'.  `level_pack` (once per
batch, whatever the number of keys) is timed separately.  Before timing, the soft search at 2^10 keys is compared with the statistic formed from
the loop's scores: every image's best statistic must be equal.

Reported: median [min .. max] over the rounds.  No time is promised in advance: the sign search and the loop in the same run are the yardsticks.

usage: python tools/key_search_soft_bench.py [--reps 5] [--window-ms 30] [--out profiles/key_search_soft_bench.txt] [--json FILE] [--quick]
"""
import argparse
import io
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gswm_amd  # noqa: E402,F401
from gswm_amd import codec, soft  # noqa: E402

LOOP_KEYS = 1 << 10
B, SHAPE, MSG_BYTES = 64, (4, 64, 64), 32
LEVELS = (1, 3, 15)


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3          # us per call


def calibrate(fn, window_ms, most=2000):
    for _ in range(2):                              # warm-up of this shape
        fn()
    torch.cuda.synchronize()
    t = window(fn, 2)
    return max(2, min(most, int(window_ms * 1e3 / max(t, 1.0))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_search_soft_bench.txt"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--quick", action="store_true", help="two rounds")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "key_search_soft_bench needs the GPU (there is no CPU path to time)"
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    Us = (1 << 10, 1 << 16)
    reps = 2 if a.quick else a.reps
    n = 1
    for s in SHAPE:
        n *= s
    M = 8 * MSG_BYTES
    keys_all = torch.randint(0, 256, (max(Us), 48), dtype=torch.uint8, device=dev, generator=g)
    head = keys_all[:LOOP_KEYS].cpu().numpy()
    pairs = [(head[u, :32].tobytes(), head[u, 32:48].tobytes()) for u in range(LOOP_KEYS)]
    owner = LOOP_KEYS // 3
    z = torch.randn(B, *SHAPE, device=dev, generator=g).half()
    z[0] = codec.embed_batch(pairs[owner][0], pairs[owner][1], bytes(range(256))[:MSG_BYTES], 1, SHAPE, seed=1).half()[0]
    signs, _ = codec.quant_pack(z, 1)
    thr = {L: soft.uniform_thresholds(z, L) for L in LEVELS}
    packed = {L: codec.level_pack(z, thr[L]) for L in LEVELS}

    recs = [soft.shared_records(key, nonce, MSG_BYTES, B, dev) for key, nonce in pairs]         # the rows soft.extract_soft builds per call, built once

    def loop(out=None, L=15):
        for u in range(LOOP_KEYS):
            score = codec.extract_soft(z, recs[u], MSG_BYTES, thr[L]).score
            if out is not None:
                out.append(score.abs().sum(dim=1, keepdim=True))

    # the two routes agree at 2^10 keys, at every level
    for L in LEVELS:
        got_idx, got_stat = codec.key_search_soft_topk(packed[L], n, keys_all[:LOOP_KEYS], MSG_BYTES, k=1)
        per_key = []
        loop(per_key, L)
        want_stat = torch.cat(per_key, dim=1).max(dim=1)[0]
        assert torch.equal(got_stat[:, 0].long(), want_stat.long()) and int(got_idx[0, 0]) == owner, "the search launch and the per-key loop disagree"

    rows = []
    from bench_board import BoardSampler
    with BoardSampler(0) as board:
        pack_fn = lambda: codec.level_pack(z, thr[15])
        pack_iters = calibrate(pack_fn, a.window_ms)
        loop()                                                                          # warm-up of the loop
        torch.cuda.synchronize()
        loop_t, pack_t = [], []
        for U in Us:
            keys = keys_all[:U]
            fns = {"sign": lambda: codec.key_search_topk(signs, n, keys, MSG_BYTES, k=1)}
            for L in LEVELS:
                fns[f"soft{L}"] = lambda L=L: codec.key_search_soft_topk(packed[L], n, keys, MSG_BYTES, k=1)
            iters = {name: calibrate(f, a.window_ms) for name, f in fns.items()}
            t = {name: [] for name in fns}
            for _ in range(reps):                                                       # alternate the versions inside every round
                for name, f in fns.items():
                    t[name].append(window(f, iters[name]))
                if U == LOOP_KEYS:
                    loop_t.append(window(loop, 1))
                    pack_t.append(window(pack_fn, pack_iters))
            row = {"U": U, "B": B, "n": n, "msg_bits": M, "iters": iters}
            for name in fns:
                row[name] = {"median_us": statistics.median(t[name]), "min_us": min(t[name]), "max_us": max(t[name])}
            per = statistics.median(loop_t) / LOOP_KEYS
            row["loop_per_key_us"] = {"median_us": per, "min_us": min(loop_t) / LOOP_KEYS, "max_us": max(loop_t) / LOOP_KEYS}
            row["loop_us"] = per * U
            row["loop_extrapolated"] = U != LOOP_KEYS
            row["level_pack_us"] = statistics.median(pack_t)
            rows.append(row)
    out = io.StringIO()
    p = lambda *x: print(*x, file=out)
    p(f"{B} images of {' x '.join(map(str, SHAPE))} ({n} bits), {M}-bit messages, k = 1; median [min .. max] us per call (Python wrapper) over {reps} alternating rounds of "
      f"~{a.window_ms:.0f} ms windows; device: {torch.cuda.get_device_name(0)}; board: {json.dumps(board.summary())}")
    p(f"loop = codec.extract_soft (soft.extract_soft's launch, its record rows built in advance) at 15 levels per key, the statistic not formed, no host round trip; measured at {LOOP_KEYS} keys, '~' = per-key time x keys (extrapolated)")
    f = lambda d: f"{d['median_us']:10.1f} [{d['min_us']:.1f} .. {d['max_us']:.1f}]"
    p(f"{'keys':>8s} {'sign search us':>32s} " + " ".join(f"{f'{L} levels us':>32s} {'x sign':>7s}" for L in LEVELS) + f" {'loop us/key':>24s} {'loop us':>14s} {'level_pack us':>13s}")
    for r in rows:
        cols = " ".join(f"{f(r[f'soft{L}']):>32s} {r[f'soft{L}']['median_us'] / r['sign']['median_us']:7.2f}" for L in LEVELS)
        p(f"{r['U']:8d} {f(r['sign']):>32s} {cols} {f(r['loop_per_key_us']):>24s} {('~' if r['loop_extrapolated'] else ' ') + format(r['loop_us'], '.0f'):>14s} {r['level_pack_us']:13.1f}")
    p("the search launch and the statistic formed from the per-key loop's scores agree on every image's best statistic at 2^10 keys, at every level")
    print(out.getvalue(), end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(out.getvalue())
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"rows": rows, "board": board.summary()}, fh, indent=1)


if __name__ == "__main__":
    main()
