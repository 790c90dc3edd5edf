"""Microbenchmark of the blind key search (codec.key_search_topk -> gsw_key_search_topk, csrc/gswm_keysearch.inc: every key of a keyring
scored without a message) against the only route the tree offered before it, timed in the same process: a Python loop over the keys of
`codec.extract_batch(return_counts=True)` -- one launch per key, and the statistic sum_t |2 c_t - V| still to be formed from the counts
(the loop is timed WITHOUT that step and without a host round trip, which favours the loop).

Cases: 64 images of 4 x 64 x 64 (16384 lattice bits) against 2^10 and 2^16 keys, at message lengths of 256 and 2048 bits.  Every shape is
warmed up first, then --reps rounds alternate a timed window of the search launch (through the C ABI and through the Python wrapper) and,
at 2^10 keys, a timed window of the loop over all 2^10 keys (device events around back-to-back calls, a device synchronise at the end of
every window).  The loop is measured at 2^10 keys only; its figure at 2^16 keys is the per-key time multiplied out -- EXTRAPOLATED, marked
with '~'.  `quant_pack` (once per batch, whatever the number of keys) is timed separately.  Before timing, the search at 2^10 keys is
compared with the statistic formed from the loop's counts: every image's best key and statistic must be equal.

Reported: median [min .. max] over the rounds and the keys searched per second.  No rate is promised in advance: the loop in the same run
is the yardstick.

usage: python tools/key_search_bench.py [--reps 5] [--window-ms 30] [--k 1] [--out profiles/key_search_bench.txt] [--json FILE] [--quick]
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
from gswm_amd import _native as N, codec  # noqa: E402

LOOP_KEYS = 1 << 10
B, SHAPE = 64, (4, 64, 64)


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
    ap.add_argument("--k", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_search_bench.txt"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--quick", action="store_true", help="two rounds")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "key_search_bench needs the GPU (there is no CPU path to time)"
    lib, dev = N.lib(), torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    Us = (1 << 10, 1 << 16)
    reps = 2 if a.quick else a.reps
    n = 1
    for s in SHAPE:
        n *= s
    keys_all = torch.randint(0, 256, (max(Us), 48), dtype=torch.uint8, device=dev, generator=g)
    head = keys_all[:LOOP_KEYS].cpu().numpy()
    pairs = [(head[u, :32].tobytes(), head[u, 32:48].tobytes()) for u in range(LOOP_KEYS)]
    rows, k = [], a.k
    from bench_board import BoardSampler
    with BoardSampler(0) as board:
        for mb in (32, 256):
            M = 8 * mb
            V = n // M
            owner = LOOP_KEYS // 3
            z = torch.randn(B, *SHAPE, device=dev, generator=g).half()
            z[0] = codec.embed_batch(pairs[owner][0], pairs[owner][1], bytes(range(256))[:mb], 1, SHAPE, seed=1).half()[0]
            signs, _ = codec.quant_pack(z, 1)

            def loop(out=None):
                for u in range(LOOP_KEYS):
                    counts = codec.extract_batch(z, pairs[u][0], pairs[u][1], M, return_counts=True)[2]
                    if out is not None:
                        out.append((2 * counts - V).abs().sum(dim=1, keepdim=True))

            # the two routes agree at 2^10 keys
            got_idx, got_stat = codec.key_search_topk(signs, n, keys_all[:LOOP_KEYS], mb, k=1)
            per_key = []
            loop(per_key)
            all_stats = torch.cat(per_key, dim=1)                                       # [B, keys]
            want_stat, want_idx = all_stats.max(dim=1)
            assert torch.equal(got_stat[:, 0].long(), want_stat.long()) and int(got_idx[0, 0]) == owner and int(got_stat[0, 0]) == n
            unique_top = (all_stats == want_stat[:, None]).sum(dim=1) == 1
            assert torch.equal(got_idx[unique_top, 0].long(), want_idx[unique_top]), "the search launch and the per-key loop disagree"

            pack_fn = lambda: codec.quant_pack(z, 1)
            pack_iters = calibrate(pack_fn, a.window_ms)
            loop()                                                                      # warm-up of the loop at this shape
            torch.cuda.synchronize()
            loop_t, pack_t = [], []
            for U in Us:
                keys = keys_all[:U]
                idx = torch.empty((B, k), dtype=torch.int32, device=dev)
                stat = torch.empty((B, k), dtype=torch.int32, device=dev)
                ws = torch.empty(lib.gsw_key_search_workspace_bytes(B, U, k) // 8, dtype=torch.int64, device=dev)
                st = codec._stream_ptr()
                fns = {"abi": lambda: lib.gsw_key_search_topk(signs.data_ptr(), B, n, keys.data_ptr(), 48, mb, U, k, idx.data_ptr(), stat.data_ptr(), ws.data_ptr(), st),
                       "call": lambda: codec.key_search_topk(signs, n, keys, mb, k=k)}
                iters = {name: calibrate(f, a.window_ms) for name, f in fns.items()}
                t = {name: [] for name in fns}
                for _ in range(reps):                                                   # alternate the versions inside every round
                    for name, f in fns.items():
                        t[name].append(window(f, iters[name]))
                    if U == LOOP_KEYS:
                        loop_t.append(window(loop, 1))
                        pack_t.append(window(pack_fn, pack_iters))
                row = {"U": U, "B": B, "n": n, "msg_bits": M, "k": k, "iters": iters}
                for name in fns:
                    row[name] = {"median_us": statistics.median(t[name]), "min_us": min(t[name]), "max_us": max(t[name])}
                per = statistics.median(loop_t) / LOOP_KEYS
                row["loop_per_key_us"] = {"median_us": per, "min_us": min(loop_t) / LOOP_KEYS, "max_us": max(loop_t) / LOOP_KEYS}
                row["loop_us"] = per * U
                row["loop_extrapolated"] = U != LOOP_KEYS
                row["quant_pack_us"] = statistics.median(pack_t)
                row["keys_per_s"] = U / row["abi"]["median_us"] * 1e6
                row["loop_over_call"] = row["loop_us"] / row["call"]["median_us"]
                row["faster_beyond_spread"] = (row["call"]["max_us"] < min(loop_t)) if U == LOOP_KEYS else None
                rows.append(row)
                del ws
    out = io.StringIO()
    p = lambda *x: print(*x, file=out)
    p(f"{B} images of {' x '.join(map(str, SHAPE))} ({n} bits), k = {k}; median [min .. max] us per call over {reps} alternating rounds of ~{a.window_ms:.0f} ms windows; "
      f"device: {torch.cuda.get_device_name(0)}; board: {json.dumps(board.summary())}")
    p(f"loop = extract_batch(return_counts=True) per key, the statistic not formed, no host round trip; measured at {LOOP_KEYS} keys, '~' = per-key time x keys (extrapolated)")
    p(f"{'M':>5s} {'keys':>8s} {'abi us':>32s} {'call us':>32s} {'loop us/key':>24s} {'loop us':>14s} {'loop/call':>10s} {'keys/s':>10s} {'quant_pack us':>13s}")
    for r in rows:
        f = lambda d: f"{d['median_us']:10.1f} [{d['min_us']:.1f} .. {d['max_us']:.1f}]"
        p(f"{r['msg_bits']:5d} {r['U']:8d} {f(r['abi']):>32s} {f(r['call']):>32s} {f(r['loop_per_key_us']):>24s} {('~' if r['loop_extrapolated'] else ' ') + format(r['loop_us'], '.0f'):>14s} "
          f"{r['loop_over_call']:10.1f} {r['keys_per_s']:10.3g} {r['quant_pack_us']:13.1f}")
    p("the search launch and the statistic formed from the per-key loop's counts agree on every image's best key and statistic at every timed shape (2^10 keys)")
    measured = [r for r in rows if not r["loop_extrapolated"]]
    p("the search launch is faster than the per-key loop beyond the spread at 2^10 keys in every case" if all(r["faster_beyond_spread"] for r in measured)
      else "the search launch is NOT faster than the per-key loop beyond the spread at 2^10 keys in every case")
    print(out.getvalue(), end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(out.getvalue())
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"rows": rows, "board": board.summary()}, fh, indent=1)


if __name__ == "__main__":
    main()
