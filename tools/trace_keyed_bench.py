"""Microbenchmark of the keyed registry search (codec.trace_keyed_topk -> gsw_trace_keyed_topk, csrc/gswm_keyed.hip: every record has
its own ChaCha20 key and nonce) against the only route the single-key tools offer for such a registry, timed in the same process:
a Python loop over the keys of `codec.extract_batch(return_counts=True)` + `codec.trace_topk` on a one-row registry -- two launches
per key.  The loop is timed WITHOUT the host round trip per key that a caller needs to compare the scores, which favours the loop.

Per case (32-byte messages; U records x B images x n lattice bits): every shape is warmed up first, then --reps rounds alternate a
timed window of the keyed launch and, at U = 2^10, a timed window of the loop over all 2^10 keys (device events around back-to-back
calls, a device synchronise at the end of every window).  The loop is measured at 2^10 keys only and reported per key; its figures
at 2^16 and 2^20 keys are that per-key time multiplied out -- EXTRAPOLATED, marked with '~'.  `sign_pack` (once per batch, whatever
the number of keys) is timed separately.  Before timing, the keyed result at 2^10 keys is compared with the loop's scores: best index
and score must be equal.

Reported: median [min .. max] over the rounds, the records searched per second, the lane-operations the algorithm needs
(U B n / 32 xor + popcount pairs plus 16 n / 512 ChaCha20 quarter-lane blocks of ~320 operations per record) over the median time.

usage: python tools/trace_keyed_bench.py [--reps 5] [--window-ms 30] [--k 1] [--json FILE] [--quick]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gswm_amd  # noqa: E402,F401
from gswm_amd import _native as N, codec  # noqa: E402

MSG_BYTES = 32
M = 8 * MSG_BYTES
LOOP_KEYS = 1 << 10


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


def lane_ops(U, B, n):
    """what the algorithm needs: an xor and a popcount per 32 bits, record and image; 4 lanes x ~320 operations per 64-byte block"""
    return U * B * (n // 32) * 2 + U * ((n // 8 + 63) // 64) * 4 * 320


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--k", type=int, default=1)
    ap.add_argument("--json", default=None)
    ap.add_argument("--quick", action="store_true", help="U up to 2^16, two rounds")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "trace_keyed_bench needs the GPU (there is no CPU path to time)"
    lib, dev = N.lib(), torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    Us = (1 << 10, 1 << 16) if a.quick else (1 << 10, 1 << 16, 1 << 20)
    reps = 2 if a.quick else a.reps
    stride = codec.keyed_record_stride(MSG_BYTES)
    records_all = torch.randint(0, 256, (max(Us), stride), dtype=torch.uint8, device=dev, generator=g)
    head = records_all[:LOOP_KEYS].cpu().numpy()
    keys = [(head[u, :32].tobytes(), head[u, 32:48].tobytes()) for u in range(LOOP_KEYS)]
    one_row = [records_all[u:u + 1, 48:48 + MSG_BYTES].contiguous().clone() for u in range(LOOP_KEYS)]     # the one-row registries of the loop
    rows, k = [], a.k
    from bench_board import BoardSampler
    with BoardSampler(0) as board:
        for n in (16384, 65536):
            V = n // M
            for B in (1, 64):
                z = torch.randn(B, n, device=dev, generator=g).half()
                z[0] = codec.embed_batch(keys[LOOP_KEYS // 3][0], keys[LOOP_KEYS // 3][1], bytes(head[LOOP_KEYS // 3, 48:48 + MSG_BYTES]), 1, (n,), seed=1).half()[0]
                signs, _ = codec.sign_pack(z)

                def loop(scores=None):
                    for u in range(LOOP_KEYS):
                        counts = codec.extract_batch(z, keys[u][0], keys[u][1], M, return_counts=True)[2]
                        s = codec.trace_topk(counts, V, one_row[u], k=1, soft=True)[1]
                        if scores is not None:
                            scores.append(s)

                # the two routes agree at 2^10 keys
                got_idx, got_score = codec.trace_keyed_topk(signs, n, records_all[:LOOP_KEYS], MSG_BYTES, k=1)
                scores = []
                loop(scores)
                all_scores = torch.cat(scores, dim=1)                                  # [B, keys]
                want_score, want_idx = all_scores.max(dim=1)                           # (ties: random data has none at the top; checked below)
                assert torch.equal(got_score[:, 0], want_score) and int(got_idx[0, 0]) == LOOP_KEYS // 3 and int(got_score[0, 0]) == n
                unique_top = (all_scores == want_score[:, None]).sum(dim=1) == 1
                assert torch.equal(got_idx[unique_top, 0].long(), want_idx[unique_top]), "the keyed launch and the per-key loop disagree"

                pack = {"fn": lambda: codec.sign_pack(z)}
                pack["iters"] = calibrate(pack["fn"], a.window_ms)
                loop_iters = 1
                loop()                                                                  # warm-up of the loop at this shape
                torch.cuda.synchronize()
                loop_t, pack_t = [], []
                for U in Us:
                    recs = records_all[:U]
                    idx = torch.empty((B, k), dtype=torch.int32, device=dev)
                    score = torch.empty((B, k), dtype=torch.int32, device=dev)
                    ws = torch.empty(lib.gsw_trace_keyed_workspace_bytes(B, U, k) // 8, dtype=torch.int64, device=dev)
                    st = codec._stream_ptr()
                    fns = {"abi": lambda: lib.gsw_trace_keyed_topk(signs.data_ptr(), B, n, recs.data_ptr(), stride, MSG_BYTES, U, k, idx.data_ptr(), score.data_ptr(), ws.data_ptr(), st),
                           "call": lambda: codec.trace_keyed_topk(signs, n, recs, MSG_BYTES, k=k)}
                    iters = {name: calibrate(f, a.window_ms) for name, f in fns.items()}
                    t = {name: [] for name in fns}
                    for _ in range(reps):                                               # alternate the versions inside every round
                        for name, f in fns.items():
                            t[name].append(window(f, iters[name]))
                        if U == LOOP_KEYS:
                            loop_t.append(window(loop, loop_iters))
                            pack_t.append(window(pack["fn"], pack["iters"]))
                    row = {"U": U, "B": B, "n": n, "k": k, "iters": iters}
                    for name in fns:
                        row[name] = {"median_us": statistics.median(t[name]), "min_us": min(t[name]), "max_us": max(t[name])}
                    per_key = statistics.median(loop_t) / LOOP_KEYS
                    row["loop_per_key_us"] = {"median_us": per_key, "min_us": min(loop_t) / LOOP_KEYS, "max_us": max(loop_t) / LOOP_KEYS}
                    row["loop_us"] = per_key * U
                    row["loop_extrapolated"] = U != LOOP_KEYS
                    row["sign_pack_us"] = statistics.median(pack_t)
                    row["records_per_s"] = U / row["abi"]["median_us"] * 1e6
                    row["lane_Gops_per_s"] = lane_ops(U, B, n) / row["abi"]["median_us"] / 1e3
                    row["loop_over_call"] = row["loop_us"] / row["call"]["median_us"]
                    row["faster_beyond_spread"] = (row["call"]["max_us"] < min(loop_t)) if U == LOOP_KEYS else None
                    rows.append(row)
                    del ws
    print(f"{MSG_BYTES}-byte messages, k = {k}; median [min .. max] us per call over {reps} alternating rounds of ~{a.window_ms:.0f} ms windows; device: "
          f"{torch.cuda.get_device_name(0)}; board: {json.dumps(board.summary())}")
    print(f"loop = extract_batch(return_counts=True) + trace_topk on a one-row registry per key, no host round trip; measured at {LOOP_KEYS} keys, '~' = per-key time x U (extrapolated)")
    print(f"{'n':>6s} {'B':>3s} {'U':>8s} {'abi us':>30s} {'call us':>30s} {'loop us/key':>24s} {'loop us':>14s} {'loop/call':>10s} {'records/s':>10s} {'lane Gop/s':>10s} {'sign_pack us':>12s}")
    for r in rows:
        f = lambda d: f"{d['median_us']:10.1f} [{d['min_us']:.1f} .. {d['max_us']:.1f}]"
        print(f"{r['n']:6d} {r['B']:3d} {r['U']:8d} {f(r['abi']):>30s} {f(r['call']):>30s} {f(r['loop_per_key_us']):>24s} {('~' if r['loop_extrapolated'] else ' ') + format(r['loop_us'], '.0f'):>14s} "
              f"{r['loop_over_call']:10.1f} {r['records_per_s']:10.3g} {r['lane_Gops_per_s']:10.0f} {r['sign_pack_us']:12.1f}")
    print("the keyed launch and the per-key loop return the same best record and score at every timed shape (2^10 keys)")
    measured = [r for r in rows if not r["loop_extrapolated"]]
    print("the keyed launch is faster than the per-key loop beyond the spread at 2^10 keys in every case" if all(r["faster_beyond_spread"] for r in measured)
          else "the keyed launch is NOT faster than the per-key loop beyond the spread at 2^10 keys in every case")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"msg_bytes": MSG_BYTES, "rows": rows, "board": board.summary()}, fh, indent=1)


if __name__ == "__main__":
    main()
