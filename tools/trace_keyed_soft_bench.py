"""Microbenchmark of the level-weighted keyed registry search (codec.trace_keyed_soft_topk -> gsw_trace_keyed_soft_topk,
csrc/gswm_keyed_soft.inc) against its two yardsticks, timed in the same process:
  * the sign search of the same run (gsw_trace_keyed_topk on the same images and records), and
  * at 2^10 distinct keys, the only thing a caller could do before: per key, `soft.extract_soft` + `codec.trace_topk` on a one-row
    registry (fed through `trace.reliability_counts`) -- two launches and a few torch operations per key, timed WITHOUT the host round trip
    per key that a caller needs to compare the scores, which favours the loop.
`codec.level_pack` is timed against `codec.sign_pack` (both once per batch, whatever the number of records).

Inputs: 64 images of 4 x 64 x 64 (fp16) against 2^10, 2^16 and 2^20 records with 32-byte messages; variants: the sign search and the soft
search at 1, 3 and 15 levels (1, 2 and 4 planes; tiles of 16, 16 and 4 images).  Every shape is warmed up first, then --reps rounds
alternate one timed window per variant (device events around back-to-back C ABI calls, a device synchronise at the end of every window);
reported is the median [min .. max] over the rounds and the ratio to the sign search.  Before timing, the soft search at 2^10 keys is
compared with the loop's scores (best index and score must be equal) and the 1-level search at threshold 0 with the sign search.

usage: python tools/trace_keyed_soft_bench.py [--reps 5] [--window-ms 30] [--json FILE] [--quick]
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
from gswm_amd import _native as N, codec, soft, trace  # noqa: E402

MSG_BYTES = 32
M = 8 * MSG_BYTES
LOOP_KEYS = 1 << 10
B, SHAPE = 64, (4, 64, 64)
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


def stat(ts):
    return {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--json", default=None)
    ap.add_argument("--quick", action="store_true", help="U up to 2^16, two rounds")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "trace_keyed_soft_bench needs the GPU (there is no CPU path to time)"
    lib, dev = N.lib(), torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    Us = (1 << 10, 1 << 16) if a.quick else (1 << 10, 1 << 16, 1 << 20)
    reps = 2 if a.quick else a.reps
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]
    V = n // M
    stride = codec.keyed_record_stride(MSG_BYTES)
    records_all = torch.randint(0, 256, (max(Us), stride), dtype=torch.uint8, device=dev, generator=g)
    head = records_all[:LOOP_KEYS].cpu().numpy()
    keys = [(head[u, :32].tobytes(), head[u, 32:48].tobytes()) for u in range(LOOP_KEYS)]
    one_row = [records_all[u:u + 1, 48:48 + MSG_BYTES].contiguous().clone() for u in range(LOOP_KEYS)]     # the one-row registries of the loop
    owner = LOOP_KEYS // 3
    z = torch.randn(B, *SHAPE, device=dev, generator=g)
    z[0] = codec.embed_batch(keys[owner][0], keys[owner][1], bytes(head[owner, 48:48 + MSG_BYTES]), 1, SHAPE, seed=1)[0]
    z[0] = (z[0] + 2.0 * torch.randn(SHAPE, device=dev, generator=g)) / 5.0 ** 0.5                          # a noisy owner, back at unit variance
    z = z.half().contiguous()
    st = codec._stream_ptr()

    signs, _ = codec.sign_pack(z)
    tables = {T: soft.uniform_thresholds(z, T) for T in LEVELS}
    packed = {T: codec.level_pack(z, tables[T]) for T in LEVELS}

    def loop(T, scores=None):
        for u in range(LOOP_KEYS):
            vote = soft.extract_soft(z, keys[u][0], keys[u][1], M, thresholds=tables[T])
            counts, copies = trace.reliability_counts(vote.score, T, V)
            s = codec.trace_topk(counts, copies, one_row[u], k=1, soft=True)[1]
            if scores is not None:
                scores.append(s // 2)

    # the routes agree at 2^10 keys; one level at threshold 0 is the sign search
    for T in LEVELS:
        got_idx, got_score = codec.trace_keyed_soft_topk(packed[T], n, records_all[:LOOP_KEYS], MSG_BYTES, k=1)
        scores = []
        loop(T, scores)
        all_scores = torch.cat(scores, dim=1)                                  # [B, keys]
        want_score, want_idx = all_scores.max(dim=1)
        assert torch.equal(got_score[:, 0], want_score) and int(got_idx[0, 0]) == owner, "the keyed soft launch and the per-key loop disagree"
        unique_top = (all_scores == want_score[:, None]).sum(dim=1) == 1
        assert torch.equal(got_idx[unique_top, 0].long(), want_idx[unique_top]), "the keyed soft launch and the per-key loop disagree"
    sign_rows = codec.level_pack(z, torch.zeros(1, device=dev))
    a_, b_ = codec.trace_keyed_soft_topk(sign_rows, n, records_all[:LOOP_KEYS], MSG_BYTES, k=8), codec.trace_keyed_topk(signs, n, records_all[:LOOP_KEYS], MSG_BYTES, k=8)
    assert torch.equal(a_[0], b_[0]) and torch.equal(a_[1], b_[1]), "one level at threshold 0 is not the sign search"

    packs = {"sign_pack": lambda: codec.sign_pack(z)}
    for T in LEVELS:
        packs[f"level_pack {T}"] = (lambda T=T: codec.level_pack(z, tables[T]))
    pack_iters = {name: calibrate(f, a.window_ms) for name, f in packs.items()}
    pack_t = {name: [] for name in packs}
    loop_t = {T: [] for T in LEVELS}
    rows = []
    from bench_board import BoardSampler
    with BoardSampler(0) as board:
        for U in Us:
            recs = records_all[:U]
            idx = torch.empty((B, 1), dtype=torch.int32, device=dev)
            score = torch.empty((B, 1), dtype=torch.int32, device=dev)
            ws = torch.empty(lib.gsw_trace_keyed_workspace_bytes(B, U, 1) // 8, dtype=torch.int64, device=dev)
            fns = {"sign": lambda: lib.gsw_trace_keyed_topk(signs.data_ptr(), B, n, recs.data_ptr(), stride, MSG_BYTES, U, 1, idx.data_ptr(), score.data_ptr(), ws.data_ptr(), st)}
            for T in LEVELS:
                r = packed[T]
                fns[f"soft {T}"] = (lambda r=r, T=T: lib.gsw_trace_keyed_soft_topk(r.signs.data_ptr(), r.planes.data_ptr(), r.wsum.data_ptr(), T, B, n, recs.data_ptr(), stride,
                                                                                  MSG_BYTES, U, 1, idx.data_ptr(), score.data_ptr(), ws.data_ptr(), st))
            iters = {name: calibrate(f, a.window_ms) for name, f in fns.items()}
            t = {name: [] for name in fns}
            for _ in range(reps):                                               # alternate the variants inside every round
                for name, f in fns.items():
                    t[name].append(window(f, iters[name]))
                if U == LOOP_KEYS:
                    for T in LEVELS:
                        loop_t[T].append(window(lambda T=T: loop(T), 1))
                    for name, f in packs.items():
                        pack_t[name].append(window(f, pack_iters[name]))
            row = {"U": U, "B": B, "n": n, "iters": iters}
            for name in fns:
                row[name] = stat(t[name])
            for T in LEVELS:
                row[f"soft {T} over sign"] = row[f"soft {T}"]["median_us"] / row["sign"]["median_us"]
            rows.append(row)
            del ws
    loops = {T: stat(loop_t[T]) for T in LEVELS}
    pack = {name: stat(ts) for name, ts in pack_t.items()}
    f = lambda d: f"{d['median_us']:10.1f} [{d['min_us']:.1f} .. {d['max_us']:.1f}]"
    print(f"{B} images of {SHAPE[0]} x {SHAPE[1]} x {SHAPE[2]} (fp16), {MSG_BYTES}-byte messages, k = 1; median [min .. max] us per C ABI call over {reps} alternating rounds of "
          f"~{a.window_ms:.0f} ms windows; device: {torch.cuda.get_device_name(0)}; board: {json.dumps(board.summary())}")
    print(f"{'U':>8s} {'sign us':>32s} " + " ".join(f"{'soft ' + str(T) + ' us':>32s} {'/ sign':>7s}" for T in LEVELS))
    for r in rows:
        print(f"{r['U']:8d} {f(r['sign']):>32s} " + " ".join(f"{f(r['soft ' + str(T)]):>32s} {r['soft ' + str(T) + ' over sign']:7.2f}" for T in LEVELS))
    print(f"per-key loop (soft.extract_soft + trace_topk on a one-row registry, no host round trip) over {LOOP_KEYS} keys, and the one keyed soft launch over the same keys:")
    first = rows[0]
    for T in LEVELS:
        print(f"  {T:2d} levels: loop {f(loops[T])} us = {loops[T]['median_us'] / LOOP_KEYS:.1f} us per key; launch {f(first['soft ' + str(T)])} us; "
              f"loop / launch = {loops[T]['median_us'] / first['soft ' + str(T)]['median_us']:.0f}")
    print("once per batch: " + "; ".join(f"{name} {f(d)} us" for name, d in pack.items()))
    print("the keyed soft launch and the per-key loop return the same best record and score (2^10 keys, every level count); one level at threshold 0 returns the sign search's rows")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"msg_bytes": MSG_BYTES, "rows": rows, "loops": {str(T): v for T, v in loops.items()}, "pack": pack, "board": board.summary()}, fh, indent=1)


if __name__ == "__main__":
    main()
