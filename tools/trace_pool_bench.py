"""Microbenchmark of the pooled trace (codec.pool_rows -> gsw_pool_rows, codec.trace_keyed_pooled_topk -> gsw_trace_keyed_pooled_topk, csrc/gswm_pool.inc) against
what a caller runs today on the same images, timed in the same process: the per-image search over the set (gsw_trace_keyed_topk at unit levels,
gsw_trace_keyed_soft_topk at 15 levels; one launch over the set's images), which scores every image alone and does not answer the set's question.

Inputs: ONE set of 16, 64 and 256 images of 4 x 64 x 64 against 2^10 and 2^20 records with 32-byte messages, at unit levels (sign rows, Q = 5, 7, 9 planes) and at
15 levels (level_pack's rows, Q = 8 and 10 planes; 256 images are beyond the 68 a set holds at 15 levels and are reported as refused).  Every shape is warmed up
first, then --reps rounds alternate one timed window per variant (device events around back-to-back C ABI calls, a device synchronise at the end of every
window); reported is the median [min .. max] over the rounds.  Before timing, the pooled scores are compared with the sums of the per-image scores at 8 records.
Nothing is gated on a time.

usage: python tools/trace_pool_bench.py [--reps 5] [--window-ms 30] [--json FILE] [--quick]
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
from gswm_amd import _native as N, codec, soft  # noqa: E402

MSG_BYTES = 32
SHAPE = (4, 64, 64)
SETS = (16, 64, 256)
LEVELS = (0, 15)                                    # 0: unit levels


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
    assert torch.cuda.is_available(), "trace_pool_bench needs the GPU (there is no CPU path to time)"
    lib, dev = N.lib(), torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    Us = (1 << 10, 1 << 16) if a.quick else (1 << 10, 1 << 20)
    reps = 2 if a.quick else a.reps
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]
    stride = codec.keyed_record_stride(MSG_BYTES)
    records_all = torch.randint(0, 256, (max(Us), stride), dtype=torch.uint8, device=dev, generator=g)
    z = torch.randn(max(SETS), *SHAPE, device=dev, generator=g).half().contiguous()
    st = codec._stream_ptr()
    signs, _ = codec.sign_pack(z)
    level_rows = codec.level_pack(z, soft.uniform_thresholds(z, 15))

    # the identity, before timing: pooled scores are the sums of the per-image scores (8 records, k = 8: every record is reported)
    few = records_all[:8]
    for levels, size in ((0, 64), (15, 64)):
        if levels:
            rows = codec.LevelRows(*(t[:size] for t in level_rows))
            idx1, s1 = codec.trace_keyed_soft_topk(rows, n, few, MSG_BYTES, k=8)
            pooled = codec.pool_rows(rows.signs, rows.planes, [size])
        else:
            idx1, s1 = codec.trace_keyed_topk(signs[:size], n, few, MSG_BYTES, k=8)
            pooled = codec.pool_rows(signs[:size], None, [size])
        idx, s = codec.trace_keyed_pooled_topk(pooled, n, few, MSG_BYTES, k=8)
        per_image = torch.zeros(size, 8, dtype=torch.int64, device=dev).scatter_(1, idx1.long(), s1.long()).sum(dim=0)
        assert torch.equal(torch.zeros(8, dtype=torch.int64, device=dev).scatter_(0, idx[0].long(), s[0].long()), per_image), "pooled scores are not the sums"

    rows_out = []
    from bench_board import BoardSampler
    with BoardSampler(0) as board:
        for levels in LEVELS:
            P = 4 if levels else 0
            for size in SETS:
                if levels and size > 1023 // 15:
                    rows_out.append({"levels": levels, "set": size, "refused": f"a set holds at most {1023 // 15} images at 15 levels"})
                    continue
                s_in = (level_rows.signs if levels else signs)[:size].contiguous()
                p_in = level_rows.planes[:size].contiguous() if levels else None
                w_in = level_rows.wsum[:size].contiguous() if levels else None
                Q = codec.pool_planes(P, size)
                ptr = torch.tensor([0, size], dtype=torch.int32, device=dev)
                pooled = codec.PooledRows(torch.empty((1, n // 8), dtype=torch.uint8, device=dev), torch.empty((1, Q, n // 8), dtype=torch.uint8, device=dev),
                                          torch.empty(1, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int64, device=dev))

                def pool():
                    return lib.gsw_pool_rows(s_in.data_ptr(), p_in.data_ptr() if levels else None, P, size, n, ptr.data_ptr(), 1, size, Q, pooled.signs.data_ptr(),
                                             pooled.planes.data_ptr(), pooled.wsum.data_ptr(), pooled.wsq.data_ptr(), st)

                assert pool() == N.GSW_OK
                for U in Us:
                    recs = records_all[:U]
                    idx1, score1 = torch.empty((size, 1), dtype=torch.int32, device=dev), torch.empty((size, 1), dtype=torch.int32, device=dev)
                    idxg, scoreg = torch.empty((1, 1), dtype=torch.int32, device=dev), torch.empty((1, 1), dtype=torch.int32, device=dev)
                    ws1 = torch.empty(lib.gsw_trace_keyed_workspace_bytes(size, U, 1) // 8, dtype=torch.int64, device=dev)
                    wsg = torch.empty(lib.gsw_trace_keyed_workspace_bytes(1, U, 1) // 8, dtype=torch.int64, device=dev)

                    def search():
                        return lib.gsw_trace_keyed_pooled_topk(pooled.signs.data_ptr(), pooled.planes.data_ptr(), pooled.wsum.data_ptr(), Q, 1, n, recs.data_ptr(), stride,
                                                               MSG_BYTES, U, 1, idxg.data_ptr(), scoreg.data_ptr(), wsg.data_ptr(), st)

                    def both():
                        pool()
                        return search()

                    if levels:
                        def per_image():
                            return lib.gsw_trace_keyed_soft_topk(s_in.data_ptr(), p_in.data_ptr(), w_in.data_ptr(), levels, size, n, recs.data_ptr(), stride, MSG_BYTES, U, 1,
                                                                 idx1.data_ptr(), score1.data_ptr(), ws1.data_ptr(), st)
                    else:
                        def per_image():
                            return lib.gsw_trace_keyed_topk(s_in.data_ptr(), size, n, recs.data_ptr(), stride, MSG_BYTES, U, 1, idx1.data_ptr(), score1.data_ptr(),
                                                            ws1.data_ptr(), st)

                    fns = {"pool_rows": pool, "pooled search": search, "pool + search": both, "per image": per_image}
                    assert search() == N.GSW_OK and per_image() == N.GSW_OK
                    iters = {name: calibrate(f, a.window_ms) for name, f in fns.items()}
                    t = {name: [] for name in fns}
                    for _ in range(reps):                                       # alternate the variants inside every round
                        for name, f in fns.items():
                            t[name].append(window(f, iters[name]))
                    row = {"levels": levels, "set": size, "Q": Q, "U": U, "iters": iters}
                    for name in fns:
                        row[name] = stat(t[name])
                    row["per image over pooled"] = row["per image"]["median_us"] / row["pool + search"]["median_us"]
                    rows_out.append(row)
                    del ws1, wsg
    f = lambda d: f"{d['median_us']:9.1f} [{d['min_us']:.1f} .. {d['max_us']:.1f}]"
    print(f"one set of images of {SHAPE[0]} x {SHAPE[1]} x {SHAPE[2]} (fp16), {MSG_BYTES}-byte messages, k = 1; median [min .. max] us per C ABI call over {reps} alternating "
          f"rounds of ~{a.window_ms:.0f} ms windows; device: {torch.cuda.get_device_name(0)}; board: {json.dumps(board.summary())}")
    print(f"{'levels':>6s} {'set':>4s} {'Q':>2s} {'U':>8s} {'pool_rows us':>28s} {'pooled search us':>30s} {'pool + search us':>30s} {'per-image search us':>32s} {'/ pooled':>8s}")
    for r in rows_out:
        if "refused" in r:
            print(f"{r['levels'] or 'unit':>6} {r['set']:4d} refused before a launch: {r['refused']}")
            continue
        print(f"{r['levels'] or 'unit':>6} {r['set']:4d} {r['Q']:2d} {r['U']:8d} {f(r['pool_rows']):>28s} {f(r['pooled search']):>30s} {f(r['pool + search']):>30s} "
              f"{f(r['per image']):>32s} {r['per image over pooled']:8.2f}")
    print("per image: gsw_trace_keyed_topk (unit) / gsw_trace_keyed_soft_topk (15 levels) in one launch over the set's images -- every image scored alone, which is "
          "what a caller runs today and does not answer the set's question.  The pooled scores equal the sums of the per-image scores (64 images, 8 records, both level counts).")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"msg_bytes": MSG_BYTES, "rows": rows_out, "board": board.summary()}, fh, indent=1)


if __name__ == "__main__":
    main()
