"""Microbenchmark of the registry search (codec.trace_topk -> gsw_trace_topk, csrc/gswm_trace.hip) against the plain-torch formulation
timed in the same process: unpack the packed registry to +-1 floats, one matrix product against the weight rows, `topk`, chunked over
the users so that the unpacked chunk and its score block fit (fp32: every product and partial sum is an integer below 2^24, so the
baseline is exact too and the two results can be compared for equality).

Per case (M = 256, V = 64; B x U x soft / hard): every shape is warmed up first, then --reps rounds alternate a timed window of the
kernel and a timed window of the baseline (device events around back-to-back calls; the number of calls per window is chosen so that a
window lasts about --window-ms).  Reported: median / min / max over the rounds of both, the kernel's registry bytes over its median
time, the ratio of the medians, and whether the kernel's slowest round beats the baseline's fastest.  Before timing, the two results
are compared at the timed size: scores must be equal, indices equal wherever the row's k+1 best scores are distinct (torch.topk does
not promise an order among equal scores; the kernel's tie rule is checked by the tests).  The board's clock is sampled during the run.

`abi` times gsw_trace_topk alone with a preallocated workspace (what a caller that keeps its buffers pays); `call` is codec.trace_topk
as a Python call (three small allocations included).

usage: python tools/trace_bench.py [--reps 5] [--window-ms 30] [--k 4] [--json FILE] [--quick]
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

M, V = 256, 64
CHUNK = 1 << 20          # users per baseline chunk: 1 GiB of unpacked fp32 + a [B, CHUNK] score block


def torch_topk(counts, registry, k, soft):
    """the plain-torch formulation; returns (idx int64 [B, k], score fp32 [B, k])"""
    c = counts.float()
    w = (2.0 * c - V) if soft else torch.where(2 * counts > V, 1.0, -1.0)
    shifts = torch.arange(7, -1, -1, device=registry.device, dtype=torch.uint8)
    best_s = best_i = None
    for u0 in range(0, registry.shape[0], CHUNK):
        r = registry[u0:u0 + CHUNK]
        pm = ((r.unsqueeze(-1) >> shifts) & 1).reshape(r.shape[0], -1).float().mul_(2.0).sub_(1.0)       # [Uc, M] of +-1
        s = w @ pm.t()                                                                               # [B, Uc]
        ts, ti = torch.topk(s, min(k, s.shape[1]), dim=1)
        ti = ti + u0
        if best_s is not None:
            cs, ci = torch.cat([best_s, ts], 1), torch.cat([best_i, ti], 1)
            ts, sel = torch.topk(cs, min(k, cs.shape[1]), dim=1)
            ti = torch.gather(ci, 1, sel)
        best_s, best_i = ts, ti
    return best_i, best_s


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3          # us per call


def calibrate(fn, window_ms):
    for _ in range(3):                              # warm-up of this shape
        fn()
    torch.cuda.synchronize()
    t = window(fn, 3)
    return max(3, min(5000, int(window_ms * 1e3 / max(t, 1.0))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--json", default=None)
    ap.add_argument("--quick", action="store_true", help="U up to 2^20 only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "trace_bench needs the GPU (there is no CPU path to time)"
    lib, dev = N.lib(), torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    Us = (1 << 16, 1 << 20) if a.quick else (1 << 16, 1 << 20, 1 << 24)
    registry_all = torch.randint(0, 256, (max(Us), M // 8), dtype=torch.uint8, device=dev, generator=g)
    rows = []
    from bench_board import BoardSampler
    with BoardSampler(0) as board:
        for U in Us:
            registry = registry_all[:U]
            for B in (1, 8, 64):
                counts = torch.randint(0, V + 1, (B, M), dtype=torch.int32, device=dev, generator=g)
                for soft in (True, False):
                    k = a.k
                    idx, score = codec.trace_topk(counts, V, registry, k=k, soft=soft)
                    ti, ts = torch_topk(counts, registry, k + 1, soft)
                    same_score = bool(torch.equal(score.float(), ts[:, :k]))
                    distinct = (ts[:, :-1] != ts[:, 1:]).all(dim=1)                       # rows whose k+1 best scores are all different
                    same_idx = bool(torch.equal(idx[distinct].long(), ti[distinct][:, :k]))
                    assert same_score and same_idx, (U, B, soft, "the kernel and the torch formulation disagree")

                    ws = torch.empty(lib.gsw_trace_workspace_bytes(B, U, k) // 8, dtype=torch.int64, device=dev)
                    st, mode = codec._stream_ptr(), (N.GSW_TRACE_SOFT if soft else N.GSW_TRACE_HARD)
                    fns = {"abi": lambda: lib.gsw_trace_topk(counts.data_ptr(), B, M, V, mode, registry.data_ptr(), U, k, idx.data_ptr(), score.data_ptr(), ws.data_ptr(), st),
                           "call": lambda: codec.trace_topk(counts, V, registry, k=k, soft=soft),
                           "torch": lambda: torch_topk(counts, registry, k, soft)}
                    iters = {n: calibrate(f, a.window_ms) for n, f in fns.items()}
                    t = {n: [] for n in fns}
                    for _ in range(a.reps):                                                # alternate the versions inside every round
                        for n, f in fns.items():
                            t[n].append(window(f, iters[n]))
                    row = {"U": U, "B": B, "mode": "soft" if soft else "hard", "k": k, "rows_with_distinct_scores": int(distinct.sum()), "iters": iters}
                    for n in fns:
                        row[n] = {"median_us": statistics.median(t[n]), "min_us": min(t[n]), "max_us": max(t[n])}
                    row["registry_GBps"] = U * (M // 8) / row["abi"]["median_us"] / 1e3
                    row["torch_over_call"] = row["torch"]["median_us"] / row["call"]["median_us"]
                    row["faster_beyond_spread"] = row["call"]["max_us"] < row["torch"]["min_us"]
                    rows.append(row)
                    del ws
    print(f"M = {M}, V = {V}, k = {a.k}; median [min .. max] us per call over {a.reps} alternating rounds of ~{a.window_ms:.0f} ms windows; device: "
          f"{torch.cuda.get_device_name(0)}; board: {json.dumps(board.summary())}")
    print(f"{'U':>9s} {'B':>3s} {'mode':4s} {'abi us':>26s} {'call us':>26s} {'torch us':>30s} {'registry GB/s':>13s} {'torch/call':>10s} {'beyond spread':>13s}")
    for r in rows:
        f = lambda d: f"{d['median_us']:9.1f} [{d['min_us']:.1f} .. {d['max_us']:.1f}]"
        print(f"{r['U']:9d} {r['B']:3d} {r['mode']:4s} {f(r['abi']):>26s} {f(r['call']):>26s} {f(r['torch']):>30s} {r['registry_GBps']:13.0f} {r['torch_over_call']:10.1f} "
              f"{'yes' if r['faster_beyond_spread'] else 'NO':>13s}")
    print("results equal at every timed size (scores exactly; indices wherever the leading scores are distinct)")
    print("the kernel is faster than the torch formulation beyond the spread in every case" if all(r["faster_beyond_spread"] for r in rows)
          else "the kernel is NOT faster beyond the spread in every case")
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"M": M, "V": V, "rows": rows, "board": board.summary()}, fh, indent=1)


if __name__ == "__main__":
    main()
