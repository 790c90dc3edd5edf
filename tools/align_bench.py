"""Microbenchmark of the alignment search (align.search_keys: codec.quant_pack -> codec.rows_align -> codec.key_search_topk -> a merge on the
device; csrc/gswm_align.inc) against the only form a caller had before it, timed in the same process: every candidate alignment of the FLOAT
latents built with the three torch ops of `align.apply` (flip, rot90, roll), all of them quantised by one `codec.quant_pack` and searched by one
`codec.key_search_topk` -- the same search launch on the same number of rows.  The composition is timed WITHOUT the merge per image, which
favours it.

Cases: 64 images of 4 x 64 x 64 fp16, l = 1, 32-byte messages; A in {8, 200, 648} candidates (d4 with shifts 0, 2, 4), K in {1, 1024} keys.
Every shape is warmed up first, then --reps rounds alternate a timed window of `rows_align` alone, of the whole `search_keys` and of the torch
composition (device events around back-to-back calls, a device synchronise at the end of every window).  Before timing, the two routes are compared:
the rows must be equal bit for bit and the best key, alignment and statistic of every image must agree.

Reported: median [min .. max] us per call over the rounds, the bytes `rows_align` writes per second, and whether the fused form is faster than
the composition beyond the spread (its slowest round against the composition's fastest).  No ratio is promised in advance.

usage: python tools/align_bench.py [--reps 5] [--window-ms 30] [--out profiles/align_bench.txt] [--json FILE] [--quick]
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
from gswm_amd import align as AL, codec  # noqa: E402

B, SHAPE, MB = 64, (4, 64, 64), 32
SHIFTS = {8: 0, 200: 2, 648: 4}


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.txt"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--quick", action="store_true", help="two rounds")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "align_bench needs the GPU (there is no CPU path to time)"
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    reps = 2 if a.quick else a.reps
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]
    keys_all = torch.randint(0, 256, (1024, 48), dtype=torch.uint8, device=dev, generator=g)
    z = torch.randn(B, *SHAPE, device=dev, generator=g).half()
    owner = keys_all[341].cpu().numpy()
    z[0] = AL.apply(codec.embed_batch(owner[:32].tobytes(), owner[32:].tobytes(), bytes(range(MB)), 1, SHAPE, seed=1).half()[0], (5, 1, -2))   # one attacked image
    packed, _ = codec.quant_pack(z, 1)
    rows_out = []
    from bench_board import BoardSampler
    with BoardSampler(0) as board:
        for A, shift in SHIFTS.items():
            aligns = AL.alignments("d4", shift, SHAPE[1], SHAPE[2])
            assert len(aligns) == A
            table = torch.from_numpy(codec.align_table(aligns, SHAPE)).to(dev)

            def compose_rows():
                t = torch.stack([AL.apply(z, al) for al in aligns], dim=1)             # [B, A, C, H, W]: what a caller builds without the kernel
                return codec.quant_pack(t.view(B * A, *SHAPE), 1)[0]

            fused_rows = codec.rows_align(packed, SHAPE, 1, table)
            assert torch.equal(fused_rows.view(B * A, -1), compose_rows()), "rows_align and the torch composition disagree"
            align_fn = lambda: codec._rows_align_launch(packed, SHAPE, 1, table)
            written = B * A * (n // 8)
            for K in (1, 1024):
                keys = keys_all[341:342].contiguous() if K == 1 else keys_all

                def fused():
                    return AL.search_keys(z, keys, MB, aligns, k=1)

                def composed():
                    return codec.key_search_topk(compose_rows(), n, keys, MB, k=1)

                ki, ai, st = fused()
                idx, stat = composed()
                stat = stat.view(B, A)
                assert torch.equal(st[:, 0], stat.max(dim=1).values), "the fused search and the torch composition disagree"
                if shift >= 2:                                                          # the attacked image: its key, and the alignment that undoes the attack
                    assert int(ki[0, 0]) == (0 if K == 1 else 341) and aligns[int(ai[0, 0])] == AL.inverse((5, 1, -2), SHAPE[1], SHAPE[2])
                fns = {"rows_align": align_fn, "search_keys": fused, "torch": composed}
                iters = {name: calibrate(f, a.window_ms) for name, f in fns.items()}
                t = {name: [] for name in fns}
                for _ in range(reps):                                                   # alternate the versions inside every round
                    for name, f in fns.items():
                        t[name].append(window(f, iters[name]))
                row = {"A": A, "K": K, "B": B, "n": n, "iters": iters}
                for name in fns:
                    row[name] = {"median_us": statistics.median(t[name]), "min_us": min(t[name]), "max_us": max(t[name])}
                row["rows_align_bytes_per_s"] = written / row["rows_align"]["median_us"] * 1e6
                row["torch_over_fused"] = row["torch"]["median_us"] / row["search_keys"]["median_us"]
                row["faster_beyond_spread"] = row["search_keys"]["max_us"] < row["torch"]["min_us"]
                rows_out.append(row)
    out = io.StringIO()
    p = lambda *x: print(*x, file=out)
    p(f"{B} images of {' x '.join(map(str, SHAPE))} fp16 ({n} bits, l = 1), {8 * MB}-bit messages, k = 1; median [min .. max] us per call over {reps} alternating rounds of "
      f"~{a.window_ms:.0f} ms windows; device: {torch.cuda.get_device_name(0)}; board: {json.dumps(board.summary())}")
    p("rows_align = the launch alone (gsw_rows_align); search_keys = quant_pack + rows_align + key_search_topk + the merge per image; torch = A float latents per image by "
      "flip / rot90 / roll, one quant_pack, one key_search_topk on the same B A rows, NO merge")
    p(f"{'A':>5s} {'keys':>6s} {'rows_align us':>30s} {'written GB/s':>13s} {'search_keys us':>32s} {'torch us':>36s} {'torch/fused':>12s}")
    for r in rows_out:
        f = lambda d: f"{d['median_us']:10.1f} [{d['min_us']:.1f} .. {d['max_us']:.1f}]"
        p(f"{r['A']:5d} {r['K']:6d} {f(r['rows_align']):>30s} {r['rows_align_bytes_per_s'] / 1e9:13.1f} {f(r['search_keys']):>32s} {f(r['torch']):>36s} {r['torch_over_fused']:12.1f}")
    p("rows_align's rows equal the quantised torch composition bit for bit, and both routes give every image the same best statistic, at every timed shape")
    lost = [(r["A"], r["K"]) for r in rows_out if not r["faster_beyond_spread"]]
    p("the fused form is faster than the torch composition beyond the spread at every measured point" if not lost
      else f"the fused form is NOT faster than the torch composition beyond the spread at (A, keys) = {lost}")
    print(out.getvalue(), end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(out.getvalue())
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"rows": rows_out, "board": board.summary()}, fh, indent=1)


if __name__ == "__main__":
    main()
