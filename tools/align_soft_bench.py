"""Microbenchmark of the alignment search ranked by reliability levels (codec.level_rows_align, align.search_keys_soft; csrc/gswm_align_soft.inc)
against what a caller had before it, timed in the same process.

(a) The launch alone (gsw_level_rows_align: the sign row and its P planes, one index walk) against the composition of the same bytes from
    `codec.rows_align`: 1 + P launches (the sign rows, then every plane's rows, the planes made contiguous OUTSIDE the timed window) plus the
    permuting copy of the planes from [B, P, A, ...] to [B, A, P, ...].  Also shown: the same composition with the P planes in ONE launch on
    [B P] rows (2 launches + the copy).
(b) The whole `align.search_keys_soft` (level_pack + level_rows_align + key_search_soft_topk + the merge per image) against 1 key and 1024 keys,
    next to the torch composition a caller has without the kernel -- `align.apply` on the float latents for every candidate, one `level_pack`
    with the un-aligned thresholds repeated, one `key_search_soft_topk`, NO merge, which favours it -- and next to `align.search_keys` (the sign
    search through the same candidates) for the price of the levels.

Cases: 64 images of 4 x 64 x 64 fp16, 256-bit messages; P in {1, 2, 4} planes (1, 3, 15 levels); A in {8, 200, 648} candidates (d4 with shifts
0, 2, 4).  Every shape is warmed up first, then --reps rounds alternate the timed windows of the variants (device events around back-to-back
calls, a device synchronise at the end of every window).  Before timing, the routes are compared bit for bit.

Reported: median [min .. max] us per call over the rounds, and whether the fused launch is slower than the composition beyond the spread (its
fastest round against the composition's slowest).  No time is promised in advance.

usage: python tools/align_soft_bench.py [--reps 5] [--window-ms 30] [--out profiles/align_soft_bench.txt] [--json FILE] [--quick]
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
from gswm_amd import align as AL, codec, soft  # noqa: E402

B, SHAPE, MB = 64, (4, 64, 64), 32
SHIFTS = {8: 0, 200: 2, 648: 4}
LEVELS = {1: 1, 2: 3, 4: 15}            # planes -> levels


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


def measure(fns, reps, window_ms):
    iters = {name: calibrate(f, window_ms) for name, f in fns.items()}
    t = {name: [] for name in fns}
    for _ in range(reps):                           # alternate the variants inside every round
        for name, f in fns.items():
            t[name].append(window(f, iters[name]))
    return {name: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "iters": iters[name]} for name, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_soft_bench.txt"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--quick", action="store_true", help="two rounds")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "align_soft_bench needs the GPU (there is no CPU path to time)"
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    reps = 2 if a.quick else a.reps
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]
    rb = n // 8
    keys_all = torch.randint(0, 256, (1024, 48), dtype=torch.uint8, device=dev, generator=g)
    z = torch.randn(B, *SHAPE, device=dev, generator=g).half()
    owner = keys_all[341].cpu().numpy()
    z[0] = AL.apply(codec.embed_batch(owner[:32].tobytes(), owner[32:].tobytes(), bytes(range(MB)), 1, SHAPE, seed=1).half()[0], (5, 1, -2))   # one attacked image
    launch_rows, search_rows = [], []
    from bench_board import BoardSampler
    with BoardSampler(0) as board:
        for P, levels in LEVELS.items():
            thr = soft.uniform_thresholds(z, levels)
            rows = codec.level_pack(z, thr)
            assert rows.planes.shape[1] == P
            planes_each = [rows.planes[:, q].contiguous() for q in range(P)]                # outside every timed window
            planes_flat = rows.planes.view(B * P, rb)
            for A, shift in SHIFTS.items():
                aligns = AL.alignments("d4", shift, SHAPE[1], SHAPE[2])
                assert len(aligns) == A
                table = torch.from_numpy(codec.align_table(aligns, SHAPE)).to(dev)

                def fused_launch():
                    return codec._level_rows_align_launch(rows, SHAPE, table)

                def composed_launches():                                                    # 1 + P launches and the permuting copy
                    s = codec._rows_align_launch(rows.signs, SHAPE, 1, table)
                    return s, torch.stack([codec._rows_align_launch(pl, SHAPE, 1, table) for pl in planes_each], dim=2)

                def composed_two():                                                         # the planes as [B P] rows: 2 launches and the permuting copy
                    s = codec._rows_align_launch(rows.signs, SHAPE, 1, table)
                    return s, codec._rows_align_launch(planes_flat, SHAPE, 1, table).view(B, P, A, rb).transpose(1, 2).contiguous()

                fs, fp = fused_launch()
                for other in (composed_launches(), composed_two()):
                    assert torch.equal(fs, other[0]) and torch.equal(fp, other[1]), "level_rows_align and the rows_align composition disagree"
                del other
                r = measure({"fused": fused_launch, "composed": composed_launches, "composed2": composed_two}, reps, a.window_ms)
                r.update(P=P, A=A, written=B * A * (1 + P) * rb)
                r["composed_over_fused"] = r["composed"]["median_us"] / r["fused"]["median_us"]
                r["slower_beyond_spread"] = r["fused"]["min_us"] > r["composed"]["max_us"]
                launch_rows.append(r)
                del fs, fp

                thr_rep = thr.repeat_interleave(A, dim=0)

                def torch_rows():
                    t = torch.stack([AL.apply(z, al) for al in aligns], dim=1)             # [B, A, C, H, W]: what a caller builds without the kernel
                    return codec.level_pack(t.view(B * A, *SHAPE), thr_rep)

                tr = torch_rows()
                fr = codec.level_rows_align(rows, SHAPE, table)
                assert torch.equal(fr.signs, tr.signs) and torch.equal(fr.planes, tr.planes), "level_rows_align and level_pack of the aligned latents disagree"
                del tr, fr
                for K in (1, 1024):
                    keys = keys_all[341:342].contiguous() if K == 1 else keys_all

                    def fused():
                        return AL.search_keys_soft(z, keys, MB, aligns, thresholds=thr, k=1)

                    def composed():
                        return codec.key_search_soft_topk(torch_rows(), n, keys, MB, k=1)

                    def signs_only():
                        return AL.search_keys(z, keys, MB, aligns, k=1)

                    ki, ai, st = fused()
                    idx, stat = composed()
                    assert torch.equal(st[:, 0], stat.view(B, A).max(dim=1).values), "the fused search and the torch composition disagree"
                    if shift >= 2:                                                          # the attacked image: its key, and the alignment that undoes the attack
                        assert int(ki[0, 0]) == (0 if K == 1 else 341) and aligns[int(ai[0, 0])] == AL.inverse((5, 1, -2), SHAPE[1], SHAPE[2])
                    r = measure({"search_keys_soft": fused, "torch": composed, "search_keys": signs_only}, reps, a.window_ms)
                    r.update(P=P, A=A, K=K)
                    r["torch_over_fused"] = r["torch"]["median_us"] / r["search_keys_soft"]["median_us"]
                    r["soft_over_signs"] = r["search_keys_soft"]["median_us"] / r["search_keys"]["median_us"]
                    search_rows.append(r)
    out = io.StringIO()
    p = lambda *x: print(*x, file=out)
    f = lambda d: f"{d['median_us']:10.1f} [{d['min_us']:.1f} .. {d['max_us']:.1f}]"
    p(f"{B} images of {' x '.join(map(str, SHAPE))} fp16 ({n} bits, l = 1), {8 * MB}-bit messages, k = 1; median [min .. max] us per call over {reps} alternating rounds of "
      f"~{a.window_ms:.0f} ms windows; device: {torch.cuda.get_device_name(0)}; board: {json.dumps(board.summary())}")
    p("(a) fused = gsw_level_rows_align alone; composed = 1 + P launches of gsw_rows_align (planes contiguous beforehand) + the permuting copy of the planes; "
      "composed2 = 2 launches (the planes as [B P] rows) + the copy")
    p(f"{'P':>2s} {'A':>5s} {'fused us':>32s} {'written GB/s':>13s} {'composed us':>34s} {'composed2 us':>34s} {'composed/fused':>15s}")
    for r in launch_rows:
        p(f"{r['P']:2d} {r['A']:5d} {f(r['fused']):>32s} {r['written'] / r['fused']['median_us'] * 1e6 / 1e9:13.1f} {f(r['composed']):>34s} {f(r['composed2']):>34s} {r['composed_over_fused']:15.2f}")
    lost = [(r["P"], r["A"]) for r in launch_rows if r["slower_beyond_spread"]]
    p("the fused launch is not slower than the 1 + P launch composition beyond the spread at any measured point" if not lost
      else f"the fused launch IS SLOWER than the 1 + P launch composition beyond the spread at (P, A) = {lost}")
    p("(b) search_keys_soft = level_pack + level_rows_align + key_search_soft_topk + the merge per image; torch = A float latents per image by flip / rot90 / roll, one "
      "level_pack, one key_search_soft_topk on the same B A rows, NO merge; search_keys = the sign search through the same candidates")
    p(f"{'P':>2s} {'A':>5s} {'keys':>6s} {'search_keys_soft us':>34s} {'torch us':>36s} {'search_keys us':>34s} {'torch/fused':>12s} {'soft/signs':>11s}")
    for r in search_rows:
        p(f"{r['P']:2d} {r['A']:5d} {r['K']:6d} {f(r['search_keys_soft']):>34s} {f(r['torch']):>36s} {f(r['search_keys']):>34s} {r['torch_over_fused']:12.1f} {r['soft_over_signs']:11.2f}")
    p("level_rows_align's rows equal both compositions and level_pack of the aligned latents bit for bit, and both search routes give every image the same best "
      "statistic, at every timed shape")
    print(out.getvalue(), end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(out.getvalue())
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"launch": launch_rows, "search": search_rows, "board": board.summary()}, fh, indent=1)


if __name__ == "__main__":
    main()
