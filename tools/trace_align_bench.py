"""Microbenchmark of the aligned registry search (trace.trace_latents_aligned: codec.quant_pack -> codec.counts_align -> codec.trace_topk -> a merge on
the device; csrc/gswm_counts_align.inc) against the two forms a caller had before it, timed in the same process:

  (a) codec.rows_align, then codec.vote_tiled with unit weights on the B A aligned rows (counts = (score + copies) / 2), then codec.trace_topk;
  (b) every candidate alignment of the FLOAT latents built with the three torch ops of `align.apply`, one codec.extract_batch(return_counts=True)
      on the B A latents, then codec.trace_topk.

Both are timed WITHOUT the merge per image, which favours them.  The keyed pair (trace.trace_latents_keyed_aligned) is the composition
rows_align -> trace_keyed_topk -> merge; it is timed beside (b'), the torch alignments quantised by one codec.quant_pack and searched by the same
codec.trace_keyed_topk, at 2^10 records only (a keyed search generates every record's keystream for every row).

Cases: 64 images of 4 x 64 x 64 fp16, l = 1, 256-bit messages; A in {8, 200, 648} candidates (d4 with shifts 0, 2, 4); registries of 2^10 and 2^20 rows.
Every shape is warmed up first, then --reps rounds alternate a timed window of every form (device events around back-to-back calls, a device
synchronise at the end of every window).  Before timing, the forms are compared: the counts must be equal bit for bit.

Reported: median [min .. max] us per call over the rounds, and whether the fused form is faster than (a) and (b) beyond the spread (its slowest round
against the other's fastest).  `whole` is trace_latents_aligned as a caller sees it, host statistics included (one call per window).  No ratio is
promised in advance.

usage: python tools/trace_align_bench.py [--reps 5] [--window-ms 30] [--out profiles/trace_align_bench.txt] [--json FILE] [--quick]
"""
import argparse
import io
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gswm_amd  # noqa: E402,F401
from gswm_amd import align as AL, codec, trace as T  # noqa: E402

B, SHAPE, MB = 64, (4, 64, 64), 32
SHIFTS = {8: 0, 200: 2, 648: 4}
ATTACK = (5, 1, -2)
KEYED_B = "(b')"


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
    """`whole` is seconds of host statistics per call (an exact binomial tail per image): one call per window, warmed up by the caller's own first call"""
    iters = {name: 1 if name == "whole" else calibrate(f, window_ms) for name, f in fns.items()}
    t = {name: [] for name in fns}
    for _ in range(reps):                           # alternate the forms inside every round
        for name, f in fns.items():
            t[name].append(window(f, iters[name]))
    return {name: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "iters": iters[name]} for name, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_align_bench.txt"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--quick", action="store_true", help="two rounds, the small registry only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "trace_align_bench needs the GPU (there is no CPU path to time)"
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    reps = 2 if a.quick else a.reps
    M, n = 8 * MB, SHAPE[0] * SHAPE[1] * SHAPE[2]
    V = n // M
    rng = np.random.default_rng(0)
    key, nonce = bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8))
    sizes = (1 << 10,) if a.quick else (1 << 10, 1 << 20)
    msgs = rng.integers(0, 256, (max(sizes), MB), dtype=np.uint8)
    regs = {}
    for U in sizes:
        reg = T.Registry(MB)
        for u in range(U):
            reg.add(f"u{u}", msgs[u].tobytes())
        regs[U] = reg
    kreg = T.KeyedRegistry(MB)
    for u in range(1 << 10):
        kreg.add(f"u{u}", key if u == 341 else bytes(rng.integers(0, 256, 32, dtype=np.uint8)), nonce, msgs[u].tobytes())
    z = torch.randn(B, *SHAPE, device=dev, generator=g).half()
    z[0] = AL.apply(codec.embed_batch(key, nonce, msgs[341].tobytes(), 1, SHAPE, seed=1).half()[0], ATTACK)   # one attacked image of user 341
    packed, _ = codec.quant_pack(z, 1)
    key_row = torch.from_numpy(np.frombuffer(key + nonce, dtype=np.uint8).copy()).to(dev)
    rows_out, keyed_out = [], []
    from bench_board import BoardSampler
    with BoardSampler(0) as board:
        for A, shift in SHIFTS.items():
            aligns = AL.alignments("d4", shift, SHAPE[1], SHAPE[2])
            assert len(aligns) == A
            table = torch.from_numpy(codec.align_table(aligns, SHAPE)).to(dev)
            keys_ba = key_row.expand(B * A, 48).contiguous()
            ones = torch.ones((B * A, SHAPE[1] // 8, SHAPE[2] // 8), dtype=torch.uint16, device=dev)

            def counts_fused():
                return codec._counts_align_launch(packed, SHAPE, 1, table, key, nonce, M)

            def counts_a():
                rows = codec._rows_align_launch(packed, SHAPE, 1, table)
                score = codec.vote_tiled(rows.view(B * A, -1), keys_ba, ones, M, SHAPE, 1, 8)[1]
                return (score + V) >> 1

            def counts_b():
                t = torch.stack([AL.apply(z, al) for al in aligns], dim=1)             # [B, A, C, H, W]: what a caller builds without any kernel
                return codec.extract_batch(t.view(B * A, *SHAPE), key, nonce, M, return_counts=True)[2]

            want = counts_fused().view(B * A, M)
            assert torch.equal(want, counts_a()) and torch.equal(want, counts_b()), "the three forms disagree on the counts"
            row = {"A": A, "B": B, "n": n, "counts": measure({"counts_align": counts_fused, "rows_align+vote_tiled": counts_a, "torch+extract_batch": counts_b}, reps, a.window_ms)}
            for U, reg in regs.items():
                reg_dev = reg.to_device(dev)

                def fused():
                    idx, score = codec.trace_topk(counts_fused().view(B * A, M), V, reg_dev, k=1)
                    return AL._merge_best(idx.view(B, A), score.view(B, A), U, stat_bits=T.ALIGNED_STAT_BITS)

                def form_a():
                    return codec.trace_topk(counts_a(), V, reg_dev, k=1)

                def form_b():
                    return codec.trace_topk(counts_b(), V, reg_dev, k=1)

                def whole():
                    return T.trace_latents_aligned(z, key, nonce, reg, aligns)

                res = whole()
                if shift >= 2:                                                          # the attacked image: its user, and the alignment that undoes the attack
                    assert res[0].attributed == "u341" and res[0].alignment == AL.inverse(ATTACK, SHAPE[1], SHAPE[2])
                ki, ai, st = fused()
                assert torch.equal(st[:, 0], form_a()[1].view(B, A).max(dim=1).values) and int(st[0, 0]) == res[0].candidates[0].score
                row[f"U{U}"] = measure({"search": fused, "(a)": form_a, "(b)": form_b, "whole": whole}, reps, a.window_ms)
                print(f"[trace_align_bench] A = {A}, U = {U} done", file=sys.stderr, flush=True)
            rows_out.append(row)
            # ---- the keyed pair, 2^10 records
            rec_dev = kreg.to_device(dev)

            def keyed_fused():
                rows = codec._rows_align_launch(packed, SHAPE, 1, table)
                idx, score = codec.trace_keyed_topk(rows.view(B * A, -1), n, rec_dev, MB, k=1)
                return AL._merge_best(idx.view(B, A), score.view(B, A), len(kreg), stat_bits=T.ALIGNED_STAT_BITS)

            def keyed_b():
                t = torch.stack([AL.apply(z, al) for al in aligns], dim=1)
                return codec.trace_keyed_topk(codec.quant_pack(t.view(B * A, *SHAPE), 1)[0], n, rec_dev, MB, k=1)

            def keyed_whole():
                return T.trace_latents_keyed_aligned(z, kreg, aligns)

            res = keyed_whole()
            if shift >= 2:
                assert res[0].attributed == "u341" and res[0].alignment == AL.inverse(ATTACK, SHAPE[1], SHAPE[2])
            assert torch.equal(keyed_fused()[2][:, 0], keyed_b()[1].view(B, A).max(dim=1).values)
            keyed_out.append({"A": A, **measure({"search": keyed_fused, KEYED_B: keyed_b, "whole": keyed_whole}, reps, a.window_ms)})
    out = io.StringIO()
    p = lambda *x: print(*x, file=out)
    f = lambda d: f"{d['median_us']:.1f} [{d['min_us']:.1f} .. {d['max_us']:.1f}]"
    p(f"{B} images of {' x '.join(map(str, SHAPE))} fp16 ({n} bits, l = 1), {M}-bit messages, k = 1; median [min .. max] us per call over {reps} alternating rounds of "
      f"~{a.window_ms:.0f} ms windows (at least 2 calls per window); device: {torch.cuda.get_device_name(0)}; board: {json.dumps(board.summary())}")
    p("the counts [B A, M] alone: counts_align = gsw_counts_align; (a) = rows_align + vote_tiled with unit weights + (score + copies) / 2; (b) = A float latents per image "
      "by flip / rot90 / roll + extract_batch(return_counts=True)")
    for r in rows_out:
        c = r["counts"]
        p(f"  A = {r['A']:3d}: counts_align {f(c['counts_align'])}   (a) {f(c['rows_align+vote_tiled'])}   (b) {f(c['torch+extract_batch'])}")
    p("the shared-key search: search = counts_align + trace_topk + the merge per image (the device part of trace_latents_aligned after quant_pack); (a), (b) = their counts + "
      "trace_topk, NO merge; whole = trace_latents_aligned, host statistics included")
    lost = []
    for r in rows_out:
        for U in sizes:
            m = r[f"U{U}"]
            p(f"  A = {r['A']:3d}, U = {U:7d}: search {f(m['search'])}   (a) {f(m['(a)'])}   (b) {f(m['(b)'])}   whole {f(m['whole'])}")
            lost += [(r["A"], U, name) for name in ("(a)", "(b)") if not m["search"]["max_us"] < m[name]["min_us"]]
    for r in rows_out:
        c = r["counts"]
        lost += [(r["A"], "counts", name) for name, k in (("(a)", "rows_align+vote_tiled"), ("(b)", "torch+extract_batch")) if not c["counts_align"]["max_us"] < c[k]["min_us"]]
    p(f"the keyed pair, {len(kreg)} records: search = rows_align + trace_keyed_topk + the merge; (b') = torch alignments + quant_pack + trace_keyed_topk, NO merge; whole = "
      "trace_latents_keyed_aligned")
    for r in keyed_out:
        p(f"  A = {r['A']:3d}: search {f(r['search'])}   (b') {f(r[KEYED_B])}   whole {f(r['whole'])}")
        lost += [(r["A"], "keyed", KEYED_B)] if not r["search"]["max_us"] < r[KEYED_B]["min_us"] else []
    p("the three forms give the same counts bit for bit and the same best score per image at every timed shape")
    p("the fused form is faster than (a), (b) and (b') beyond the spread at every measured point" if not lost
      else f"the fused form is NOT faster beyond the spread at (A, registry or part, form) = {lost}")
    print(out.getvalue(), end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(out.getvalue())
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"rows": rows_out, "keyed": keyed_out, "board": board.summary()}, fh, indent=1)


if __name__ == "__main__":
    main()
