"""Microbenchmark of the aligned registry search ranked by reliability levels (trace.trace_latents_aligned_soft: codec.level_pack ->
codec.level_counts_align -> codec.trace_topk -> a merge on the device; csrc/gswm_counts_align_soft.inc) against the two forms a caller had before it,
timed in the same process:

  (a) codec.level_rows_align, then codec.decode_robust(iters=0) on the B A aligned rows (its score and wsum are the level-weighted vote);
  (b) every candidate alignment of the FLOAT latents built with the three torch ops of `align.apply`, one soft.extract_soft on the B A latents with the
      table given (each aligned latent with its image's row of it).

Both yardsticks are compositions of entry points that existed before gsw_level_counts_align; both are timed WITHOUT the bias, the merge or the search.
codec.counts_align (signs alone) is timed next to them.  Then the whole shared-key search against registries of 2^10 and 2^20 rows, and the keyed
composition (trace.trace_latents_keyed_aligned_soft: level_rows_align -> trace_keyed_soft_topk -> merge, no kernel of its own) against 2^10 records.

Cases: 64 images of 4 x 64 x 64 fp16, 256-bit messages; levels in {1, 3, 15} (P = 1, 2, 4 planes); A in {8, 200, 648} candidates (d4 with shifts 0, 2,
4).  Every shape is warmed up first, then --reps rounds alternate a timed window of every form (device events around back-to-back calls, a device
synchronise at the end of every window).  Before timing, the forms are compared: score and wsum must be equal bit for bit.

Reported: median [min .. max] us per call over the rounds, and where the fused form is NOT faster than (a) or (b) beyond the spread (its slowest round
against the other's fastest).  No ratio is promised in advance.

usage: python tools/trace_align_soft_bench.py [--reps 5] [--window-ms 30] [--out profiles/trace_align_soft_bench.txt] [--json FILE] [--quick]
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
from gswm_amd import align as AL, codec, soft as S, trace as T  # noqa: E402

B, SHAPE, MB = 64, (4, 64, 64), 32
SHIFTS = {8: 0, 200: 2, 648: 4}
LEVELS = (1, 3, 15)
ATTACK = (5, 1, -2)
SIGMA = 2.0


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
    """`whole` includes host statistics: one call per window, warmed up by the caller's own first call"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_align_soft_bench.txt"))
    ap.add_argument("--json", default=None)
    ap.add_argument("--quick", action="store_true", help="two rounds, the small registry only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "trace_align_soft_bench needs the GPU (there is no CPU path to time)"
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
    marked = AL.apply(codec.embed_batch(key, nonce, msgs[341].tobytes(), 1, SHAPE, seed=1)[0], ATTACK)          # one attacked, noisy image of user 341
    z[0] = (marked + SIGMA * torch.randn(*SHAPE, device=dev, generator=g)).clamp(-8.0, 8.0).half()
    packed, _ = codec.quant_pack(z, 1)
    key_row = torch.from_numpy(np.frombuffer(key + nonce, dtype=np.uint8).copy()).to(dev)
    counts_out, shared_out, keyed_out = [], [], []
    from bench_board import BoardSampler
    with BoardSampler(0) as board:
        for A, shift in SHIFTS.items():
            aligns = AL.alignments("d4", shift, SHAPE[1], SHAPE[2])
            assert len(aligns) == A
            table = torch.from_numpy(codec.align_table(aligns, SHAPE)).to(dev)
            keys_ba = key_row.expand(B * A, 48).contiguous()

            def counts_signs():
                return codec._counts_align_launch(packed, SHAPE, 1, table, key, nonce, M)

            for levels in LEVELS:
                thr = S.uniform_thresholds(z, levels)
                rows = codec.level_pack(z, thr)
                P = rows.planes.shape[1]
                thr_ba = thr.repeat_interleave(A, dim=0).contiguous()
                bias = levels * V

                def fused():
                    return codec._level_counts_align_launch(rows, SHAPE, table, key, nonce, M, 0, True)

                def form_a():
                    al = codec.level_rows_align(rows, SHAPE, table)
                    v = codec.decode_robust(al.signs, al.planes, keys_ba, M, SHAPE, 1, 8, iters=0)
                    return v.score, v.wsum

                def form_b():
                    t = torch.stack([AL.apply(z, al) for al in aligns], dim=1)             # [B, A, C, H, W]: what a caller builds without any kernel
                    v = S.extract_soft(t.view(B * A, *SHAPE), key, nonce, M, thresholds=thr_ba)
                    return v.score, v.wsum

                want = tuple(t.view(B * A, M) for t in fused())
                for name, other in (("(a)", form_a()), ("(b)", form_b())):
                    assert torch.equal(want[0], other[0]) and torch.equal(want[1], other[1]), f"the fused form and {name} disagree"
                counts_out.append({"A": A, "levels": levels, "P": P,
                                   **measure({"fused": fused, "(a)": form_a, "(b)": form_b, "counts_align": counts_signs}, reps, a.window_ms)})
                for U, reg in regs.items():
                    reg_dev = reg.to_device(dev)

                    def search():
                        counts = codec._level_counts_align_launch(rows, SHAPE, table, key, nonce, M, bias)
                        idx, score = codec.trace_topk(counts.view(B * A, M), 2 * bias, reg_dev, k=1)
                        return AL._merge_best(idx.view(B, A), torch.where(idx >= 0, score // 2, score).view(B, A), U, stat_bits=AL.SOFT_STAT_BITS)

                    def search_a():
                        counts = form_a()[0] + bias
                        idx, score = codec.trace_topk(counts, 2 * bias, reg_dev, k=1)
                        return idx, torch.where(idx >= 0, score // 2, score)

                    def whole():
                        return T.trace_latents_aligned_soft(z, key, nonce, reg, aligns, thresholds=thr)

                    res = whole()
                    if shift >= 2:                                                      # the attacked image: its user, and the alignment that undoes the attack
                        assert res[0].attributed == "u341" and res[0].alignment == AL.inverse(ATTACK, SHAPE[1], SHAPE[2])
                    st = search()[2]
                    assert torch.equal(st[:, 0], search_a()[1].view(B, A).max(dim=1).values) and int(st[0, 0]) == res[0].candidates[0].score
                    shared_out.append({"A": A, "levels": levels, "U": U, **measure({"search": search, "(a)": search_a, "whole": whole}, reps, a.window_ms)})
                    print(f"[trace_align_soft_bench] A = {A}, levels = {levels}, U = {U} done", file=sys.stderr, flush=True)
                # ---- the keyed composition, 2^10 records
                rec_dev = kreg.to_device(dev)

                def keyed_search():
                    signs, planes = codec._level_rows_align_launch(rows, SHAPE, table)
                    al = codec.LevelRows(signs.view(B * A, -1), planes.view(B * A, P, -1), rows.wsum.repeat_interleave(A), rows.wsq, rows.flags)
                    idx, score = codec.trace_keyed_soft_topk(al, n, rec_dev, MB, k=1)
                    return AL._merge_best(idx.view(B, A), score.view(B, A), len(kreg), stat_bits=AL.SOFT_STAT_BITS)

                def keyed_whole():
                    return T.trace_latents_keyed_aligned_soft(z, kreg, aligns, thresholds=thr)

                res = keyed_whole()
                if shift >= 2:
                    assert res[0].attributed == "u341" and res[0].alignment == AL.inverse(ATTACK, SHAPE[1], SHAPE[2])
                assert int(keyed_search()[2][0, 0]) == res[0].candidates[0].score
                keyed_out.append({"A": A, "levels": levels, **measure({"search": keyed_search, "whole": keyed_whole}, reps, a.window_ms)})
    out = io.StringIO()
    p = lambda *x: print(*x, file=out)
    f = lambda d: f"{d['median_us']:.1f} [{d['min_us']:.1f} .. {d['max_us']:.1f}]"
    p(f"{B} images of {' x '.join(map(str, SHAPE))} fp16 ({n} elements, l = 1), {M}-bit messages, k = 1; median [min .. max] us per call over {reps} alternating rounds "
      f"of ~{a.window_ms:.0f} ms windows (at least 2 calls per window); device: {torch.cuda.get_device_name(0)}; board: {json.dumps(board.summary())}")
    p("score and wsum [B A, M] alone: fused = gsw_level_counts_align (both outputs, no bias); (a) = level_rows_align + decode_robust(iters=0) on the B A rows; "
      "(b) = A float latents per image by flip / rot90 / roll + soft.extract_soft with the table given; counts_align = the sign counts of the same alignments")
    lost = []
    for r in counts_out:
        p(f"  A = {r['A']:3d}, levels = {r['levels']:2d} (P = {r['P']}): fused {f(r['fused'])}   (a) {f(r['(a)'])}   (b) {f(r['(b)'])}   counts_align {f(r['counts_align'])}")
        lost += [(r["A"], r["levels"], "counts", name) for name in ("(a)", "(b)") if not r["fused"]["max_us"] < r[name]["min_us"]]
    p("the shared-key search: search = level_counts_align (bias = levels V) + trace_topk + the merge per image (the device part of trace_latents_aligned_soft after "
      "level_pack); (a) = its score + bias + trace_topk, NO merge; whole = trace_latents_aligned_soft with the table given, host statistics included")
    for r in shared_out:
        p(f"  A = {r['A']:3d}, levels = {r['levels']:2d}, U = {r['U']:7d}: search {f(r['search'])}   (a) {f(r['(a)'])}   whole {f(r['whole'])}")
        lost += [(r["A"], r["levels"], r["U"], "(a)")] if not r["search"]["max_us"] < r["(a)"]["min_us"] else []
    p(f"the keyed composition, {len(kreg)} records: search = level_rows_align + trace_keyed_soft_topk + the merge (no kernel of its own); whole = "
      "trace_latents_keyed_aligned_soft with the table given")
    for r in keyed_out:
        p(f"  A = {r['A']:3d}, levels = {r['levels']:2d}: search {f(r['search'])}   whole {f(r['whole'])}")
    p("the three forms give the same score and wsum bit for bit and the same best score per image at every timed shape")
    p("the fused form is faster than (a) and (b) beyond the spread at every measured point" if not lost
      else f"the fused form is NOT faster beyond the spread at (A, levels, registry or part, form) = {lost}")
    print(out.getvalue(), end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(out.getvalue())
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"counts": counts_out, "shared": shared_out, "keyed": keyed_out, "board": board.summary()}, fh, indent=1)


if __name__ == "__main__":
    main()
