"""Microbenchmark of the reliability levels of multi-bit windows through the alignment searches: codec.level_rows_align_l and
codec.level_counts_align_l (csrc/gswm_align_soft_l.inc, csrc/gswm_counts_align_soft_l.inc) and the searches built on them, against what a caller had before
them, timed in the same process:

  rows    fused = one gsw_level_rows_align_l launch for the row and its P planes;
          (a)   = 1 + P launches of codec.rows_align at that l (each computes the source element of every output element again) and the copy that lays the
                  P aligned planes out as [B, A, P, rowbytes];
          (b)   = every candidate alignment of the FLOAT latents by the three torch ops of `align.apply`, one codec.level_pack_l on the B A latents
  counts  fused = one gsw_level_counts_align_l launch (score and wsum, no bias);
          (a)   = level_rows_align_l, then codec.decode_robust(iters=0) on the B A aligned rows (its score and wsum are the level-weighted vote);
          (b)   = the float latents as above, one soft.extract_soft_l on the B A latents
  search  the whole entries with the table given, host statistics included: align.search_keys_soft_l over a 12-key ring against (b) + key_search_soft_topk + the
          merge; trace.trace_latents_aligned_soft_l and trace.trace_latents_keyed_aligned_soft_l over 2^10 records (the keyed one is a composition and has no
          other form)

Cases: 64 images of 4 x 64 x 64 fp16, 256-bit messages; l in {2, 4}; A in {8, 648} candidates (d4 with shifts 0 and 4); levels in {1, 15} (P = 1 and 4 planes).
Every shape is warmed up first, then --reps rounds alternate a timed window of every form (device events around back-to-back calls, a device synchronise at the
end of every window).  Before timing, the forms are compared: every output must be equal bit for bit.

Reported: median [min .. max] us per call over the rounds, and where a fused form is NOT faster than (a) or (b) beyond the spread (its slowest round against
the other's fastest).  No ratio is promised in advance.

usage: python tools/align_soft_l_bench.py [--reps 5] [--window-ms 30] [--out profiles/align_soft_l_bench.txt] [--quick]
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
SHIFTS = {8: 0, 648: 4}
LEVELS = (1, 15)
WINDOWS = (2, 4)


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
    for _ in range(reps):                           # alternate the forms inside every round
        for name, f in fns.items():
            t[name].append(window(f, iters[name]))
    return {name: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "iters": iters[name]} for name, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=30.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_soft_l_bench.txt"))
    ap.add_argument("--quick", action="store_true", help="two rounds")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "align_soft_l_bench needs the GPU (there is no CPU path to time)"
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    reps = 2 if a.quick else a.reps
    M, n = 8 * MB, SHAPE[0] * SHAPE[1] * SHAPE[2]
    rng = np.random.default_rng(0)
    key, nonce = bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8))
    U = 1 << 10
    msgs = rng.integers(0, 256, (U, MB), dtype=np.uint8)
    reg = T.Registry(MB)
    kreg = T.KeyedRegistry(MB)
    for u in range(U):
        reg.add(f"u{u}", msgs[u].tobytes())
        kreg.add(f"u{u}", bytes(rng.integers(0, 256, 32, dtype=np.uint8)), nonce, msgs[u].tobytes())
    ring = np.stack([np.frombuffer(bytes(rng.integers(0, 256, 48, dtype=np.uint8)), dtype=np.uint8) for _ in range(12)])
    keys_dev = torch.from_numpy(ring.copy()).to(dev)
    z = torch.randn(B, *SHAPE, device=dev, generator=g).half()
    key_row = torch.from_numpy(np.frombuffer(key + nonce, dtype=np.uint8).copy()).to(dev)
    rows_out, counts_out, search_out = [], [], []
    from bench_board import BoardSampler
    with BoardSampler(0) as board:
        for l in WINDOWS:
            for A, shift in SHIFTS.items():
                aligns = AL.alignments("d4", shift, SHAPE[1], SHAPE[2])
                assert len(aligns) == A
                table = torch.from_numpy(codec.align_table(aligns, SHAPE)).to(dev)
                keys_ba = key_row.expand(B * A, 48).contiguous()
                for levels in LEVELS:
                    thr = S.window_thresholds(z, l, levels)
                    rows = codec.level_pack_l(z, thr, l)
                    P, rb = rows.planes.shape[1], rows.signs.shape[1]
                    thr_ba = thr.repeat_interleave(A, dim=0).contiguous()
                    plane_rows = [rows.planes[:, k].contiguous() for k in range(P)]

                    def floats():
                        return torch.stack([AL.apply(z, al) for al in aligns], dim=1).view(B * A, *SHAPE)      # what a caller builds without any kernel

                    def rows_fused():
                        return codec._level_rows_align_launch(rows, SHAPE, table, l)

                    def rows_a():
                        s = codec._rows_align_launch(rows.signs, SHAPE, l, table)
                        return s, torch.stack([codec._rows_align_launch(p, SHAPE, l, table) for p in plane_rows], dim=2)

                    def rows_b():
                        r = codec.level_pack_l(floats(), thr_ba, l)
                        return r.signs.view(B, A, rb), r.planes.view(B, A, P, rb)

                    want = rows_fused()
                    for name, other in (("(a)", rows_a()), ("(b)", rows_b())):
                        assert torch.equal(want[0], other[0]) and torch.equal(want[1], other[1]), f"rows: the fused form and {name} disagree"
                    rows_out.append({"l": l, "A": A, "levels": levels, "P": P, **measure({"fused": rows_fused, "(a)": rows_a, "(b)": rows_b}, reps, a.window_ms)})

                    def counts_fused():
                        return codec._level_counts_align_launch(rows, SHAPE, table, key, nonce, M, 0, True, l)

                    def counts_a():
                        s, p = codec._level_rows_align_launch(rows, SHAPE, table, l)
                        v = codec.decode_robust(s.view(B * A, rb), p.view(B * A, P, rb), keys_ba, M, SHAPE, l, 8, iters=0)
                        return v.score, v.wsum

                    def counts_b():
                        v = S.extract_soft_l(floats(), key, nonce, M, l, thresholds=thr_ba)
                        return v.score, v.wsum

                    want = tuple(t.view(B * A, M) for t in counts_fused())
                    forms = {"fused": counts_fused, "(b)": counts_b}
                    try:
                        counts_a()
                        forms["(a)"] = counts_a
                    except ValueError as err:                                           # decode_robust's own limits (its LDS cap binds before this kernel's)
                        print(f"[align_soft_l_bench] l = {l}, levels = {levels}: form (a) of the counts is refused: {err}", file=sys.stderr)
                    for name, f in forms.items():
                        if name != "fused":
                            other = f()
                            assert torch.equal(want[0], other[0]) and torch.equal(want[1], other[1]), f"counts: the fused form and {name} disagree"
                    counts_out.append({"l": l, "A": A, "levels": levels, "P": P, **measure(forms, reps, a.window_ms)})

                    def keys_whole():
                        return AL.search_keys_soft_l(z, keys_dev, MB, aligns, l, thresholds=thr)

                    def keys_b():
                        r = codec.level_pack_l(floats(), thr_ba, l)
                        idx, stat = codec.key_search_soft_topk(r, n * l, keys_dev, MB, k=1)
                        return AL._merge_best(idx.view(B, A), stat.view(B, A), 12, stat_bits=AL.SOFT_STAT_BITS)

                    assert all(torch.equal(x, y) for x, y in zip(keys_whole(), keys_b())), "key search: the entry and (b) disagree"

                    def shared_whole():
                        return T.trace_latents_aligned_soft_l(z, key, nonce, reg, aligns, l, thresholds=thr)

                    def keyed_whole():
                        return T.trace_latents_keyed_aligned_soft_l(z, kreg, aligns, l, thresholds=thr)

                    search_out.append({"l": l, "A": A, "levels": levels,
                                       **measure({"keys": keys_whole, "keys (b)": keys_b, "shared": shared_whole, "keyed": keyed_whole}, reps, a.window_ms)})
                    print(f"[align_soft_l_bench] l = {l}, A = {A}, levels = {levels} done", file=sys.stderr, flush=True)
    out = io.StringIO()
    p = lambda *x: print(*x, file=out)
    f = lambda d: f"{d['median_us']:.1f} [{d['min_us']:.1f} .. {d['max_us']:.1f}]" if d else "refused"
    p(f"{B} images of {' x '.join(map(str, SHAPE))} fp16 ({n} elements), {M}-bit messages, k = 1; median [min .. max] us per call over {reps} alternating rounds "
      f"of ~{a.window_ms:.0f} ms windows (at least 2 calls per window); device: {torch.cuda.get_device_name(0)}; board: {json.dumps(board.summary())}")
    p("the aligned rows [B, A, (1 + P), n l / 8]: fused = gsw_level_rows_align_l; (a) = 1 + P launches of rows_align(l) + the copy of the planes to [B, A, P, .]; "
      "(b) = A float latents per image by flip / rot90 / roll + level_pack_l")
    lost = []
    for r in rows_out:
        p(f"  l = {r['l']}, A = {r['A']:3d}, levels = {r['levels']:2d} (P = {r['P']}): fused {f(r['fused'])}   (a) {f(r['(a)'])}   (b) {f(r['(b)'])}")
        lost += [("rows", r["l"], r["A"], r["levels"], name) for name in ("(a)", "(b)") if not r["fused"]["max_us"] < r[name]["min_us"]]
    p("score and wsum [B A, M]: fused = gsw_level_counts_align_l (both outputs, no bias); (a) = level_rows_align_l + decode_robust(iters=0) on the B A rows; "
      "(b) = the float latents + soft.extract_soft_l with the table given")
    for r in counts_out:
        p(f"  l = {r['l']}, A = {r['A']:3d}, levels = {r['levels']:2d} (P = {r['P']}): fused {f(r['fused'])}   (a) {f(r.get('(a)'))}   (b) {f(r['(b)'])}")
        lost += [("counts", r["l"], r["A"], r["levels"], name) for name in ("(a)", "(b)") if name in r and not r["fused"]["max_us"] < r[name]["min_us"]]
    p(f"the whole searches, the table given, host statistics included: keys = align.search_keys_soft_l over 12 keys; keys (b) = the float latents + level_pack_l + "
      f"key_search_soft_topk + the merge; shared = trace_latents_aligned_soft_l, keyed = trace_latents_keyed_aligned_soft_l over {U} records")
    for r in search_out:
        p(f"  l = {r['l']}, A = {r['A']:3d}, levels = {r['levels']:2d}: keys {f(r['keys'])}   keys (b) {f(r['keys (b)'])}   shared {f(r['shared'])}   keyed {f(r['keyed'])}")
        lost += [("keys", r["l"], r["A"], r["levels"], "(b)")] if not r["keys"]["max_us"] < r["keys (b)"]["min_us"] else []
    p("the forms give the same rows, the same score and wsum and the same best key per image bit for bit at every timed shape")
    p("the fused forms are faster than (a) and (b) beyond the spread at every measured point" if not lost
      else f"a fused form is NOT faster beyond the spread at (part, l, A, levels, form) = {lost}")
    print(out.getvalue(), end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(out.getvalue())


if __name__ == "__main__":
    main()
