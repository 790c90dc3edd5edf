#!/usr/bin/env python3
"""The punctured payload codes through both Viterbi reads: the plain read (gsw_viterbi_decode_rate) and the list read (gsw_viterbi_list_decode_rate, L = 1, 2,
4, 8) under "conv" (rate 1/2), "conv23" (2/3) and "conv34" (3/4), next to the older rate-1/2 entry points on the same run.

    python tools/ecc_rate_bench.py [--images 1 64 16384] [--rounds 20] [--reps 10] [--out profiles/ecc_rate_bench.txt]

Method (tools/ecc_list_bench.py's).  Votes of B latents of 4x64x64 fp16 under their own records (gsw_extract_soft, 15 uniform levels), messages of M = 256 and
M = 2048 bits, every code's own coded payloads.  One process; per round every way runs once, one after the other (interleaved), into buffers allocated before
the first round: the C entry points are called directly, `reps` launches back to back between two device events, the time of a way in a round is the events'
time over `reps`.  The report is the median over the rounds with the spread (min .. max) and the ratio of each code to the rate-1/2 read of the same run at
the same M, B and L -- the yardstick; no speed target is fixed in advance.  The expectation it confirms or refutes: time follows the trellis steps T, about
4/3 (conv23) and 3/2 (conv34) of the rate-1/2 read.  Needs a GPU."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

LS = (0, 1, 2, 4, 8)                    # 0: the plain read


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, nargs="+", default=[1, 64, 16384])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ecc_rate_bench.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import gswm_amd  # noqa: F401
    from gswm_amd import _native as N, codec, ecc, soft
    import ecc_rate_reference as Q
    if not torch.cuda.is_available():
        raise SystemExit("ecc_rate_bench: no GPU; nothing is measured on a CPU")
    lib = N.lib()
    stream = codec._stream_ptr()
    shape = (4, 64, 64)
    name = lambda L: "plain" if L == 0 else f"L{L}"
    lines = [f"# tools/ecc_rate_bench.py --images {' '.join(map(str, a.images))} --rounds {a.rounds} --reps {a.reps}: votes of B x 4x64x64 fp16 under their own "
             f"records, 15 uniform levels, every code's own coded payloads",
             f"# device: {torch.cuda.get_device_name(0)}; one process, the ways interleaved per round, {a.reps} launches between two device events, "
             f"median of {a.rounds} rounds (min .. max) of the time per launch",
             "# conv / conv23 / conv34 = gsw_viterbi_decode_rate and gsw_viterbi_list_decode_rate at rate 0 / 1 / 2; old = gsw_viterbi_decode and "
             "gsw_viterbi_list_decode (rate 1/2); vs_conv = the way's median over the rate-1/2 read of the same run at the same M, B and L",
             "#     M       B  read   code        T   median_us     min_us     max_us   us/image    vs_conv   results_equal"]
    all_ok = True
    summary = []
    for M in (256, 2048):
        mb = M // 8
        for B in a.images:
            rs = np.random.RandomState(B + M)
            score = {}
            for code in ecc.CODES:
                payloads = [rs.bytes(ecc.capacity(M, code)) for _ in range(min(B, 64))]
                coded = [ecc.encode(p, M, code) for p in payloads]
                rows = np.zeros((B, codec.keyed_record_stride(mb)), dtype=np.uint8)
                rows[:, :48] = rs.randint(0, 256, (B, 48), dtype=np.uint8)
                rows[:, 48:48 + mb] = np.frombuffer(b"".join(coded[b % len(coded)] for b in range(B)), dtype=np.uint8).reshape(B, mb)
                records = torch.from_numpy(rows).cuda()
                z = codec.embed_records(records, mb, shape, seed=1, dtype=torch.float16, fast=True)
                z = (z.float() + 1.5 * torch.randn(z.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(B + M))).half() * (1.0 / 3.25 ** 0.5)
                score[code] = codec.extract_soft(z, records, mb, soft.uniform_thresholds(z, 15)).score.contiguous()
            i32 = lambda: torch.empty((B,), dtype=torch.int32, device="cuda")
            outs, calls = {}, {}

            def buffers(w, code):
                outs[w] = (torch.empty((B, codec.viterbi_steps(M, code) // 8), dtype=torch.uint8, device="cuda"),
                           torch.empty((B, M // 8), dtype=torch.uint8, device="cuda"), i32(), i32(), i32(), i32(), i32())
                return [t.data_ptr() for t in outs[w]]

            for L in LS:
                for rate, code in enumerate(ecc.CODES):
                    ptr, sc = buffers((L, code), code), score[code]
                    if L == 0:
                        calls[(L, code)] = lambda ptr=ptr, sc=sc, rate=rate: lib.gsw_viterbi_decode_rate(sc.data_ptr(), M, B, M, rate, *ptr[:5], stream)
                    else:
                        calls[(L, code)] = lambda ptr=ptr, sc=sc, rate=rate, L=L: lib.gsw_viterbi_list_decode_rate(sc.data_ptr(), M, B, M, rate, L, *ptr, stream)
                ptr, sc = buffers((L, "old"), "conv"), score["conv"]
                if L == 0:
                    calls[(L, "old")] = lambda ptr=ptr, sc=sc: lib.gsw_viterbi_decode(sc.data_ptr(), M, B, M, *ptr[:5], stream)
                else:
                    calls[(L, "old")] = lambda ptr=ptr, sc=sc, L=L: lib.gsw_viterbi_list_decode(sc.data_ptr(), M, B, M, L, *ptr, stream)
            times = {w: [] for w in calls}
            for r in range(a.warmup + a.rounds):
                for w, call in calls.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.reps):
                        st = call()
                    e1.record()
                    torch.cuda.synchronize()
                    if st != 0:
                        raise SystemExit(f"ecc_rate_bench: {w} returned {st}")
                    if r >= a.warmup:
                        times[w].append(e0.elapsed_time(e1) * 1e-3 / a.reps)
            # what is timed is also right: rate 0 equals the older entry point, four rows of the batch equal the restatement
            equal = {}
            for (L, code) in calls:
                n = 5 if L == 0 else 7
                if code == "old":
                    equal[(L, code)] = True
                    continue
                ok = True
                if code == "conv":
                    ok = all(torch.equal(x, y) for x, y in zip(outs[(L, "conv")][:n], outs[(L, "old")][:n]))
                want = Q.decode_list(score[code].cpu().numpy()[:4], max(L, 1), code)
                ok = ok and all(np.array_equal(outs[(L, code)][i].cpu().numpy()[:4], want[k]) for i, k in enumerate(Q.NAMES[:n]))
                equal[(L, code)] = ok
            all_ok = all_ok and all(equal.values())
            med = {w: statistics.median(t) for w, t in times.items()}
            for (L, code), t in times.items():
                T = codec.viterbi_steps(M, "conv" if code == "old" else code)
                lines.append(f"{M:>7} {B:>7}  {name(L):<5}  {code:<7} {T:>6}  {med[(L, code)] * 1e6:>10.1f}  {min(t) * 1e6:>9.1f}  {max(t) * 1e6:>9.1f}  "
                             f"{med[(L, code)] * 1e6 / B:>9.3f}  {med[(L, code)] / med[(L, 'conv')]:>9.2f}   {equal[(L, code)]}")
            for L in LS:
                lo, hi = min(times[(L, "old")]), max(times[(L, "old")])
                summary.append(f"# M = {M}, B = {B}, {name(L)}: conv23 / conv = {med[(L, 'conv23')] / med[(L, 'conv')]:.2f} (T ratio "
                               f"{codec.viterbi_steps(M, 'conv23') / codec.viterbi_steps(M, 'conv'):.2f}), conv34 / conv = "
                               f"{med[(L, 'conv34')] / med[(L, 'conv')]:.2f} (T ratio {codec.viterbi_steps(M, 'conv34') / codec.viterbi_steps(M, 'conv'):.2f}); "
                               f"rate 0 through the new entry point is {'within' if lo <= med[(L, 'conv')] <= hi else 'OUTSIDE'} the older entry point's spread "
                               f"({med[(L, 'conv')] * 1e6:.1f} us against {lo * 1e6:.1f} .. {hi * 1e6:.1f} us)")
    lines += summary
    lines.append(f"# every timed result {'equals' if all_ok else 'DIFFERS from'} the restatement on the rows compared, and rate 0 the older entry points")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
