#!/usr/bin/env python3
"""The Viterbi read of error-corrected payloads (codec.viterbi_decode) next to the soft vote that feeds it, and the sigma walk through the device path.

    python tools/ecc_bench.py [--images 1 64 16384] [--rounds 20] [--out profiles/ecc_bench.txt]

Speed.  B latents of 4x64x64 fp16 under their own records, messages of M = 256 and M = 2048 bits, 15 uniform levels.  Per round, one after the other in one
process and timed with device events: gsw_extract_soft on the images, then gsw_viterbi_decode on the votes it wrote.  The report is the median over the
rounds and the spread (min .. max), the decode's time per image, and whether the decode stays below the vote's own launch.

Walk.  tools/ecc_sigma_walk.py's walk (tests/ecc_reference.WALK: 4x32x32 latents, M = 256, 20 images per point, the same keys, payloads, uniforms and noise)
with the embed, the soft vote (`soft.uniform_thresholds` on the device) and the decode on the device: per sigma the coded payloads read back exactly with
ok, next to the CPU walk's count.  Needs a GPU."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, nargs="+", default=[1, 64, 16384])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ecc_bench.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import gswm_amd  # noqa: F401
    from gswm_amd import codec, ecc, soft
    import ecc_reference as R
    if not torch.cuda.is_available():
        raise SystemExit("ecc_bench: no GPU; nothing is measured on a CPU")
    shape = (4, 64, 64)
    lines = [f"# tools/ecc_bench.py --images {' '.join(map(str, a.images))} --rounds {a.rounds}: B x 4x64x64 fp16 under their own records, 15 uniform levels",
             f"# device: {torch.cuda.get_device_name(0)}; vote (gsw_extract_soft) and decode (gsw_viterbi_decode on the vote's scores) interleaved per round; "
             f"median of {a.rounds} rounds (min .. max), device events",
             "#     M       B  way       median_us     min_us     max_us   us/image   decode/vote   payloads_ok"]
    all_ok = True
    below = {}
    for M in (256, 2048):
        mb, pb = M // 8, ecc.capacity(M)
        for B in a.images:
            rs = np.random.RandomState(B + M)
            payloads = [rs.bytes(pb) for _ in range(min(B, 64))]
            coded = [ecc.encode(p, M) for p in payloads]
            rows = np.zeros((B, codec.keyed_record_stride(mb)), dtype=np.uint8)
            rows[:, :48] = rs.randint(0, 256, (B, 48), dtype=np.uint8)
            rows[:, 48:48 + mb] = np.frombuffer(b"".join(coded[b % len(coded)] for b in range(B)), dtype=np.uint8).reshape(B, mb)
            records = torch.from_numpy(rows).cuda()
            z = codec.embed_records(records, mb, shape, seed=1, dtype=torch.float16, fast=True)
            thr = soft.uniform_thresholds(z, 15)
            vote = codec.extract_soft(z, records, mb, thr)
            calls = {"vote": lambda: codec.extract_soft(z, records, mb, thr), "decode": lambda: codec.viterbi_decode(vote.score)}
            times = {w: [] for w in calls}
            for r in range(a.warmup + a.rounds):
                for w, call in calls.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    call()
                    e1.record()
                    torch.cuda.synchronize()
                    if r >= a.warmup:
                        times[w].append(e0.elapsed_time(e1) * 1e-3)
            read = ecc.read(vote.score)                                  # what is timed is also right: every clean image gives its payload back
            ok = all(read.ok) and all(read.payload[b] == payloads[b % len(payloads)] for b in range(B)) and not any(read.flips)
            all_ok = all_ok and ok
            med = {w: statistics.median(t) for w, t in times.items()}
            for w, t in times.items():
                lines.append(f"{M:>7} {B:>7}  {w:<7}  {med[w] * 1e6:>10.1f}  {min(t) * 1e6:>9.1f}  {max(t) * 1e6:>9.1f}  {med[w] * 1e6 / B:>9.3f}  "
                             f"{med['decode'] / med['vote']:>12.3f}   {ok}")
            below[(M, B)] = med["decode"] < med["vote"]
    for M in (256, 2048):
        if (M, 64) in below:
            lines.append(f"# M = {M}, B = 64: the decode {'stays below' if below[(M, 64)] else 'takes longer than'} the vote's own launch")

    # ---- the walk through the device path
    W = R.WALK
    s = R.walk_setup()
    Bw, Mw = W["images"], W["M"]
    coded = [ecc.encode(p, Mw) for p in s["payloads"]]
    rows = np.zeros((Bw, codec.keyed_record_stride(Mw // 8)), dtype=np.uint8)
    rows[:, :48 + Mw // 8] = np.frombuffer(b"".join(s["keys"][b] + s["nonces"][b] + coded[b] for b in range(Bw)), dtype=np.uint8).reshape(Bw, -1)
    records = torch.from_numpy(rows).cuda()
    clean = codec.embed_records(records, Mw // 8, W["shape"], u=torch.from_numpy(s["u"]).cuda(), dtype=torch.float32)
    noise = torch.from_numpy(s["noise"]).cuda().view_as(clean)
    cpu = {sg: c for sg, c, _ in R.walk()}
    lines += [f"# the walk of tools/ecc_sigma_walk.py through the device: embed_records, extract_soft with soft.uniform_thresholds (15 levels), viterbi_decode; "
              f"{Bw} images of {'x'.join(map(str, W['shape']))}, M = {Mw}",
              "#  sigma   coded_device   coded_cpu"]
    for sigma in W["sigmas"]:
        zs = ((clean + sigma * noise) / (1.0 + sigma * sigma) ** 0.5).contiguous()
        read = ecc.read(codec.extract_soft(zs, records, Mw // 8, soft.uniform_thresholds(zs, W["levels"], W["clip"])).score)
        got = sum(1 for b in range(Bw) if read.ok[b] and read.payload[b] == s["payloads"][b])
        lines.append(f"{sigma:>8.2f}  {got:>13}  {cpu[sigma]:>10}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
