#!/usr/bin/env python3
"""Embed + extract with one record per image (codec.embed_records / codec.extract_records) against the two ways a caller has without them.

    python tools/codec_keyed_bench.py [--images 64 16384] [--rounds 20] [--out profiles/codec_keyed_bench.txt]

Shape: B latents of 4x64x64 fp16, 32-byte messages, l = 1, embed on the fp32 core and the in-kernel Philox stream.  Per round, one after
the other and timed with device events:
  keyed   : ONE gsw_embed_keyed launch, ONE gsw_extract_keyed launch, every image under its own key, nonce and message
  shared  : gsw_embed / gsw_extract of the same B under ONE key (codec.embed_batch / extract_batch): the ceiling, the keystream is
            computed once per chunk for the whole batch
  loop    : B one-image launches of the shared-key kernels, each with its image's record: what per-image keys cost a caller before
            (at most --loop_images images are looped and the time is scaled to B; the loop is launch-bound, so it scales linearly)
The report is the median over the rounds and the spread (min .. max).  Needs a GPU: there is no CPU path to time.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, nargs="+", default=[64, 16384])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop_images", type=int, default=256, help="images the one-launch-per-image loop really runs per round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec_keyed_bench.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import gswm_amd  # noqa: F401
    from gswm_amd import codec
    if not torch.cuda.is_available():
        raise SystemExit("codec_keyed_bench: no GPU; nothing is measured on a CPU")
    shape, M, mb = (4, 64, 64), 256, 32
    ways = ("keyed", "shared", "loop")
    lines = [f"# tools/codec_keyed_bench.py --images {' '.join(map(str, a.images))} --rounds {a.rounds}: B x 4x64x64 fp16, 32-byte messages, l = 1, embed fast/Philox",
             f"# device: {torch.cuda.get_device_name(0)}; keyed / shared / loop interleaved per round; median of {a.rounds} rounds (min .. max); bytes = the latents, once per launch",
             "#     B  way     launch   median_us     min_us     max_us   GB/s(median)   vs_shared   vs_loop   round_trip_ok"]
    all_ok = True
    for B in a.images:
        rs = np.random.RandomState(B)
        rows = np.zeros((B, codec.keyed_record_stride(mb)), dtype=np.uint8)
        rows[:, :48 + mb] = rs.randint(0, 256, (B, 48 + mb), dtype=np.uint8)
        records = torch.from_numpy(rows).cuda()
        recs = [(bytes(r[:32]), bytes(r[32:48]), bytes(r[48:48 + mb])) for r in rows]
        z = torch.empty((B, *shape), dtype=torch.float16, device="cuda")
        nbytes = z.numel() * z.element_size()
        LB = min(B, a.loop_images)
        scale = B / LB
        times = {(w, s): [] for w in ways for s in ("embed", "extract")}
        ok = {}

        def timed(way, record, embed, extract):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            embed()
            e1.record()
            res = extract()
            e2.record()
            torch.cuda.synchronize()
            if record:
                f = scale if way == "loop" else 1.0
                times[(way, "embed")].append(e0.elapsed_time(e1) * 1e-3 * f)
                times[(way, "extract")].append(e1.elapsed_time(e2) * 1e-3 * f)
            return res

        def loop_embed():
            for b in range(LB):
                codec.embed_batch(*recs[b], 1, shape, seed=1, image_index0=b, dtype=torch.float16, fast=True, out=z[b:b + 1])

        def loop_extract():
            return [codec.extract_batch(z[b:b + 1], recs[b][0], recs[b][1], M) for b in range(LB)]

        for r in range(a.warmup + a.rounds):
            rec = r >= a.warmup
            bits, flags = timed("shared", rec, lambda: codec.embed_batch(*recs[0], B, shape, seed=1, dtype=torch.float16, fast=True, out=z),
                                lambda: codec.extract_batch(z, recs[0][0], recs[0][1], M))
            if r == 0:
                ok["shared"] = int(flags.abs().sum()) == 0 and int(codec.bit_matches(bits, M, recs[0][2]).min()) == M
            res = timed("loop", rec, loop_embed, loop_extract)
            if r == 0:
                ok["loop"] = all(int(f.abs().sum()) == 0 and bt.cpu().numpy().tobytes() == recs[b][2] for b, (bt, f) in enumerate(res))
            bits, flags, matches = timed("keyed", rec, lambda: codec.embed_records(records, mb, shape, seed=1, dtype=torch.float16, fast=True, out=z),
                                         lambda: codec.extract_records(z, records, mb))
            if r == 0:      # what is timed is also right: every image gives its own message back
                ok["keyed"] = int(flags.abs().sum()) == 0 and int(matches.min()) == M and bool((bits.cpu() == torch.from_numpy(rows[:, 48:48 + mb])).all())
        for s in ("embed", "extract"):
            for w in ways:
                t = times[(w, s)]
                med = statistics.median(t)
                sh, lo = statistics.median(times[("shared", s)]), statistics.median(times[("loop", s)])
                note = f" (x{scale:g} from {LB} images)" if w == "loop" and scale != 1 else ""
                lines.append(f"{B:>7}  {w:<6}  {s:<7}  {med * 1e6:>9.1f}  {min(t) * 1e6:>9.1f}  {max(t) * 1e6:>9.1f}  {nbytes / med / 1e9:>12.1f}  {sh / med:>10.3f}  {lo / med:>8.2f}  "
                             f"{ok[w]}{note}")
        all_ok = all_ok and all(ok.values())
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
