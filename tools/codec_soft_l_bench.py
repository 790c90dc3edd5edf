#!/usr/bin/env python3
"""The soft-decision vote for multi-bit windows (codec.extract_soft_l, codec.level_pack_l) against the kernels that move the same bytes
(codec.extract_records(l=...), codec.quant_pack), and what the vote buys.

    python tools/codec_soft_l_bench.py [--images 64 16384] [--rounds 20] [--out profiles/codec_soft_l_bench.txt]

Speed.  B latents of 4x64x64 fp16, 32-byte messages, every image under its own record, l = 2 and 4.  Per round, one after the other in one
process and timed with device events: gsw_extract_keyed at that l, gsw_extract_soft_l at 1 level (the table of zeros: the sign vote), 3 and
15 levels (`soft.window_thresholds`), then gsw_quant_pack and gsw_level_pack_l at 1, 3 and 15 levels.  The keyed extract and quant_pack of
the same round are the yardsticks; the report is the median over the rounds and the spread (min .. max).

Robustness.  --noise_images watermarked images (embed_records at that l), Gaussian noise drawn on the device at sigma = 0.5, 1 and 2, fp16:
bits recovered by the keyed extract (the sign vote) and by the window vote at 3 and 15 levels with `soft.window_thresholds`.  Needs a GPU.
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
    ap.add_argument("--noise_images", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec_soft_l_bench.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import gswm_amd  # noqa: F401
    from gswm_amd import codec, soft
    if not torch.cuda.is_available():
        raise SystemExit("codec_soft_l_bench: no GPU; nothing is measured on a CPU")
    shape, mb = (4, 64, 64), 32
    M = 8 * mb
    level_set = (1, 3, 15)
    ways = ("keyed",) + tuple(f"soft{t}" for t in level_set) + ("qpack",) + tuple(f"lpack{t}" for t in level_set)

    def records_for(B):
        rs = np.random.RandomState(B)
        rows = np.zeros((B, codec.keyed_record_stride(mb)), dtype=np.uint8)
        rows[:, :48 + mb] = rs.randint(0, 256, (B, 48 + mb), dtype=np.uint8)
        return torch.from_numpy(rows).cuda()

    lines = [f"# tools/codec_soft_l_bench.py --images {' '.join(map(str, a.images))} --rounds {a.rounds}: B x 4x64x64 fp16, 32-byte messages, one record per image",
             f"# device: {torch.cuda.get_device_name(0)}; the eight ways interleaved per round; median of {a.rounds} rounds (min .. max); bytes = the latents, once per launch",
             "# keyed = gsw_extract_keyed(l), softT = gsw_extract_soft_l at T levels, qpack = gsw_quant_pack(l), lpackT = gsw_level_pack_l at T levels; "
             "vs = the yardstick's median / this median (keyed for soft*, qpack for lpack*)",
             "#  l       B  way      median_us     min_us     max_us   GB/s(median)         vs   clean_ok"]
    all_ok = True
    for l in (2, 4):
        for B in a.images:
            records = records_for(B)
            z = codec.embed_records(records, mb, shape, seed=1, dtype=torch.float16, fast=True, l=l)
            nbytes = z.numel() * z.element_size()
            tables = {t: soft.window_thresholds(z, l, t) for t in level_set}
            tables[1] = torch.zeros((B, l, 1), dtype=torch.float32, device="cuda")   # one level at 0: the sign vote, bit for bit the keyed extract's result
            calls = {"keyed": lambda: codec.extract_records(z, records, mb, l=l), "qpack": lambda: codec.quant_pack(z, l)}
            for t in level_set:
                calls[f"soft{t}"] = (lambda thr: lambda: codec.extract_soft_l(z, records, mb, thr, l))(tables[t])
                calls[f"lpack{t}"] = (lambda thr: lambda: codec.level_pack_l(z, thr, l))(tables[t])
            times = {w: [] for w in ways}
            ok = {}
            sign_row = None
            for r in range(a.warmup + a.rounds):
                for w in ways:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    res = calls[w]()
                    e1.record()
                    torch.cuda.synchronize()
                    if r >= a.warmup:
                        times[w].append(e0.elapsed_time(e1) * 1e-3)
                    if r == 0:      # what is timed is also right: a clean image gives its own message back, a packed row is quant_pack's
                        if w == "qpack":
                            sign_row = res[0]
                            ok[w] = int(res[1].abs().sum()) == 0
                        elif w.startswith("lpack"):
                            ok[w] = bool(torch.equal(res.signs, sign_row)) and int(res.flags.abs().sum()) == 0
                        else:
                            ok[w] = int(res[1].abs().sum()) == 0 and int(res[2].min()) == M
            base = {"keyed": statistics.median(times["keyed"]), "qpack": statistics.median(times["qpack"])}
            for w in ways:
                t = times[w]
                med = statistics.median(t)
                ref = base["qpack"] if w in ("qpack",) or w.startswith("lpack") else base["keyed"]
                lines.append(f"{l:>4} {B:>7}  {w:<7}  {med * 1e6:>9.1f}  {min(t) * 1e6:>9.1f}  {max(t) * 1e6:>9.1f}  {nbytes / med / 1e9:>12.1f}  {ref / med:>9.3f}  {ok[w]}")
            all_ok = all_ok and all(ok.values())

    B = a.noise_images
    records = records_for(B)
    gen = torch.Generator(device="cuda").manual_seed(3)
    lines += [f"# bits recovered of {B} x {M} = {B * M}: {B} images of 4x64x64 under their own records, z' = fp16(z + sigma n), n drawn on the device; "
              "sign = gsw_extract_keyed(l), levels = gsw_extract_soft_l with soft.window_thresholds (clip 2.5)",
              "#  l   sigma   sign_vote   3_levels   15_levels   15_levels - sign"]
    for l in (2, 4):
        clean = codec.embed_records(records, mb, shape, seed=2, dtype=torch.float32, l=l)
        for sigma in (0.5, 1.0, 2.0):
            z = (clean + sigma * torch.randn(clean.shape, generator=gen, device="cuda")).to(torch.float16)
            sign = int(codec.extract_records(z, records, mb, l=l)[2].sum())
            lv = {t: int(codec.extract_soft_l(z, records, mb, soft.window_thresholds(z, l, t), l).matches.sum()) for t in (3, 15)}
            lines.append(f"{l:>4} {sigma:>7.1f}  {sign:>10}  {lv[3]:>9}  {lv[15]:>10}  {lv[15] - sign:>17}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
