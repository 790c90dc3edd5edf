#!/usr/bin/env python3
"""Embed + extract launch pair of the codec at l = 1, 2 and 4, interleaved in one run on one device.

    python tools/codec_l_bench.py [--images 16384] [--rounds 20] [--out profiles/codec_l_bench.txt]

Shape: `--images` latents of 4x64x64 fp16, a 256-bit message.  l = 1 runs gsw_embed / gsw_extract (the kernels every earlier commit ships),
l = 2, 4 run gsw_embed_l / gsw_extract_l.  The same bytes move at every l (the embed writes the latents, the extract reads them), so the
l = 1 pair of the same file is the yardstick for the other two.  Each round times the six launches one after the other with device
events; the report is the median over the rounds and the spread (min .. max).  Embed mode: the fp32 core on the in-kernel Philox stream
(what pipeline.embed runs).  Needs a GPU: there is no CPU path to time.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=16384)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec_l_bench.txt"))
    a = ap.parse_args()
    import torch
    import gswm_amd  # noqa: F401
    from gswm_amd import codec
    if not torch.cuda.is_available():
        raise SystemExit("codec_l_bench: no GPU; nothing is measured on a CPU")
    key = bytes.fromhex("5822ff9cce6772f714192f43863f6bad1bf54b78326973897e6b66c3186b77a7")
    nonce = bytes.fromhex("05072fd1c2265f6f2e2a4080a2bfbdd8")
    k = codec.pad_message("lthero", 32)
    B, shape, n, M = a.images, (4, 64, 64), 16384, 256
    z = torch.empty((B, *shape), dtype=torch.float16, device="cuda")
    nbytes = z.numel() * z.element_size()
    windows = (1, 2, 4)
    times = {(l, w): [] for l in windows for w in ("embed", "extract")}
    ok = {}

    def pair(l, record):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        codec.embed_batch(key, nonce, k, B, shape, seed=1, dtype=torch.float16, fast=True, out=z, l=l)
        e1.record()
        bits, flags = codec.extract_batch(z, key, nonce, M, l=l)
        e2.record()
        torch.cuda.synchronize()
        if record:
            times[(l, "embed")].append(e0.elapsed_time(e1) * 1e-3)
            times[(l, "extract")].append(e1.elapsed_time(e2) * 1e-3)
        return bits, flags

    for r in range(a.warmup + a.rounds):
        for l in windows:
            bits, flags = pair(l, r >= a.warmup)
            if r == 0:      # what is timed is also right: every image gives the message back
                ok[l] = int(flags.abs().sum()) == 0 and int(codec.bit_matches(bits, M, k).min()) == M
    lines = [f"# tools/codec_l_bench.py --images {B} --rounds {a.rounds}: {B} x 4x64x64 fp16 ({nbytes / 2**20:.0f} MiB), 256-bit message, embed fast/Philox",
             f"# device: {torch.cuda.get_device_name(0)}; interleaved l = 1, 2, 4 per round; median of {a.rounds} rounds (min .. max); bytes = the latents, once per launch",
             "# l  launch   median_us   min_us   max_us   GB/s(median)   vs_l1   round_trip_ok"]
    for l in windows:
        for w in ("embed", "extract"):
            t = times[(l, w)]
            med, base = statistics.median(t), statistics.median(times[(1, w)])
            lines.append(f"{l:>3}  {w:<7}  {med * 1e6:>9.1f}  {min(t) * 1e6:>7.1f}  {max(t) * 1e6:>7.1f}  {nbytes / med / 1e9:>12.1f}  {base / med:>6.3f}  {ok[l]}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0 if all(ok.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
