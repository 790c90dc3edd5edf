#!/usr/bin/env python3
"""Launch times of the tile agreement map, the tile-weighted vote and the robust decode against the plain vote, interleaved in one run on one device.

    python tools/tamper_bench.py [--batches 1,16,256] [--rounds 30] [--out profiles/tamper_bench.txt]

Shape: latents of 4x64x64 fp16 with a planted 256-bit message and the top 48 rows replaced by noise, l = 1, tile 8.  Every round times, one after the
other with device events: `extract_batch` (the yardstick: the vote every earlier commit ships, on the same inputs), `quant_pack`, `tile_agreement`,
`vote_tiled` and `tamper.extract_robust(iters=2)` (1 pack + 3 votes + 3 maps).  The report is the median over the rounds and the spread (min .. max);
interleaving puts every row of a batch size under the same clocks and the same neighbours.  Needs a GPU: there is no CPU path to time.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROWS = ("extract_batch", "quant_pack", "tile_agreement", "vote_tiled", "extract_robust")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", default="1,16,256")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tamper_bench.txt"))
    a = ap.parse_args()
    import torch
    import gswm_amd  # noqa: F401
    from gswm_amd import codec, tamper
    if not torch.cuda.is_available():
        raise SystemExit("tamper_bench: no GPU; nothing is measured on a CPU")
    key = bytes.fromhex("5822ff9cce6772f714192f43863f6bad1bf54b78326973897e6b66c3186b77a7")
    nonce = bytes.fromhex("05072fd1c2265f6f2e2a4080a2bfbdd8")
    msg = codec.pad_message("lthero", 32)
    shape, M, tile = (4, 64, 64), 256, 8
    lines = [f"# tools/tamper_bench.py --batches {a.batches} --rounds {a.rounds}: B x 4x64x64 fp16, 256-bit message, l = 1, tile 8, the top 48 rows replaced by noise",
             f"# device: {torch.cuda.get_device_name(0)}; the five rows of a batch size interleaved per round; median of {a.rounds} rounds (min .. max)",
             "#     B  launch           median_us   min_us   max_us   vs_extract_batch   bits_right(plain -> robust)"]
    ok = True
    for B in (int(b) for b in a.batches.split(",")):
        z = codec.embed_batch(key, nonce, msg, B, shape, seed=1, dtype=torch.float16, fast=True)
        z[:, :, :48, :] = torch.randn((B, 4, 48, 64), device="cuda", dtype=torch.float16)
        keys = tamper.keys_tensor([(key, nonce)] * B, "cuda")
        msgs = tamper._message_rows([msg] * B, M, "cuda")
        packed, _ = codec.quant_pack(z, 1)
        weights = tamper.default_weights(codec.tile_agreement(packed, keys, msgs, M, shape, 1, tile), 256)
        calls = {"extract_batch": lambda: codec.extract_batch(z, key, nonce, M),
                 "quant_pack": lambda: codec.quant_pack(z, 1),
                 "tile_agreement": lambda: codec.tile_agreement(packed, keys, msgs, M, shape, 1, tile),
                 "vote_tiled": lambda: codec.vote_tiled(packed, keys, weights, M, shape, 1, tile),
                 "extract_robust": lambda: tamper.extract_robust(z, key, nonce, M, tile=tile, iters=2)}
        times = {name: [] for name in ROWS}
        for r in range(a.warmup + a.rounds):
            for name in ROWS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                calls[name]()
                e1.record()
                torch.cuda.synchronize()
                if r >= a.warmup:
                    times[name].append(e0.elapsed_time(e1) * 1e-3)
        plain = int(codec.bit_matches(calls["extract_batch"]()[0], M, msg).sum())
        robust = int(codec.bit_matches(calls["extract_robust"]()[0], M, msg).sum())
        ok = ok and robust >= plain
        base = statistics.median(times["extract_batch"])
        for name in ROWS:
            t = times[name]
            med = statistics.median(t)
            lines.append(f"{B:>7}  {name:<15}  {med * 1e6:>9.1f}  {min(t) * 1e6:>7.1f}  {max(t) * 1e6:>7.1f}  {med / base:>16.2f}   {plain}/{M * B} -> {robust}/{M * B}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
