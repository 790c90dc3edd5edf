#!/usr/bin/env python3
"""Launch times of the one-launch robust decode (`codec.decode_robust`) against the seven launches of `tamper.extract_robust`, interleaved in one run on one
device, and the bits each decoder recovers on the same damaged latents.

    python tools/robust_soft_bench.py [--batches 1,16,256] [--rounds 30] [--sigma 1.5] [--rows 48] [--out profiles/robust_soft_bench.txt]

Shape: latents of 4x64x64 fp16 with a planted 256-bit message, N(0, sigma^2) added and the top `rows` rows replaced by N(0, 1), l = 1, tile 8, 15 levels from
the image's RMS.  Every round times, one after the other with device events: `vote_tiled` and `extract_soft` (one launch each, the yardsticks),
`decode_robust` on packed rows without planes (P = 0) and with the four planes of 15 levels (P = 4), both at iters = 2, and the two whole calls from latents:
`tamper.extract_robust(iters=2)` (1 pack + 3 votes + 3 maps + torch glue) and `tamper.extract_robust_soft(iters=2)` (the table, 1 pack, 1 decode), the latter
also with the table given (`_table`: 1 pack, 1 decode) and with levels = 0 (`_L0`: `quant_pack` + 1 decode, what `extract_robust` computes).  The report
is the median over the rounds and the spread (min .. max); interleaving puts every row of a batch size under the same clocks and the same neighbours.  Then the
bits recovered by the plain vote, `extract_robust`, the soft vote and `extract_robust_soft` under both sign_rounds.  Needs a GPU: there is no CPU path to time.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROWS = ("vote_tiled", "extract_soft", "decode_robust_P0", "decode_robust_P4", "extract_robust", "extract_robust_soft", "extract_robust_soft_table", "extract_robust_soft_L0")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", default="1,16,256")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=1.5)
    ap.add_argument("--rows", type=int, default=48)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "robust_soft_bench.txt"))
    a = ap.parse_args()
    import torch
    import gswm_amd  # noqa: F401
    from gswm_amd import codec, soft, tamper
    if not torch.cuda.is_available():
        raise SystemExit("robust_soft_bench: no GPU; nothing is measured on a CPU")
    key = bytes.fromhex("5822ff9cce6772f714192f43863f6bad1bf54b78326973897e6b66c3186b77a7")
    nonce = bytes.fromhex("05072fd1c2265f6f2e2a4080a2bfbdd8")
    msg = codec.pad_message("lthero", 32)
    shape, M, tile, iters, levels = (4, 64, 64), 256, 8, 2, 15
    lines = [f"# tools/robust_soft_bench.py --batches {a.batches} --rounds {a.rounds} --sigma {a.sigma} --rows {a.rows}: B x 4x64x64 fp16, 256-bit message, l = 1, tile 8, "
             f"iters {iters}, {levels} levels; N(0, {a.sigma}^2) added, the top {a.rows} rows replaced by N(0, 1)",
             f"# device: {torch.cuda.get_device_name(0)}; the eight rows of a batch size interleaved per round; median of {a.rounds} rounds (min .. max)",
             "# decode_robust_P0 / _P4: the one launch on packed rows (no planes / four planes); extract_robust: the whole call, 1 pack + 3 votes + 3 maps;",
             "# extract_robust_soft: the whole call, the table (soft.uniform_thresholds, torch ops) + 1 pack + 1 decode; _table: the table given; _L0: levels = 0, quant_pack + 1 decode",
             "#     B  launch                     median_us   min_us   max_us   vs_extract_robust"]
    acc = ["# bits recovered on the same latents: plain vote | extract_robust(iters=2) | soft vote | extract_robust_soft sign_rounds=0 | sign_rounds=1",
           "#     B   of       plain   robust     soft    both0    both1"]
    g = torch.Generator(device="cuda").manual_seed(0)
    for B in (int(b) for b in a.batches.split(",")):
        z = codec.embed_batch(key, nonce, msg, B, shape, seed=1, dtype=torch.float32, fast=True)
        z = z + a.sigma * torch.randn(z.shape, device="cuda", generator=g)
        z[:, :, :a.rows, :] = torch.randn((B, 4, a.rows, 64), device="cuda", generator=g)
        z = z.half().contiguous()
        keys = tamper.keys_tensor([(key, nonce)] * B, "cuda")
        msgs = tamper._message_rows([msg] * B, M, "cuda")
        records = soft.shared_records(key, nonce, M // 8, B, "cuda")
        table = soft.uniform_thresholds(z, levels, 2.5)
        rows = codec.level_pack(z, table)
        assert rows.planes.shape[1] == 4
        weights = tamper.default_weights(codec.tile_agreement(rows.signs, keys, msgs, M, shape, 1, tile), 256)
        calls = {"vote_tiled": lambda: codec.vote_tiled(rows.signs, keys, weights, M, shape, 1, tile),
                 "extract_soft": lambda: codec.extract_soft(z, records, M // 8, table),
                 "decode_robust_P0": lambda: codec.decode_robust(rows.signs, None, keys, M, shape, 1, tile, iters, 0),
                 "decode_robust_P4": lambda: codec.decode_robust(rows.signs, rows.planes, keys, M, shape, 1, tile, iters, 0),
                 "extract_robust": lambda: tamper.extract_robust(z, key, nonce, M, tile=tile, iters=iters),
                 "extract_robust_soft": lambda: tamper.extract_robust_soft(z, key, nonce, M, tile=tile, iters=iters, levels=levels),
                 "extract_robust_soft_table": lambda: tamper.extract_robust_soft(z, key, nonce, M, tile=tile, iters=iters, thresholds=table),
                 "extract_robust_soft_L0": lambda: tamper.extract_robust_soft(z, key, nonce, M, tile=tile, iters=iters, levels=0)}
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
        base = statistics.median(times["extract_robust"])
        for name in ROWS:
            t = times[name]
            med = statistics.median(t)
            lines.append(f"{B:>7}  {name:<25}  {med * 1e6:>9.1f}  {min(t) * 1e6:>7.1f}  {max(t) * 1e6:>7.1f}  {med / base:>18.2f}")
        right = [int(codec.bit_matches(bits.contiguous(), M, msg).sum()) for bits in (
            codec.extract_batch(z, key, nonce, M)[0], calls["extract_robust"]()[0], calls["extract_soft"]().bits,
            tamper.extract_robust_soft(z, key, nonce, M, tile=tile, iters=iters, levels=levels, sign_rounds=0).bits,
            tamper.extract_robust_soft(z, key, nonce, M, tile=tile, iters=iters, levels=levels, sign_rounds=1).bits)]
        acc.append(f"{B:>7}  {M * B:>7}  " + "  ".join(f"{v:>7}" for v in right))
    text = "\n".join(lines + acc) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
