#!/usr/bin/env python3
"""What the extra capacity of l > 1 costs in robustness: bit accuracy of the codec under Gaussian noise on the latent.

    python tools/codec_l_noise_curve.py [--images 256] [--out profiles/codec_l_noise_curve.txt]

For l = 1, 2, 4: embed `--images` latents of 4x64x64 (fp32, exact core, in-kernel Philox stream) carrying a 256-bit message, disturb them as
z' = (z + sigma n) / sqrt(1 + sigma^2) with n ~ N(0, 1) (the latent stays standard normal, as an inverted image's does), extract with the
same l.  Reported per sigma: the fraction of cipher bits read back right per element (before the vote; from quant_pack against a noiseless
quant_pack) and the fraction of message bits right after the vote over 64 l copies.  A measurement, nothing is asserted on it.  Needs a GPU.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIGMAS = (0.0, 0.25, 0.5, 1.0, 1.5, 2.0, 3.0)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "codec_l_noise_curve.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import gswm_amd  # noqa: F401
    from gswm_amd import codec
    if not torch.cuda.is_available():
        raise SystemExit("codec_l_noise_curve: no GPU")
    key = bytes.fromhex("5822ff9cce6772f714192f43863f6bad1bf54b78326973897e6b66c3186b77a7")
    nonce = bytes.fromhex("05072fd1c2265f6f2e2a4080a2bfbdd8")
    k = codec.pad_message("lthero", 32)
    B, shape, M = a.images, (4, 64, 64), 256
    g = torch.Generator(device="cuda").manual_seed(0)
    noise = torch.randn((B, *shape), generator=g, device="cuda", dtype=torch.float32)
    popcount = torch.tensor([bin(i).count("1") for i in range(256)], device="cuda")
    lines = [f"# tools/codec_l_noise_curve.py --images {B}: 4x64x64 fp32 latents, 256-bit message, z' = (z + sigma n) / sqrt(1 + sigma^2), device {torch.cuda.get_device_name(0)}",
             "# element: cipher bits read back right, before the vote; voted: message bits right after the majority over `copies`; images: share of images whose",
             "# whole message comes back",
             "# l  copies  sigma   element_bit_acc   voted_bit_acc   images_all_bits"]
    for l in (1, 2, 4):
        z = codec.embed_batch(key, nonce, k, B, shape, seed=7, dtype=torch.float32, l=l)
        clean, _ = codec.quant_pack(z, l)
        copies = codec.vote_copies(16384, M, l)
        for s in SIGMAS:
            zn = ((z + s * noise) / float(np.sqrt(1.0 + s * s))).contiguous()
            packed, _ = codec.quant_pack(zn, l)
            wrong = popcount[(packed ^ clean).long()].sum().item()
            elem = 1.0 - wrong / (B * 16384 * l)
            bits, flags = codec.extract_batch(zn, key, nonce, M, l=l)
            match = codec.bit_matches(bits, M, k)
            lines.append(f"{l:>3}  {copies:>6}  {s:>5.2f}  {elem:>16.6f}  {match.float().mean().item() / M:>14.6f}  {(match == M).float().mean().item():>16.4f}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
