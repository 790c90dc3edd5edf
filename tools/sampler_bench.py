#!/usr/bin/env python3
"""DDIM-50 against DPM-Solver++ 2M at 20 and 25 sampling steps, end to end on one GPU: `GaussianShadingPipeline.roundtrip` (embed -> CFG sampling ->
50-step DDIM inversion -> vote) on the SD 2.1-shaped UNet with synthetic weights at batch 64, 8 and 1.  Prints images/s and the bits recovered per
configuration and writes the table to profiles/sampler_bench.txt.

    python tools/sampler_bench.py [--batches 64,8,1] [--steps 2] [--warmup 1] [--out profiles/sampler_bench.txt]

The parent never touches the GPU: every configuration runs in a child process of its own under its own time limit, and after a child that failed,
crashed or ran out of time nothing more is started."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONFIGS = (("ddim", 50), ("dpmpp_2m", 20), ("dpmpp_2m", 25))
KEY = "5822ff9cce6772f714192f43863f6bad1bf54b78326973897e6b66c3186b77a7"
NONCE = "05072fd1c2265f6f2e2a4080a2bfbdd8"


def worker(a):
    import torch
    import gswm_amd  # noqa: F401
    from gswm_amd import codec, unet as U
    from gswm_amd.pipeline import GaussianShadingPipeline
    dev, dtype, B = torch.device("cuda", 0), torch.float16, a.batch
    torch.cuda.set_device(dev)
    model = U.synthetic_init_(U.UNet2DCondition(), seed=0).to(dev, dtype).eval()
    g = torch.Generator(device="cpu").manual_seed(1)
    cu = torch.randn(1, 77, 1024, generator=g).to(dev, dtype)
    ct = torch.randn(B, 77, 1024, generator=g).to(dev, dtype)
    msg = codec.pad_message("lthero", 32)
    pipe = GaussianShadingPipeline(model, bytes.fromhex(KEY), bytes.fromhex(NONCE), msg, num_inference_steps=50, dtype=dtype, device=dev, ctx_uncond=cu,
                                   sampler=a.sampler, num_sampling_steps=a.sampling_steps)
    for i in range(a.warmup):
        pipe.roundtrip(B, ct, seed=2024, image_index0=i * B)
    torch.cuda.synchronize()
    matched = torch.zeros((), dtype=torch.int64, device=dev)
    flagged = torch.zeros((), dtype=torch.int64, device=dev)
    t0 = time.perf_counter()
    for i in range(a.steps):
        z_T, x0, bits, flags = pipe.roundtrip(B, ct, seed=2024, image_index0=(a.warmup + i) * B)
        matched += codec.bit_matches(bits, 256, msg).sum()
        flagged += (flags != 0).sum()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    agree = ((pipe.invert(x0) >= 0) == (z_T >= 0)).float().mean().item()
    print(json.dumps({"batch": B, "sampler": a.sampler, "sampling_steps": a.sampling_steps, "inversion_steps": 50, "images_per_s": B * a.steps / dt,
                      "s_per_roundtrip": dt / a.steps, "bits_recovered": int(matched), "bits_total": 256 * B * a.steps, "flagged_images": int(flagged),
                      "sign_agreement_last_batch": agree, "x0_finite": bool(torch.isfinite(x0).all()), "device": torch.cuda.get_device_name(0)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,8,1")
    ap.add_argument("--steps", type=int, default=2, help="timed round trips per configuration")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=float, default=240.0, help="time limit of one configuration's process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler_bench.txt"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--batch", type=int, default=64, help=argparse.SUPPRESS)
    ap.add_argument("--sampler", default="ddim", help=argparse.SUPPRESS)
    ap.add_argument("--sampling-steps", type=int, default=50, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    rows, lines = [], []
    for B in (int(b) for b in a.batches.split(",")):
        for sampler, S in CONFIGS:
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--batch", str(B), "--sampler", sampler, "--sampling-steps", str(S),
                   "--steps", str(a.steps), "--warmup", str(a.warmup)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                print(f"sampler_bench: batch {B} {sampler}/{S} exceeded its {a.timeout:.0f} s limit; stopping", file=sys.stderr)
                return 124
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                print(f"sampler_bench: batch {B} {sampler}/{S} exited with {r.returncode}; stopping", file=sys.stderr)
                return r.returncode if r.returncode > 0 else 1
            rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
            d = rows[-1]
            base = next(x for x in rows if x["batch"] == B and x["sampler"] == "ddim")
            lines.append(f"batch {B:3d}  {sampler:9s} {S:2d} sampling + 50 inversion steps  {d['images_per_s']:9.3f} images/s  x{d['images_per_s'] / base['images_per_s']:.2f} vs ddim/50  "
                         f"bits {d['bits_recovered']}/{d['bits_total']}  flagged {d['flagged_images']}  sign agreement {d['sign_agreement_last_batch']:.4f}")
            print(lines[-1], flush=True)
    head = [f"tools/sampler_bench.py --batches {a.batches} --steps {a.steps} --warmup {a.warmup}   ({rows[0]['device']}; SD 2.1-shaped UNet, synthetic weights, fp16, "
            f"512x512, guidance 7.5, 256-bit message; roundtrip = embed -> sampling -> 50-step DDIM inversion -> vote; no VAE)"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(head + lines + [""] + [json.dumps(r) for r in rows]) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
