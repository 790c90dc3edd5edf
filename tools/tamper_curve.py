#!/usr/bin/env python3
"""What the tile map and the tile-weighted vote are worth through the real pipeline: generate watermarked images, attack them with `erasing`,
`randomcrop` and `resizedcrop` at the strength table's values, invert, and compare the plain vote with `--robust 1`; next to it, the share of
tiles the known-message map calls intact inside and outside the attacked area.

    python tools/tamper_curve.py --model_id <checkpoint dir> [--images 8] [--strengths 0.1,0.3,0.5,0.7,0.9] [--out profiles/tamper_curve.txt]
    python tools/tamper_curve.py --allow_synthetic_weights ...      # plumbing only: the file then says so on its first line

Images: `GaussianShadingPipeline.txt2img` on the empty prompt (guidance 1), 512 x 512, DDIM at --steps for sampling and inversion.  Attacks:
`gswm_amd.distortions.apply_distortion` at RELATIVE strengths of its table (distortion_strength_paras), image b with seed b.  The attacked area
is recomputed from the same seeds: the erased box, everything outside the kept crop, or (resizedcrop) the whole image, since every pixel moves.
A tile counts as inside / outside when all of its 8 tile x 8 tile pixels are; tiles the box cuts through are left out of both shares.
Synthetic weights are not an autoencoder and not a denoiser: the numbers of such a run say nothing about how far an edit spreads through the VAE
and the UNet.  Needs a GPU."""
import argparse
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ATTACKS = ("erasing", "randomcrop", "resizedcrop")
KEY = "5822ff9cce6772f714192f43863f6bad1bf54b78326973897e6b66c3186b77a7"
NONCE = "05072fd1c2265f6f2e2a4080a2bfbdd8"


def attacked_pixels(kind, H, W, s, seed):
    """bool [H, W]: the pixels the attack replaced, from the parameters `distortions._geometric` draws for this seed"""
    import numpy as np
    from gswm_amd import distortions as D, imaging
    mask = np.zeros((H, W), dtype=bool)
    if kind == "resizedcrop":
        mask[:] = True
    elif kind == "erasing":
        box = imaging.erasing_params(H, W, s, D._generator(seed))
        if box is not None:
            mask[box[0]:box[0] + box[2], box[1]:box[1] + box[3]] = True
    else:
        i, j, h, w = imaging.resized_crop_params(H, W, s, D._generator(seed))
        mask[:] = True
        mask[i:i + h, j:j + w] = False
    return mask


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model_id", default="stabilityai/stable-diffusion-2-1-base")
    ap.add_argument("--allow_synthetic_weights", action="store_true")
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--strengths", default="0.1,0.3,0.5,0.7,0.9")
    ap.add_argument("--tile", type=int, default=8, choices=(8, 16, 32))
    ap.add_argument("--fpr", type=float, default=1e-6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tamper_curve.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import gswm_amd  # noqa: F401
    from gswm_amd import codec, distortions as D, extract as X, imaging, tamper
    from gswm_amd.pipeline import GaussianShadingPipeline
    if not torch.cuda.is_available():
        raise SystemExit("tamper_curve: no GPU; the pipeline has no CPU path")
    key, nonce, msg = bytes.fromhex(KEY), bytes.fromhex(NONCE), codec.pad_message("lthero", 32)
    B, H, W, M, T = a.images, 512, 512, 256, a.tile
    args = types.SimpleNamespace(model_id=a.model_id, allow_synthetic_weights=a.allow_synthetic_weights, width=W, height=H, num_inference_steps=a.steps,
                                 scheduler="DDIM", strict_kernels=None)
    synthetic = X._no_checkpoint(a.model_id)
    lines = []
    with X._strictness(args, synthetic), torch.no_grad():
        models = X.load_models(a.model_id, allow_synthetic=X._synthetic_allowed(args))
        pipe = GaussianShadingPipeline(models.unet, key, nonce, msg, height=H, width=W, num_inference_steps=a.steps, dtype=models.dtype, ctx_uncond=models.ctx_empty,
                                       prediction_type=models.prediction_type)
        images, _, _ = pipe.txt2img(models.ctx_empty.expand(B, -1, -1), models.vae, seed=7, guidance_scale=1.0)
        u8 = imaging.tensor_to_image(images)

        def measure(batch_u8):
            z = X.invert_decoded_images(list(batch_u8.cpu().numpy()), args)
            plain = codec.bit_matches(codec.extract_batch(z, key, nonce, M)[0], M, msg).float().mean().item() / M
            robust = codec.bit_matches(tamper.extract_robust(z, key, nonce, M, tile=T)[0], M, msg).float().mean().item() / M
            return plain, robust, tamper.tamper_map(z, key, nonce, msg, tile=T, fpr=a.fpr)

        plain, robust, maps = measure(u8)
        share = np.mean([m.intact.mean() for m in maps if not isinstance(m, Exception)] or [float("nan")])
        lines.append(f"{'none':<12} {0.0:>8.2f} {0.0:>8.2f}   plain {plain:.4f}   robust {robust:.4f}   intact inside   -      outside {share:.3f}")
        for kind in ATTACKS:
            for rel in (float(s) for s in a.strengths.split(",")):
                s_abs = D.relative_strength_to_absolute(rel, kind)
                att = D.apply_distortion(u8, kind, rel, distortion_seed=0, same_operation=False, relative_strength=True)
                plain, robust, maps = measure(att)
                inside, outside = [], []
                for b, m in enumerate(maps):
                    if isinstance(m, Exception):
                        continue
                    px = attacked_pixels(kind, H, W, s_abs, b).reshape(H // (8 * T), 8 * T, W // (8 * T), 8 * T)
                    full, none = px.all(axis=(1, 3)), ~px.any(axis=(1, 3))
                    inside += m.intact[full].tolist()
                    outside += m.intact[none].tolist()
                fi = f"{np.mean(inside):.3f}" if inside else "  -  "
                fo = f"{np.mean(outside):.3f}" if outside else "  -  "
                lines.append(f"{kind:<12} {rel:>8.2f} {s_abs:>8.2f}   plain {plain:.4f}   robust {robust:.4f}   intact inside {fi}   outside {fo}")
                print(lines[-1], flush=True)
    head = [("SYNTHETIC WEIGHTS: plumbing only, these figures say nothing about a real VAE / UNet.  " if synthetic else "") +
            f"tools/tamper_curve.py --model_id {a.model_id} --images {B} --steps {a.steps} --tile {T} --fpr {a.fpr}   ({torch.cuda.get_device_name(0)})",
            "512 x 512, 256-bit message, l = 1, empty prompt at guidance 1; plain / robust = mean bit accuracy of extract_batch / extract_robust(iters=2); "
            "intact = share of tiles the known-message map proves present, inside / outside the attacked area (tiles the edge cuts are in neither)",
            "attack       relative absolute"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(head + lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
