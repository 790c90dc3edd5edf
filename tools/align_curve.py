#!/usr/bin/env python3
"""What the alignment search is worth through the real pipeline: generate watermarked images, mirror them, turn them by quarters or translate them
by a multiple of the VAE's 8 pixels, invert, and run `detect.detect_latents` with and without `align`.

    python tools/align_curve.py --model_id <checkpoint dir> [--images 8] [--out profiles/align_curve.txt]
    python tools/align_curve.py --allow_synthetic_weights ...      # plumbing only: the file then says so on its first line

Images: `GaussianShadingPipeline.txt2img` on the empty prompt (guidance 1), 512 x 512, DDIM at --steps for sampling and inversion, under one key of
a keyring of --keys keys.  Attacks: `imaging.pointwise(.., "horizontal_flip" / "vertical_flip")`, `imaging.rotate(.., 90 / 180 / 270)` (the device twins of the
distortions tool) and a cyclic translation of the pixels by (8, 0), (0, 16) and (16, -8).  Candidates: `align.alignments("d4", 2, 64, 64)`, 200 per
image.  Per attack: how many images name the right key at --fpr with and without the search, the median log10 p of the right key's bound, the mean
bit accuracy of the message read, and how many images report the alignment that undoes the attack on the lattice.
How much of the vote survives a flip depends on how symmetric the trained VAE and UNet are; synthetic weights are neither an autoencoder nor a
denoiser, and the numbers of such a run say nothing about that.  Needs a GPU."""
import argparse
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model_id", default="stabilityai/stable-diffusion-2-1-base")
    ap.add_argument("--allow_synthetic_weights", action="store_true")
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--keys", type=int, default=12)
    ap.add_argument("--fpr", type=float, default=1e-6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_curve.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import gswm_amd  # noqa: F401
    from gswm_amd import align as AL, codec, detect as D, extract as X, imaging
    from gswm_amd.pipeline import GaussianShadingPipeline
    if not torch.cuda.is_available():
        raise SystemExit("align_curve: no GPU; the pipeline has no CPU path")
    rng = np.random.default_rng(419)
    ring = D.Keyring()
    for u in range(a.keys):
        ring.add(f"key-{u}", bytes(rng.integers(0, 256, 32, dtype=np.uint8)), bytes(rng.integers(0, 256, 16, dtype=np.uint8)))
    own = a.keys // 2
    key, nonce = ring.row_at(own)
    msg = codec.pad_message("lthero", 32)
    B, H, W, M = a.images, 512, 512, 256
    args = types.SimpleNamespace(model_id=a.model_id, allow_synthetic_weights=a.allow_synthetic_weights, width=W, height=H, num_inference_steps=a.steps,
                                 scheduler="DDIM", strict_kernels=None)
    synthetic = X._no_checkpoint(a.model_id)
    cands = AL.alignments("d4", 2, H // 8, W // 8)
    # attack -> (the image transform, the lattice transform it is expected to be: apply(lattice, that) models the attacked latent)
    attacks = [("none", lambda x: x, (0, 0, 0)),
               ("horizontal_flip", lambda x: imaging.pointwise(x, "horizontal_flip"), (4, 0, 0)),
               ("vertical_flip", lambda x: imaging.pointwise(x, "vertical_flip"), (6, 0, 0)),
               ("rotation 90", lambda x: imaging.rotate(x, 90), (1, 0, 0)),
               ("rotation 180", lambda x: imaging.rotate(x, 180), (2, 0, 0)),
               ("rotation 270", lambda x: imaging.rotate(x, 270), (3, 0, 0)),
               ("translate (8,0)", lambda x: torch.roll(x, (8, 0), (1, 2)), (0, 1, 0)),
               ("translate (0,16)", lambda x: torch.roll(x, (0, 16), (1, 2)), (0, 0, 2)),
               ("translate (16,-8)", lambda x: torch.roll(x, (16, -8), (1, 2)), (0, 2, -1))]
    lines = []
    with X._strictness(args, synthetic), torch.no_grad():
        models = X.load_models(a.model_id, allow_synthetic=X._synthetic_allowed(args))
        pipe = GaussianShadingPipeline(models.unet, key, nonce, msg, height=H, width=W, num_inference_steps=a.steps, dtype=models.dtype, ctx_uncond=models.ctx_empty,
                                       prediction_type=models.prediction_type)
        images, _, _ = pipe.txt2img(models.ctx_empty.expand(B, -1, -1), models.vae, seed=7, guidance_scale=1.0)
        u8 = imaging.tensor_to_image(images)
        for name, attack, lattice in attacks:
            z = X.invert_decoded_images(list(attack(u8).contiguous().cpu().numpy()), args)
            undo = AL.inverse(lattice, H // 8, W // 8)
            cols = []
            for res in (D.detect_latents(z, ring, M, fpr=a.fpr), D.detect_latents(z, ring, M, fpr=a.fpr, align=cands)):
                named = sum(r.key_id == f"key-{own}" for r in res)
                wrong = sum(r.key_id not in (None, f"key-{own}") for r in res)
                best = float(np.median([r.candidates[0].log10_p_any for r in res]))
                acc = [np.mean(np.unpackbits(np.frombuffer(r.message, dtype=np.uint8)) == np.unpackbits(np.frombuffer(msg, dtype=np.uint8))) for r in res if r.message]
                found = sum(r.alignment == undo for r in res)
                cols.append(f"named {named}/{B} wrong {wrong}   median log10 p {best:9.1f}   bit accuracy {np.mean(acc) if acc else float('nan'):.4f}   undoing alignment {found}/{B}")
            lines.append(f"{name:<18} plain: {cols[0]}\n{'':<18} align: {cols[1]}")
            print(lines[-1], flush=True)
    head = [("SYNTHETIC WEIGHTS: plumbing only, these figures say nothing about a real VAE / UNet.  " if synthetic else "") +
            f"tools/align_curve.py --model_id {a.model_id} --images {B} --steps {a.steps} --keys {a.keys} --fpr {a.fpr}   ({torch.cuda.get_device_name(0)})",
            f"512 x 512, 256-bit message, l = 1, empty prompt at guidance 1, key {own} of {a.keys}; plain = detect_latents, align = detect_latents(align=alignments('d4', 2, 64, 64)), "
            f"{len(cands)} candidates, Bonferroni over {a.keys * len(cands)} pairs; named = the right key at fpr {a.fpr}, wrong = another key named; bit accuracy over the images "
            "that name a key; undoing alignment = the reported alignment is the lattice inverse of the attack (plain reports none)"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(head + lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
