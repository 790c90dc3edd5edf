"""Twin of the reference's `distortions` tool (the robustness attacks of its README) on device batches.

    python -m gswm_amd.distortions --input_dir D --output_dir_base O --distortion_type rotation --strength 0.5 --relative_strength

Same strength table, seeding and CLI flags as the reference.  Every attack but two runs as HIP kernels through `imaging`, one launch per
batch (two for the crop and resize), bit-exact against Pillow: the ten point-wise / resampling / JPEG types of `imaging.apply_distortion`
and the four geometric ones (rotation, resizedcrop, erasing, randomcrop), whose random parameters are drawn on the host from torch's
CPU generator seeded the way the reference seeds it (`set_random_seed(seed)` -> `torch.manual_seed(seed)`).  "elastic" (torchvision v2's
float grid_sample on a random field) and "reversed" (a whole diffusion inversion) are refused.

Seeding: `apply_distortion` on a batch gives image b the seed `distortion_seed + b`, or `distortion_seed` for every image when
`same_operation` is set (distortions:69-79).  The CLI hands the reference one image per call, so there every file uses `distortion_seed`.
"""
from __future__ import annotations

import argparse
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import imaging

# distortions:17-34
distortion_strength_paras = dict(
    rotation=(0, 360),
    scaling=(0, 1),
    resizedcrop=(1, 0.1),
    erasing=(0, 1),
    brightness=(1, 16),
    contrast=(1, 6),
    blurring=(0, 20),
    noise=(0, 0.5),
    compression=(100, 0),
    reversed=(0, 100),
    elastic=(0, 100),
    horizontal_flip=(0, 0),
    vertical_flip=(0, 0),
    togray=(0, 0),
    randomcrop=(1, 0),
    invert=(0, 0),
)

# distortions:330-346: the add2one chain (only rotation enabled)
Distortion_types_need2deal = {
    "rotation": {"relative_strength": 0.5, "enable": 1},
    "scaling": {"relative_strength": 0.3, "enable": 0},
    "resizedcrop": {"relative_strength": 0.5, "enable": 0},
    "erasing": {"relative_strength": 0.5, "enable": 0},
    "brightness": {"relative_strength": 0.5, "enable": 0},
    "contrast": {"relative_strength": 0.5, "enable": 0},
    "blurring": {"relative_strength": 0.5, "enable": 0},
    "noise": {"relative_strength": 0.5, "enable": 0},
    "compression": {"relative_strength": 0.3, "enable": 0},
    "elastic": {"relative_strength": 0.5, "enable": 0},
    "horizontal_flip": {"relative_strength": 0.5, "enable": 0},
    "vertical_flip": {"relative_strength": 0.5, "enable": 0},
    "togray": {"relative_strength": 0.5, "enable": 0},
    "randomcrop": {"relative_strength": 0.3, "enable": 0},
    "invert": {"relative_strength": 0.5, "enable": 0},
}

GEOMETRIC = ("rotation", "resizedcrop", "erasing", "randomcrop")
NOT_ON_DEVICE = ("elastic", "reversed")
IMAGE_EXTENSIONS = (".png", ".jpg", ".jpeg")


def relative_strength_to_absolute(strength: float, distortion_type: str) -> float:
    """distortions:37-49."""
    assert 0 <= strength <= 1
    lo, hi = distortion_strength_paras[distortion_type]
    s = strength * (hi - lo) + lo
    s = max(s, min(lo, hi))
    return min(s, max(lo, hi))


def _seeds(B: int, distortion_seed: int, same_operation: bool) -> List[int]:
    return [distortion_seed if same_operation else distortion_seed + b for b in range(B)]


def _generator(seed: int) -> torch.Generator:
    # set_random_seed(seed) starts with torch.manual_seed(seed + 0); a private generator seeded alike gives the same draws
    return torch.Generator().manual_seed(seed)


def _geometric(images: torch.Tensor, distortion_type: str, s: float, seeds: List[int], out: str) -> torch.Tensor:
    B, H, W, _ = images.shape
    if distortion_type == "rotation":                                       # distortions:107-113
        return imaging.rotate(images, s, out=out)
    if distortion_type == "erasing":                                        # distortions:126-137
        boxes = [imaging.erasing_params(H, W, s, _generator(sd)) or (0, 0, 0, 0) for sd in seeds]    # None: the image unchanged
        return imaging.box_mask(images, boxes, keep_inside=False, out=out)
    params = [imaging.resized_crop_params(H, W, s, _generator(sd)) for sd in seeds]
    if distortion_type == "randomcrop":                                     # distortions:207-222
        return imaging.box_mask(images, params, keep_inside=True, out=out)
    # distortions:115-124: F.resized_crop(img, i, j, h, w, image.size) reads (W, H) as [height, width]: the output is H wide, W high
    sizes = {(h, w) for _, _, h, w in params}
    assert len(sizes) == 1, sizes                                           # (h, w) depends on (H, W, s) only
    return imaging.crop_resize(images, [(i, j) for i, j, _, _ in params], sizes.pop(), (H, W), filter="bilinear", out=out)


def apply_distortion(images: torch.Tensor, distortion_type: str, strength: Optional[float] = None, distortion_seed: int = 0,
                     same_operation: bool = False, relative_strength: bool = True, out: str = "u8") -> torch.Tensor:
    """distortions:52-83 on a uint8 [B, H, W, 3] device batch -> a batch of the `out` kind ('u8', 'f16', 'f32').  Unlike the reference,
    the geometric types need a strength (the reference would draw one from Python's `random`)."""
    if distortion_type in NOT_ON_DEVICE:
        raise ValueError(f"distortion type {distortion_type!r} is not implemented on the device (elastic and reversed are out of scope)")
    if distortion_type not in distortion_strength_paras:
        raise ValueError(f"unknown distortion type {distortion_type!r}")
    if distortion_type not in GEOMETRIC:
        return imaging.apply_distortion(images, distortion_type, strength, distortion_seed=distortion_seed, relative_strength=relative_strength,
                                        out=out)
    if strength is None:
        raise ValueError(f"distortion type {distortion_type!r} needs a strength")
    images = imaging._check_images(images)
    if relative_strength:
        strength = relative_strength_to_absolute(strength, distortion_type)
    lo, hi = distortion_strength_paras[distortion_type]
    assert min(lo, hi) <= strength <= max(lo, hi)
    return _geometric(images, distortion_type, strength, _seeds(images.shape[0], distortion_seed, same_operation), out)


def apply_multiple_distortions(images: torch.Tensor, distortion_params: Dict = Distortion_types_need2deal, distortion_seed: int = 0,
                               out: str = "u8") -> Tuple[torch.Tensor, Dict[str, float]]:
    """distortions:348-359 (the add2one chain) on a batch: every enabled type in table order at its relative strength, the seed + 1 per
    enabled type; every image of the batch is one file of the reference's loop, so all of them use the same seed chain."""
    seed = distortion_seed
    applied = {}
    for distortion_type, params in distortion_params.items():
        if params["enable"]:
            strength = relative_strength_to_absolute(params["relative_strength"], distortion_type)
            images = apply_distortion(images, distortion_type, strength, distortion_seed=seed, same_operation=True, relative_strength=False)
            applied[distortion_type] = strength
            seed += 1
    return (images if out == "u8" else imaging.to_tensor(images, out=out)), applied


def create_output_dir(base_dir: str, strengths: Dict[str, float]) -> str:
    """distortions:361-366."""
    output_dir = os.path.join(base_dir, "_".join(f"{key}_{round(value, 2)}" for key, value in strengths.items()))
    os.makedirs(output_dir, exist_ok=True)
    return output_dir


def output_dir_name(distortion_type: str, strength: float, relative_strength: bool = True) -> str:
    """distortions:252-254: f"{type}_{round(strength, 2)}" of the absolute strength (the reference only names the relative case)."""
    s = relative_strength_to_absolute(strength, distortion_type) if relative_strength else strength
    return f"{distortion_type}_{round(s, 2)}"


def list_images(input_dir: str) -> List[str]:
    return [f for f in os.listdir(input_dir) if f.lower().endswith(IMAGE_EXTENSIONS)]


def _decode(path: str) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        if im.mode != "RGB":
            raise ValueError(f"{path}: mode {im.mode!r}, the device attacks take RGB images")
        return np.asarray(im, dtype=np.uint8).copy()


def _run_files(paths: List[str], fn, device: str = "cuda"):
    """Decode `paths` on host threads, send the files of one size to the device as one batch, and yield (path, uint8 [h, w, 3]) of
    fn(batch) for every file."""
    from concurrent.futures import ThreadPoolExecutor
    # PIL releases the GIL while it reads and decodes (as in extract.py)
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        arrs = list(pool.map(_decode, paths))
    groups: Dict[tuple, List[int]] = {}
    for k, a in enumerate(arrs):
        groups.setdefault(a.shape, []).append(k)
    for idx in groups.values():
        res = fn(torch.from_numpy(np.stack([arrs[k] for k in idx])).to(device)).cpu().numpy()
        for n, k in enumerate(idx):
            yield paths[k], res[n]


def _save(arr: np.ndarray, path: str):
    from PIL import Image
    Image.fromarray(arr).save(path)                                         # by extension, as the reference saves (a .jpg re-encodes)


def process_images_in_directory(input_dir: str, output_dir_base: str, distortion_type: str, strength: Optional[float] = None,
                                distortion_seed: int = 0, same_operation: bool = False, relative_strength: bool = True) -> str:
    """distortions:241-281: every .png / .jpg / .jpeg of `input_dir` attacked and saved under the same name in
    `output_dir_base/{type}_{round(absolute strength, 2)}`.  The reference attacks one file per call, so every file uses
    `distortion_seed` (`same_operation` changes nothing here).  Returns the output directory."""
    output_dir = os.path.join(output_dir_base, output_dir_name(distortion_type, strength, relative_strength))
    os.makedirs(output_dir, exist_ok=True)
    names = list_images(input_dir)
    fn = lambda batch: apply_distortion(batch, distortion_type, strength=strength, distortion_seed=distortion_seed, same_operation=True,
                                        relative_strength=relative_strength)
    for path, arr in _run_files([os.path.join(input_dir, f) for f in names], fn):
        _save(arr, os.path.join(output_dir, os.path.basename(path)))
    return output_dir


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(
        description="Apply distortions to images in a directory (on the GPU).",
        epilog="Divergence from the reference: without --relative_strength the reference's process_images_in_directory fails with a "
               "NameError (it names the output directory only on the relative branch); here the directory is named after the absolute "
               "strength. 'elastic' and 'reversed' are refused.")
    parser.add_argument("--input_dir", required=True, type=str, help="Directory containing the input images.")
    parser.add_argument("--output_dir_base", required=True, type=str, help="Base directory for saving output images.")
    parser.add_argument("--distortion_type", type=str, choices=list(distortion_strength_paras.keys()), help="Type of distortion to apply.")
    parser.add_argument("--strength", type=float, default=None, help="Strength of the distortion (optional).")
    parser.add_argument("--sgstart", type=float, default=0.1, help="Start strength for looping (optional).")
    parser.add_argument("--sgend", type=float, default=1, help="End strength for looping (optional).")
    parser.add_argument("--distortion_seed", type=int, default=0, help="Seed for random distortion (optional).")
    parser.add_argument("--same_operation", action="store_true", help="Apply the same distortion to all images (optional).")
    parser.add_argument("--relative_strength", action="store_true",
                        help="Use relative strength for distortion (optional). Without it the strength is absolute and names the output "
                             "directory (the reference fails there with a NameError).")
    parser.add_argument("--add2one", action="store_true", help="Add all distortion to one pic (optional).")
    return parser


def main(argv: Optional[List[str]] = None) -> int:
    """distortions:370-434."""
    args = build_parser().parse_args(argv)
    run = dict(distortion_seed=args.distortion_seed, same_operation=args.same_operation, relative_strength=args.relative_strength)
    if args.add2one:
        names = list_images(args.input_dir)
        if not names:
            print("No image files found in the input directory.")
            return 1
        applied = {}

        def chain(batch):
            res, strengths = apply_multiple_distortions(batch, Distortion_types_need2deal, args.distortion_seed)
            applied.update(strengths)
            return res

        for path, arr in _run_files([os.path.join(args.input_dir, f) for f in names], chain):
            _save(arr, os.path.join(create_output_dir(args.output_dir_base, applied), os.path.basename(path)))
    elif args.distortion_type and args.strength is not None:
        process_images_in_directory(args.input_dir, args.output_dir_base, args.distortion_type, strength=args.strength, **run)
    elif args.distortion_type:
        for s in np.arange(args.sgstart, args.sgend, 0.1):
            process_images_in_directory(args.input_dir, args.output_dir_base, args.distortion_type, strength=float(s), **run)
    else:
        for distortion_type, params in Distortion_types_need2deal.items():
            if params["enable"]:
                for s in np.arange(args.sgstart, args.sgend, 0.1):
                    process_images_in_directory(args.input_dir, args.output_dir_base, distortion_type, strength=float(s), **run)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
