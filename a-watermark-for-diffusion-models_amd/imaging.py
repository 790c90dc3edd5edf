"""Image-side stages either side of the latent loops, on the device (csrc/gswm_image.hip).

Host-side mirror of what the reference does with PIL / torchvision on the CPU, one image at a time:

* `load_image` of extract.py:31-37 (Lanczos resize -> ToTensor) plus the `.to(float16)` / `2.*x - 1.` that follow (extract.py:48,40)
  -> `resize_lanczos(..., out="f16")`: the fp16 CHW batch the VAE encoder consumes, bit-identical to the reference's tensor.
* `decode_image` / numpy_to_pil of the generation pipeline -> `tensor_to_image`.
* the `distortions` tool (apply_single_distortion): "compression" (JPEG QF), "scaling", "blurring", "brightness", "contrast", "noise",
  "togray", "invert", "horizontal_flip", "vertical_flip" -> `apply_distortion`, same strength conventions (`relative_strength_to_absolute`).
* its geometric attacks, bit-exact against Pillow: "rotation" (`Image.rotate`, NEAREST) -> `rotation_coefficients` + `rotate`;
  "resizedcrop" (`crop().resize(BILINEAR)`) -> `resized_crop_params` + `crop_resize`; "erasing" and "randomcrop" -> `erasing_params` /
  `resized_crop_params` + `box_mask`.  The per-image parameters are drawn on the host from torch's CPU generator, as torchvision draws
  them; `distortions.py` is the twin of the whole tool on top of these.

Images are uint8 [B, H, W, 3] device tensors (np.asarray(PIL image) stacked).  There is no CPU fallback: every function launches the
HIP kernels of libgswm through the C ABI.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _native as N
from .codec import _dt, _stream_ptr

_MODES = {"u8": N.GSW_IMG_U8_HWC, "f16": N.GSW_IMG_F16_CHW, "f32": N.GSW_IMG_F32_CHW}
_PLANS: Dict[Tuple[int, int, str], Tuple[torch.Tensor, torch.Tensor, int]] = {}
_FILTER_PLANS: Dict[Tuple[int, int, int, str], Tuple[torch.Tensor, torch.Tensor, int]] = {}
_FILTERS = {"bilinear": N.GSW_RESAMPLE_BILINEAR, "lanczos": N.GSW_RESAMPLE_LANCZOS}


def _check_images(images: torch.Tensor):
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3 or not images.is_cuda:
        raise ValueError("images must be a uint8 [B, H, W, 3] device tensor")
    return images.contiguous()


def _alloc_out(B: int, H: int, W: int, out: str, device) -> torch.Tensor:
    if out == "u8":
        return torch.empty((B, H, W, 3), dtype=torch.uint8, device=device)
    if out == "f16":
        return torch.empty((B, 3, H, W), dtype=torch.float16, device=device)
    if out == "f32":
        return torch.empty((B, 3, H, W), dtype=torch.float32, device=device)
    raise ValueError("out must be 'u8', 'f16' or 'f32'")


def lanczos_plan_host(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray, int]:
    """Pillow's coefficient table for one axis (Resample.c precompute_coeffs + normalize_coeffs_8bpc), computed by libgswm on the host."""
    lib = N.lib()
    ksize = lib.gsw_lanczos_plan(in_size, out_size, None, None, 0)
    if ksize <= 0:
        N.check(-ksize)
    bounds = np.empty((out_size, 2), dtype=np.int32)
    kk = np.empty((out_size, ksize), dtype=np.int32)
    rc = lib.gsw_lanczos_plan(in_size, out_size, bounds.ctypes.data_as(C.c_void_p), kk.ctypes.data_as(C.c_void_p), kk.size)
    if rc <= 0:
        N.check(-rc)
    return bounds, kk, ksize


def _plan(in_size: int, out_size: int, device) -> Tuple[torch.Tensor, torch.Tensor, int]:
    k = (in_size, out_size, str(device))
    if k not in _PLANS:
        bounds, kk, ksize = lanczos_plan_host(in_size, out_size)
        _PLANS[k] = (torch.from_numpy(bounds).to(device), torch.from_numpy(kk).to(device), ksize)
    return _PLANS[k]


def resize_lanczos(images: torch.Tensor, size: Union[int, Tuple[int, int], None], *, out: str = "u8") -> torch.Tensor:
    """`pil_img.resize(size, Image.Resampling.LANCZOS)` for a batch (size = (width, height) as PIL takes it; None keeps the size),
    with the output conversion fused: out = 'u8' (PIL image), 'f32' (ToTensor) or 'f16' (the reference's VAE-encoder input)."""
    images = _check_images(images)
    B, H, W, _ = images.shape
    if size is None:
        size = (W, H)
    if isinstance(size, int):
        size = (size, size)
    Wo, Ho = int(size[0]), int(size[1])
    dev = images.device
    res = _alloc_out(B, Ho, Wo, out, dev)
    hb = hk = vb = vk = None
    hks = vks = 0
    if Wo != W:
        hb, hk, hks = _plan(W, Wo, dev)
    if Ho != H:
        vb, vk, vks = _plan(H, Ho, dev)
    tmp = torch.empty((B, H, Wo, 3), dtype=torch.uint8, device=dev) if (Wo != W and (Ho != H or out != "u8")) else None
    with torch.cuda.device(dev):
        N.check(N.lib().gsw_resize_lanczos(images.data_ptr(), B, H, W, res.data_ptr(), Ho, Wo, _MODES[out], tmp.data_ptr() if tmp is not None else None,
                                           hb.data_ptr() if hb is not None else None, hk.data_ptr() if hk is not None else None, hks,
                                           vb.data_ptr() if vb is not None else None, vk.data_ptr() if vk is not None else None, vks, _stream_ptr()))
    return res


def to_tensor(images: torch.Tensor, *, out: str = "f16") -> torch.Tensor:
    """ToTensor (+ fp16 cast and 2x-1 when out='f16') without resizing."""
    return resize_lanczos(images, None, out=out)


def tensor_to_image(x: torch.Tensor, *, denormalise: bool = False) -> torch.Tensor:
    """[B, 3, H, W] float tensor -> uint8 [B, H, W, 3] like numpy_to_pil: (x * 255).round(); denormalise=True first applies the
    pipeline's (x / 2 + 0.5).clamp(0, 1)."""
    if x.dim() != 4 or x.shape[1] != 3 or not x.is_cuda:
        raise ValueError("x must be a [B, 3, H, W] device tensor")
    x = x.contiguous()
    B, _, H, W = x.shape
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        N.check(N.lib().gsw_tensor_to_image(x.data_ptr(), _dt(x.dtype), B, H, W, 1 if denormalise else 0, out.data_ptr(), _stream_ptr()))
    return out


def jpeg_quant_tables(quality: int) -> Tuple[np.ndarray, np.ndarray]:
    lum = np.empty(64, dtype=np.uint8)
    chrom = np.empty(64, dtype=np.uint8)
    N.check(N.lib().gsw_jpeg_quant_tables(int(quality), lum.ctypes.data_as(C.c_void_p), chrom.ctypes.data_as(C.c_void_p)))
    return lum.reshape(8, 8), chrom.reshape(8, 8)


def jpeg_roundtrip(images: torch.Tensor, quality: int, *, out: str = "u8") -> torch.Tensor:
    """distortions:175-184: what `Image.open(BytesIO(image.save(format="JPEG", quality=q)))` decodes to, for a batch, on the device."""
    images = _check_images(images)
    B, H, W, _ = images.shape
    dev = images.device
    res = _alloc_out(B, H, W, out, dev)
    ws = torch.empty(N.lib().gsw_jpeg_workspace_bytes(B, H, W), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        N.check(N.lib().gsw_jpeg_roundtrip(images.data_ptr(), B, H, W, int(quality), res.data_ptr(), _MODES[out], ws.data_ptr(), _stream_ptr()))
    return res


def gaussian_blur_params(radius: float, passes: int = 3) -> Tuple[int, int, int]:
    """(box radius, ww, fw) Pillow derives from a Gaussian radius (BoxBlur.c), computed by libgswm on the host."""
    r, ww, fw = C.c_int(), C.c_uint32(), C.c_uint32()
    N.check(N.lib().gsw_gaussian_blur_params(float(radius), int(passes), C.byref(r), C.byref(ww), C.byref(fw)))
    return r.value, ww.value, fw.value


def gaussian_blur(images: torch.Tensor, radius: float) -> torch.Tensor:
    """distortions:157-164: `image.filter(ImageFilter.GaussianBlur(radius))` for a batch, bit-exact, on the device."""
    images = _check_images(images)
    B, H, W, _ = images.shape
    out, tmp = torch.empty_like(images), torch.empty_like(images)
    with torch.cuda.device(images.device):
        N.check(N.lib().gsw_gaussian_blur(images.data_ptr(), B, H, W, float(radius), out.data_ptr(), tmp.data_ptr(), _stream_ptr()))
    return out


_OPS = {"brightness": N.GSW_PW_BRIGHTNESS, "contrast": N.GSW_PW_CONTRAST, "invert": N.GSW_PW_INVERT, "togray": N.GSW_PW_GRAY,
        "horizontal_flip": N.GSW_PW_HFLIP, "vertical_flip": N.GSW_PW_VFLIP, "noise": N.GSW_PW_NOISE}


def pointwise(images: torch.Tensor, op: str, strength: float = 0.0, *, seed: int = 0, image_index0: int = 0, out: str = "u8") -> torch.Tensor:
    images = _check_images(images)
    B, H, W, _ = images.shape
    dev = images.device
    res = _alloc_out(B, H, W, out, dev)
    ws = torch.empty(B, dtype=torch.int64, device=dev) if op == "contrast" else None
    with torch.cuda.device(dev):
        N.check(N.lib().gsw_image_pointwise(images.data_ptr(), B, H, W, _OPS[op], float(strength), int(seed), int(image_index0), res.data_ptr(),
                                            _MODES[out], ws.data_ptr() if ws is not None else None, _stream_ptr()))
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# geometric attacks (distortions:107-137,207-222)
# ---------------------------------------------------------------------------------------------------------------------------------
def resample_plan_host(filter: str, in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray, int]:
    """Pillow's coefficient table for one axis and filter ('bilinear' or 'lanczos'), computed by libgswm on the host (gsw_resample_plan)."""
    lib, f = N.lib(), _FILTERS[filter]
    ksize = lib.gsw_resample_plan(f, in_size, out_size, None, None, 0)
    if ksize <= 0:
        N.check(-ksize)
    bounds = np.empty((out_size, 2), dtype=np.int32)
    kk = np.empty((out_size, ksize), dtype=np.int32)
    rc = lib.gsw_resample_plan(f, in_size, out_size, bounds.ctypes.data_as(C.c_void_p), kk.ctypes.data_as(C.c_void_p), kk.size)
    if rc <= 0:
        N.check(-rc)
    return bounds, kk, ksize


def _filter_plan(filter: str, in_size: int, out_size: int, device) -> Tuple[torch.Tensor, torch.Tensor, int]:
    k = (_FILTERS[filter], in_size, out_size, str(device))
    if k not in _FILTER_PLANS:
        bounds, kk, ksize = resample_plan_host(filter, in_size, out_size)
        _FILTER_PLANS[k] = (torch.from_numpy(bounds).to(device), torch.from_numpy(kk).to(device), ksize)
    return _FILTER_PLANS[k]


def _fix16(v: float) -> int:
    return math.floor(v * 65536.0 + 0.5)                                    # Geometry.c FIX


def rotation_coefficients(angle: float, W: int, H: int) -> np.ndarray:
    """int32 [6] coefficient row of gsw_affine_nearest for `img.rotate(angle, NEAREST, expand=False, center=None, fillcolor=0)` on a
    W x H image, restating Image.rotate and Geometry.c step by step: the angle is reduced mod 360; 0 degrees (a copy), 180 degrees and, on
    a square image, 90 / 270 degrees are Pillow's transpose fast paths, written as exact integer rows; every other angle builds the
    matrix from round(cos / sin(-radians(angle)), 15) about (W / 2, H / 2) and takes affine_fixed's 16.16 rounding.  When the sine
    rounds to zero (for example 1e-14 degrees) Pillow runs ImagingScaleAffine instead; with a cosine of exactly +-1 that is the same
    gather (tests/test_geom_host.py checks it against Pillow).  Raises ValueError where Pillow leaves the fixed-point path
    (check_fixed: a transformed corner at 32768 or beyond), and for any angle on an image wider or higher than 32768 pixels, whose
    indices 16.16 fixed point cannot hold."""
    W, H = int(W), int(H)
    if W <= 0 or H <= 0:
        raise ValueError("image size must be positive")
    if W > 32768 or H > 32768:
        raise ValueError(f"rotation of a {W} x {H} image: sides beyond 32768 do not fit 16.16 fixed point")
    angle = float(angle) % 360.0
    one, half = 1 << 16, 1 << 15
    if angle == 0:
        c = (one, 0, half, 0, one, half)
    elif angle == 180:
        c = (-one, 0, ((W - 1) << 16) | half, 0, -one, ((H - 1) << 16) | half)
    elif angle == 90 and W == H:                                            # Transpose.ROTATE_90: out(x, y) = in(W - 1 - y, x)
        c = (0, -one, ((W - 1) << 16) | half, one, 0, half)
    elif angle == 270 and W == H:                                           # Transpose.ROTATE_270: out(x, y) = in(y, H - 1 - x)
        c = (0, one, half, -one, 0, ((H - 1) << 16) | half)
    else:
        cx, cy = W / 2, H / 2
        a = -math.radians(angle)
        m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
        m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
        m[2] += cx
        m[5] += cy
        for x, y in ((0, 0), (W, H), (0, H), (W, 0)):                       # Geometry.c check_fixed on the four corners
            if not (abs(x * m[0] + y * m[1] + m[2]) < 32768.0 and abs(x * m[3] + y * m[4] + m[5]) < 32768.0):
                raise ValueError(f"rotation of a {W} x {H} image leaves Pillow's 16.16 fixed-point path (corner beyond 32768)")
        c = (_fix16(m[0]), _fix16(m[1]), _fix16(m[2] + m[0] * 0.5 + m[1] * 0.5), _fix16(m[3]), _fix16(m[4]), _fix16(m[5] + m[3] * 0.5 + m[4] * 0.5))
    return np.array(c, dtype=np.int32)


def _per_image(v, B: int, what: str) -> list:
    if isinstance(v, (int, float)):
        return [v] * B
    v = list(v)
    if len(v) != B:
        raise ValueError(f"{what}: {len(v)} entries for {B} images")
    return v


def _host_int_table(rows, B: int, width: int, what: str) -> np.ndarray:
    if isinstance(rows, torch.Tensor):
        if rows.is_cuda:
            raise ValueError(f"{what} must be host data (they are checked against the image size before the launch)")
        rows = rows.numpy()
    t = np.asarray(rows, dtype=np.int64).reshape(-1, width) if np.size(rows) else np.zeros((0, width), np.int64)
    if t.shape[0] == 1 and B > 1:
        t = np.repeat(t, B, axis=0)
    if t.shape[0] != B:
        raise ValueError(f"{what}: {t.shape[0]} rows for {B} images")
    return t


def _upload_table(t: np.ndarray, device) -> torch.Tensor:
    """int32 copy of a small per-image table on the device, staged in pinned memory so that the copy is queued on the stream
    instead of synchronising it (the caching host allocator keeps the staging block until the copy has run)."""
    return torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32)).pin_memory().to(device, non_blocking=True)


def rotate(images: torch.Tensor, angle: Union[float, Sequence[float]], *, out: str = "u8") -> torch.Tensor:
    """distortions:107-113 `F.rotate(img, angle)` (= `img.rotate(angle, NEAREST, expand=False, fillcolor=0)`) for a batch, bit-exact:
    one launch; `angle` is one angle or one per image."""
    images = _check_images(images)
    B, H, W, _ = images.shape
    cf = np.stack([rotation_coefficients(a, W, H) for a in _per_image(angle, B, "angle")])
    dev = images.device
    res = _alloc_out(B, H, W, out, dev)
    cf_dev = _upload_table(cf, dev)
    with torch.cuda.device(dev):
        N.check(N.lib().gsw_affine_nearest(images.data_ptr(), B, H, W, cf_dev.data_ptr(), res.data_ptr(), _MODES[out], _stream_ptr()))
    return res


def crop_resize(images: torch.Tensor, origins, crop_size: Tuple[int, int], size: Tuple[int, int], *, filter: str = "bilinear",
                out: str = "u8") -> torch.Tensor:
    """`img.crop((left, top, left + w, top + h)).resize(size, filter)` for a batch, bit-exact (Pillow's two passes, horizontal first):
    origins = (top, left) per image (host data, one row for all), crop_size = (h, w) shared by the batch, size = (width, height) as
    PIL takes it.  Two launches."""
    images = _check_images(images)
    B, H, W, _ = images.shape
    h, w = int(crop_size[0]), int(crop_size[1])
    Wo, Ho = int(size[0]), int(size[1])
    org = _host_int_table(origins, B, 2, "origins")
    if not (0 < h <= H and 0 < w <= W) or Wo <= 0 or Ho <= 0:
        raise ValueError(f"crop {h} x {w} -> {Ho} x {Wo} does not fit a {H} x {W} image")
    if (org < 0).any() or (org[:, 0] + h > H).any() or (org[:, 1] + w > W).any():
        raise ValueError(f"a {h} x {w} crop box lies outside the {H} x {W} image")
    dev = images.device
    res = _alloc_out(B, Ho, Wo, out, dev)
    tmp = torch.empty((B, h, Wo, 3), dtype=torch.uint8, device=dev)
    hb = hk = vb = vk = None
    hks = vks = 0
    if Wo != w:
        hb, hk, hks = _filter_plan(filter, w, Wo, dev)
    if Ho != h:
        vb, vk, vks = _filter_plan(filter, h, Ho, dev)
    org_dev = _upload_table(org, dev)
    with torch.cuda.device(dev):
        N.check(N.lib().gsw_crop_resize(images.data_ptr(), B, H, W, org_dev.data_ptr(), h, w, res.data_ptr(), Ho, Wo, _MODES[out], tmp.data_ptr(),
                                        hb.data_ptr() if hb is not None else None, hk.data_ptr() if hk is not None else None, hks,
                                        vb.data_ptr() if vb is not None else None, vk.data_ptr() if vk is not None else None, vks, _stream_ptr()))
    return res


def box_mask(images: torch.Tensor, boxes, *, keep_inside: bool, out: str = "u8") -> torch.Tensor:
    """One rectangle per image, boxes = (top, left, height, width) (host data, one row for all): keep_inside=True keeps it and blacks
    out the rest (distortions:207-222 "randomcrop": the crop pasted onto a black canvas at (left, top)); keep_inside=False blacks it
    out (distortions:126-137 "erasing" with value 0).  An empty box is allowed.  One launch."""
    images = _check_images(images)
    B, H, W, _ = images.shape
    bx = _host_int_table(boxes, B, 4, "boxes")
    if (bx < 0).any() or (bx[:, 0] + bx[:, 2] > H).any() or (bx[:, 1] + bx[:, 3] > W).any():
        raise ValueError(f"a box lies outside the {H} x {W} image")
    dev = images.device
    res = _alloc_out(B, H, W, out, dev)
    bx_dev = _upload_table(bx, dev)
    with torch.cuda.device(dev):
        N.check(N.lib().gsw_box_mask(images.data_ptr(), B, H, W, bx_dev.data_ptr(), 1 if keep_inside else 0, res.data_ptr(), _MODES[out], _stream_ptr()))
    return res


def resized_crop_params(H: int, W: int, scale: float, generator: Optional[torch.Generator] = None) -> Tuple[int, int, int, int]:
    """torchvision `RandomResizedCrop.get_params(img, scale=(scale, scale), ratio=(1, 1))` for an H x W image -> (top, left, h, w), drawing
    from `generator` (torch's global CPU generator when None) exactly as torchvision does: per try one uniform_ for the area and one
    for the log aspect ratio (both consumed although their ranges are single points), then randint for the origin; after 10
    failed tries the centred crop."""
    area = H * W
    for _ in range(10):
        target_area = area * torch.empty(1).uniform_(scale, scale, generator=generator).item()
        aspect_ratio = math.exp(torch.empty(1).uniform_(0.0, 0.0, generator=generator).item())          # log(ratio) = (0, 0)
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= W and 0 < h <= H:
            i = torch.randint(0, H - h + 1, size=(1,), generator=generator).item()
            j = torch.randint(0, W - w + 1, size=(1,), generator=generator).item()
            return i, j, h, w
    if W < H:                                                               # fallback: in_ratio against ratio (1, 1)
        w = h = W
    elif W > H:
        w = h = H
    else:
        w, h = W, H
    return (H - h) // 2, (W - w) // 2, h, w


def erasing_params(H: int, W: int, scale: float, generator: Optional[torch.Generator] = None) -> Optional[Tuple[int, int, int, int]]:
    """torchvision `RandomErasing.get_params(img, scale=(scale, scale), ratio=(1, 1), value=[0])` for an H x W image -> (top, left, h, w)
    of the erased box, or None where torchvision returns the image itself (10 tries without a box strictly inside the image)."""
    area = H * W
    for _ in range(10):
        erase_area = area * torch.empty(1).uniform_(scale, scale, generator=generator).item()
        aspect_ratio = math.exp(torch.empty(1).uniform_(0.0, 0.0, generator=generator).item())
        h = int(round(math.sqrt(erase_area * aspect_ratio)))
        w = int(round(math.sqrt(erase_area / aspect_ratio)))
        if not (h < H and w < W):
            continue
        i = torch.randint(0, H - h + 1, size=(1,), generator=generator).item()
        j = torch.randint(0, W - w + 1, size=(1,), generator=generator).item()
        return i, j, h, w
    return None


# the strength ranges of the reference's tool (distortions:17-34), for the distortion types this module runs on the device
distortion_strength_paras = dict(scaling=(0, 1), brightness=(1, 16), contrast=(1, 6), blurring=(0, 20), noise=(0, 0.5), compression=(100, 0),
                                 horizontal_flip=(0, 0), vertical_flip=(0, 0), togray=(0, 0), invert=(0, 0))


def relative_strength_to_absolute(strength: float, distortion_type: str) -> float:
    """distortions:37-49."""
    assert 0 <= strength <= 1
    lo, hi = distortion_strength_paras[distortion_type]
    s = strength * (hi - lo) + lo
    s = max(s, min(lo, hi))
    return min(s, max(lo, hi))


def apply_distortion(images: torch.Tensor, distortion_type: str, strength: Optional[float] = None, *, distortion_seed: int = 0,
                     relative_strength: bool = True, out: str = "u8") -> torch.Tensor:
    """Batch form of distortions:52-233 `apply_distortion` for the device-resident types; `strength` follows the reference
    (relative in [0, 1] unless relative_strength=False).  Unlike the reference the whole batch is one launch; for "noise" the image
    index keys the generator (the reference increments the seed per image)."""
    if distortion_type not in distortion_strength_paras:
        raise ValueError(f"distortion type {distortion_type!r} is not implemented on the device")
    if strength is not None and relative_strength:
        strength = relative_strength_to_absolute(strength, distortion_type)
    lo, hi = distortion_strength_paras[distortion_type]
    if strength is not None:
        assert min(lo, hi) <= strength <= max(lo, hi)
    if distortion_type == "compression":
        return jpeg_roundtrip(images, int(strength), out=out)
    if distortion_type == "blurring":
        blurred = gaussian_blur(images, int(strength))                  # distortions:158-164: kernel_size = int(strength)
        return blurred if out == "u8" else to_tensor(blurred, out=out)
    if distortion_type == "scaling":
        _, H, W, _ = images.shape
        return resize_lanczos(images, (int(W * strength), int(H * strength)), out=out)
    return pointwise(images, distortion_type, 0.0 if strength is None else strength, seed=distortion_seed, out=out)
