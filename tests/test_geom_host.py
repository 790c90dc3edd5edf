"""CPU (no GPU): the host halves of the geometric attacks (rotation, resizedcrop, erasing, randomcrop) against Pillow and torch, and the
`distortions` twin's table, naming, CLI parsing and refusals.  The device kernels consume exactly these coefficient rows, plans and boxes
(tests/test_gpu_geom.py checks them byte for byte against Pillow on the GPU)."""
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

import gswm_amd
from gswm_amd import _native as N, distortions as D, imaging

ANGLES = [0, 0.5, 1, 17.3, 45, 89.999, 90, 135, 179.9, 180, 180.0001, 270, 300.7, 359.99, 360, -30, 720.5, 1e-10, 90.00000000000001,
          179.99999999999997, 359.99999999999994, 5e-14]
SCALE_ONLY = [1e-14, 2e-14, 3e-16, 180.00000000000003]                          # round(sin, 15) == 0 away from the fast paths
SIZES = [(512, 512), (64, 96), (96, 64), (77, 51), (1, 7), (7, 1), (33, 33)]      # (W, H)
REL = [round(0.1 * k, 1) for k in range(11)]


def gather(img, c):
    """the gather of gsw_affine_nearest_kernel in NumPy: 32-bit wrapping sums, arithmetic shift, black outside"""
    H, W, _ = img.shape
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)

    def wrap(v):
        return ((v + 2 ** 31) % 2 ** 32) - 2 ** 31

    c = [int(v) for v in c]
    xin = wrap(c[2] + y * c[1] + x * c[0]) >> 16
    yin = wrap(c[5] + y * c[4] + x * c[3]) >> 16
    ok = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    out = np.zeros_like(img)
    out[ok] = img[yin[ok], xin[ok]]
    return out


def pil_rotate(img, angle):
    # torchvision F.rotate(img, angle) on a PIL image
    return np.asarray(Image.fromarray(img).rotate(angle, Image.Resampling.NEAREST, expand=False, center=None, fillcolor=(0, 0, 0)))


@pytest.mark.parametrize("W,H", SIZES)
def test_rotation_coefficients_equal_pillow(W, H):
    img = np.random.default_rng(W * 1000 + H).integers(0, 256, (H, W, 3), dtype=np.uint8)
    angles = ANGLES + SCALE_ONLY + [D.relative_strength_to_absolute(r, "rotation") for r in REL]
    for a in angles:
        c = imaging.rotation_coefficients(a, W, H)
        assert c.dtype == np.int32 and c.shape == (6,)
        assert np.array_equal(gather(img, c), pil_rotate(img, a)), (W, H, a)


def test_scale_only_angles_take_the_scale_affine_path():
    """The SCALE_ONLY angles are the ones Pillow serves with ImagingScaleAffine (a1 == a3 == 0 away from the fast paths); the gather
    above equals Pillow on them at every test size."""
    for a in SCALE_ONLY:
        r = -math.radians(a % 360.0)
        assert a % 360.0 not in (0.0, 90.0, 180.0, 270.0) and round(math.sin(r), 15) == 0.0, a
        c = imaging.rotation_coefficients(a, 64, 96)
        assert c[1] == 0 and c[3] == 0 and abs(int(c[0])) == 65536


def test_large_image_rotation_is_refused():
    """Geometry.c leaves the fixed-point path when a transformed corner reaches 32768: coefficients only, no image allocated."""
    for a in (17.3, 45, 300.7, 1e-14):
        with pytest.raises(ValueError):
            imaging.rotation_coefficients(a, 40000, 40000)
        with pytest.raises(ValueError):
            imaging.rotation_coefficients(a, 70000, 10)
    imaging.rotation_coefficients(45, 20000, 20000)                      # corners at ~24142: still fixed point
    for a in (0, 90, 180, 270):                                          # the transposes and the copy as 16.16 rows: sides up to 32768
        c = imaging.rotation_coefficients(a, 32768, 32768)
        assert int(c[2]) >= 0 and int(c[5]) >= 0
        with pytest.raises(ValueError):
            imaging.rotation_coefficients(a, 32769, 16)


def bilinear_plan_numpy(in_size, out_size):
    """Resample.c precompute_coeffs (bilinear, support 1) + normalize_coeffs_8bpc restated"""
    scale = filterscale = in_size / out_size
    filterscale = max(filterscale, 1.0)
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = []
        for x in range(xmax):
            t = abs((x + xmin - center + 0.5) * ss)
            w.append(1.0 - t if t < 1.0 else 0.0)
        ww = sum(w) if w else 0.0
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22))
        bounds[xx] = (xmin, xmax)
    return bounds, kk, ksize


PLAN_CASES = [(362, 512), (512, 362), (51, 77), (77, 51), (1, 7), (7, 1), (100, 100), (512, 52), (3, 1000), (1000, 3)]


@pytest.mark.parametrize("n_in,n_out", PLAN_CASES)
def test_resample_plan_bilinear_and_lanczos(n_in, n_out):
    b, k, ks = imaging.resample_plan_host("bilinear", n_in, n_out)
    rb, rk, rks = bilinear_plan_numpy(n_in, n_out)
    assert ks == rks and np.array_equal(b, rb) and np.array_equal(k, rk)
    lb, lk, lks = imaging.resample_plan_host("lanczos", n_in, n_out)
    ob, ok, oks = imaging.lanczos_plan_host(n_in, n_out)
    assert lks == oks and np.array_equal(lb, ob) and np.array_equal(lk, ok)
    assert N.lib().gsw_resample_plan(7, n_in, n_out, None, None, 0) == -N.GSW_ERR_BAD_ARG
    assert N.lib().gsw_resample_plan(N.GSW_RESAMPLE_BILINEAR, 0, n_out, None, None, 0) == -N.GSW_ERR_BAD_ARG


def two_pass(img, size):
    """ImagingResample with the libgswm plans: horizontal pass, uint8, vertical pass; a pass is skipped when its size is kept"""
    H, W, _ = img.shape
    Wo, Ho = size
    a = img.astype(np.int64)
    for axis, n_in, n_out in ((1, W, Wo), (0, H, Ho)):
        if n_in == n_out:
            continue
        bounds, kk, _ = imaging.resample_plan_host("bilinear", n_in, n_out)
        a = np.moveaxis(a, axis, 0)
        res = np.empty((n_out,) + a.shape[1:], np.int64)
        for o in range(n_out):
            xmin, xmax = bounds[o]
            ss = (1 << 21) + np.tensordot(kk[o, :xmax].astype(np.int64), a[xmin:xmin + xmax], axes=(0, 0))
            res[o] = np.clip(ss >> 22, 0, 255)
        a = np.moveaxis(res, 0, axis)
    return a.astype(np.uint8)


@pytest.mark.parametrize("HW,box,size", [
    ((512, 512), (75, 75, 437, 437), (512, 512)),       # resizedcrop 0.5-ish: upscaling
    ((512, 512), (0, 0, 512, 512), (256, 256)),         # downscaling
    ((96, 64), (5, 9, 52, 61), (96, 64)),               # non-square input: F.resized_crop's transposed output (width H, height W)
    ((64, 96), (3, 1, 51, 50), (64, 96)),
    ((77, 51), (10, 2, 40, 73), (40, 30)),              # non-square crop and output
    ((77, 51), (0, 0, 51, 77), (51, 33)),               # width kept: vertical pass only
    ((77, 51), (0, 0, 30, 77), (80, 77)),               # height kept: horizontal pass only
    ((7, 1), (0, 2, 1, 5), (7, 1)),
    ((1, 7), (0, 0, 7, 1), (1, 7)),
])
def test_two_pass_bilinear_equals_pillow_crop_resize(HW, box, size):
    H, W = HW
    img = np.random.default_rng(H * 7 + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    left, top, right, bottom = box
    ref = np.asarray(Image.fromarray(img).crop(box).resize(size, Image.Resampling.BILINEAR))
    assert np.array_equal(two_pass(img[top:bottom, left:right], size), ref)


# ------------------------------------------------------------------------------------------------------------------------------
# torchvision's get_params, restated the way torchvision writes them, on the global generator
# ------------------------------------------------------------------------------------------------------------------------------
def tv_resized_crop_params(height, width, scale, ratio=(1, 1)):
    area = height * width
    log_ratio = torch.log(torch.tensor(ratio))
    for _ in range(10):
        target_area = area * torch.empty(1).uniform_(scale[0], scale[1]).item()
        aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1])).item()
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= width and 0 < h <= height:
            i = torch.randint(0, height - h + 1, size=(1,)).item()
            j = torch.randint(0, width - w + 1, size=(1,)).item()
            return i, j, h, w
    in_ratio = float(width) / float(height)
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w = width
        h = height
    i = (height - h) // 2
    j = (width - w) // 2
    return i, j, h, w, "fallback"


def tv_erasing_params(img_h, img_w, scale, ratio=(1, 1), value=(0,)):
    area = img_h * img_w
    log_ratio = torch.log(torch.tensor(ratio))
    for _ in range(10):
        erase_area = area * torch.empty(1).uniform_(scale[0], scale[1]).item()
        aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1])).item()
        h = int(round(math.sqrt(erase_area * aspect_ratio)))
        w = int(round(math.sqrt(erase_area / aspect_ratio)))
        if not (h < img_h and w < img_w):
            continue
        v = torch.tensor(value)[:, None, None]        # noqa: F841 (value given: no draw)
        i = torch.randint(0, img_h - h + 1, size=(1,)).item()
        j = torch.randint(0, img_w - w + 1, size=(1,)).item()
        return i, j, h, w
    return None


PARAM_SIZES = [(512, 512), (64, 96), (96, 64), (51, 77), (7, 1), (1, 7)]       # (H, W)


def test_crop_and_erasing_params_equal_torchvision():
    fallbacks = {"resizedcrop": 0, "randomcrop": 0, "erasing": 0}
    for H, W in PARAM_SIZES:
        for r in REL:
            for t in ("resizedcrop", "randomcrop", "erasing"):
                s = D.relative_strength_to_absolute(r, t)
                for seed in range(21):
                    got = (imaging.erasing_params if t == "erasing" else imaging.resized_crop_params)(H, W, s, torch.Generator().manual_seed(seed))
                    torch.manual_seed(seed)
                    ref = (tv_erasing_params if t == "erasing" else tv_resized_crop_params)(H, W, (s, s))
                    if t == "erasing":
                        fallbacks[t] += ref is None
                        assert got == ref, (t, H, W, r, seed)
                    else:
                        fallbacks[t] += len(ref) == 5
                        assert got == tuple(ref[:4]), (t, H, W, r, seed)
                        i, j, h, w = got
                        assert 0 <= i and i + h <= H and 0 <= j and j + w <= W
    assert all(v > 0 for v in fallbacks.values()), fallbacks                 # every fallback branch is exercised
    # the private generator leaves the global one alone
    torch.manual_seed(3)
    a = torch.rand(1).item()
    torch.manual_seed(3)
    imaging.resized_crop_params(64, 64, 0.5, torch.Generator().manual_seed(0))
    assert torch.rand(1).item() == a


def test_strength_table_and_names():
    assert D.distortion_strength_paras == dict(
        rotation=(0, 360), scaling=(0, 1), resizedcrop=(1, 0.1), erasing=(0, 1), brightness=(1, 16), contrast=(1, 6), blurring=(0, 20),
        noise=(0, 0.5), compression=(100, 0), reversed=(0, 100), elastic=(0, 100), horizontal_flip=(0, 0), vertical_flip=(0, 0),
        togray=(0, 0), randomcrop=(1, 0), invert=(0, 0))
    assert list(D.distortion_strength_paras) == ["rotation", "scaling", "resizedcrop", "erasing", "brightness", "contrast", "blurring", "noise",
                                                 "compression", "reversed", "elastic", "horizontal_flip", "vertical_flip", "togray", "randomcrop",
                                                 "invert"]
    enabled = [k for k, v in D.Distortion_types_need2deal.items() if v["enable"]]
    assert enabled == ["rotation"] and D.Distortion_types_need2deal["rotation"]["relative_strength"] == 0.5
    assert len(D.Distortion_types_need2deal) == 15 and "reversed" not in D.Distortion_types_need2deal
    assert D.relative_strength_to_absolute(0.5, "rotation") == 180.0
    assert D.relative_strength_to_absolute(0.5, "resizedcrop") == 0.55
    assert D.relative_strength_to_absolute(0.3, "randomcrop") == 0.7
    assert D.relative_strength_to_absolute(1.0, "erasing") == 1.0
    for t in imaging.distortion_strength_paras:                                # the ten device types share the table
        assert imaging.distortion_strength_paras[t] == D.distortion_strength_paras[t]
    assert D.output_dir_name("rotation", 0.5) == "rotation_180.0"
    assert D.output_dir_name("resizedcrop", 0.3) == "resizedcrop_0.73"
    assert D.output_dir_name("rotation", 17.3, relative_strength=False) == "rotation_17.3"
    assert D.output_dir_name("compression", np.arange(0.1, 1, 0.1)[2]) == "compression_70.0"
    assert gswm_amd.distortions is D and "distortions" in gswm_amd.__all__


def test_cli_parsing():
    p = D.build_parser()
    a = p.parse_args(["--input_dir", "i", "--output_dir_base", "o", "--distortion_type", "rotation", "--strength", "0.5", "--relative_strength"])
    assert (a.input_dir, a.output_dir_base, a.distortion_type, a.strength, a.relative_strength) == ("i", "o", "rotation", 0.5, True)
    assert (a.sgstart, a.sgend, a.distortion_seed, a.same_operation, a.add2one) == (0.1, 1, 0, False, False)
    a = p.parse_args(["--input_dir", "i", "--output_dir_base", "o", "--add2one", "--distortion_seed", "7", "--same_operation", "--sgstart", "0.2",
                      "--sgend", "0.5"])
    assert (a.add2one, a.distortion_seed, a.same_operation, a.sgstart, a.sgend, a.distortion_type, a.strength) == (True, 7, True, 0.2, 0.5, None, None)
    with pytest.raises(SystemExit):
        p.parse_args(["--input_dir", "i", "--output_dir_base", "o", "--distortion_type", "swirl"])
    with pytest.raises(SystemExit):
        p.parse_args(["--output_dir_base", "o"])
    assert "NameError" in p.format_help()


def test_refusals_need_no_gpu():
    x = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    for t in ("elastic", "reversed"):
        with pytest.raises(ValueError, match=t):
            D.apply_distortion(x, t, 0.5)
    for t in D.GEOMETRIC:
        with pytest.raises(ValueError, match="strength"):
            D.apply_distortion(x, t, None)
    with pytest.raises(ValueError):
        D.apply_distortion(x, "swirl", 0.5)
    with pytest.raises(ValueError):                                             # host tensor
        D.apply_distortion(x, "rotation", 0.5)
    with pytest.raises(ValueError):
        imaging.box_mask(x, [(0, 0, 4, 4)], keep_inside=True)


def test_non_rgb_file_is_named(tmp_path):
    p = tmp_path / "rgba.png"
    Image.fromarray(np.zeros((4, 4, 4), np.uint8), "RGBA").save(p)
    with pytest.raises(ValueError, match="rgba.png"):
        D._decode(str(p))
    q = tmp_path / "ok.png"
    Image.fromarray(np.full((4, 5, 3), 9, np.uint8)).save(q)
    assert D._decode(str(q)).shape == (4, 5, 3)
    (tmp_path / "notes.txt").write_text("x")
    assert sorted(D.list_images(str(tmp_path))) == ["ok.png", "rgba.png"]
    assert os.path.basename(D.create_output_dir(str(tmp_path), {"rotation": 180.0, "erasing": 0.5})) == "rotation_180.0_erasing_0.5"
