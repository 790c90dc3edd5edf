"""Microbenchmark of the geometric attacks (csrc/gswm_image.hip: gsw_affine_nearest, gsw_crop_resize, gsw_box_mask) against two yardsticks
timed in the same process: the horizontal flip of gsw_image_pointwise (the same bytes moved) and gsw_resize_lanczos 380^2 -> 512^2 (the same
two-pass structure with more taps).  Launch time only: the per-image tables, crop origins and plans are on the device before the clock
starts, and every row calls the C ABI directly, so the Python wrappers' host work (parameter draws, table uploads) is not in the figures.
Each figure is the median of --reps timed loops of --iters back-to-back launches.

usage: python tools/geom_bench.py [--B 64] [--reps 7] [--iters 20] [--parent-lib PATH] [--pil]
  --parent-lib: a libgswm.so built from another commit; its gsw_resize_lanczos (512^2 -> 256^2, 380^2 -> 512^2) is timed interleaved with
                this tree's, run-to-run spread reported, so that a change of the shared resampler shows against the spread
  --pil:        also the 1-core PIL time per image of each attack (context only)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gswm_amd  # noqa: E402
from gswm_amd import _native as N, distortions as D, imaging  # noqa: E402
from gswm_amd.codec import _stream_ptr  # noqa: E402


def timeit(fn, iters, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) / iters * 1e3)                 # us per launch
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--pil", action="store_true")
    ap.add_argument("--json", default=None, help="also write the rows as JSON to this file")
    a = ap.parse_args()
    B, lib, st = a.B, N.lib(), _stream_ptr()
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (B, 512, 512, 3), dtype=torch.uint8, generator=g).cuda()
    img380 = torch.randint(0, 256, (B, 380, 380, 3), dtype=torch.uint8, generator=g).cuda()
    outs = {m: imaging._alloc_out(B, 512, 512, m, img.device) for m in ("u8", "f16")}
    modes = {"u8": N.GSW_IMG_U8_HWC, "f16": N.GSW_IMG_F16_CHW}

    def table(rows):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(rows, dtype=np.int32))).cuda()

    rot = {a_: table([imaging.rotation_coefficients(a_, 512, 512)] * B) for a_ in (180.0, 17.3, 45.0)}
    s_rc = D.relative_strength_to_absolute(0.5, "resizedcrop")
    rc = [imaging.resized_crop_params(512, 512, s_rc, torch.Generator().manual_seed(b)) for b in range(B)]
    ch, cw = rc[0][2], rc[0][3]
    rc_org = table([(i, j) for i, j, _, _ in rc])
    rc_tmp = torch.empty((B, ch, 512, 3), dtype=torch.uint8, device="cuda")
    hb, hk, hks = imaging._filter_plan("bilinear", cw, 512, img.device)
    vb, vk, vks = imaging._filter_plan("bilinear", ch, 512, img.device)
    er = table([imaging.erasing_params(512, 512, D.relative_strength_to_absolute(0.5, "erasing"), torch.Generator().manual_seed(b)) or (0, 0, 0, 0)
                for b in range(B)])
    s_cr = D.relative_strength_to_absolute(0.3, "randomcrop")
    cr = table([imaging.resized_crop_params(512, 512, s_cr, torch.Generator().manual_seed(b)) for b in range(B)])
    lz_tmp = torch.empty((B, 512, 512, 3), dtype=torch.uint8, device="cuda")
    lz = {(380, 512): (imaging._plan(380, 512, img.device), img380), (512, 256): (imaging._plan(512, 256, img.device), img)}
    modes_of = {torch.uint8: N.GSW_IMG_U8_HWC, torch.float16: N.GSW_IMG_F16_CHW}

    def lanczos(L, key, res):
        (b_, k_, ks), src = lz[key]
        n_in, n_out = key
        return lambda: L.gsw_resize_lanczos(src.data_ptr(), B, n_in, n_in, res.data_ptr(), n_out, n_out, modes_of[res.dtype], lz_tmp.data_ptr(),
                                            b_.data_ptr(), k_.data_ptr(), ks, b_.data_ptr(), k_.data_ptr(), ks, st)

    rows = []
    from bench_board import BoardSampler
    with BoardSampler(0) as board:
        for m in ("u8", "f16"):
            o, md = outs[m], modes[m]
            cases = [
                ("flip (yardstick)", lambda: lib.gsw_image_pointwise(img.data_ptr(), B, 512, 512, N.GSW_PW_HFLIP, 0.0, 0, 0, o.data_ptr(), md, None, st)),
                ("lanczos 380^2->512^2 (yardstick)", lanczos(lib, (380, 512), o)),
                ("rotate 180", lambda: lib.gsw_affine_nearest(img.data_ptr(), B, 512, 512, rot[180.0].data_ptr(), o.data_ptr(), md, st)),
                ("rotate 17.3", lambda: lib.gsw_affine_nearest(img.data_ptr(), B, 512, 512, rot[17.3].data_ptr(), o.data_ptr(), md, st)),
                ("rotate 45", lambda: lib.gsw_affine_nearest(img.data_ptr(), B, 512, 512, rot[45.0].data_ptr(), o.data_ptr(), md, st)),
                (f"resizedcrop 0.5 ({ch}^2->512^2)", lambda: lib.gsw_crop_resize(img.data_ptr(), B, 512, 512, rc_org.data_ptr(), ch, cw, o.data_ptr(), 512, 512, md,
                                                                              rc_tmp.data_ptr(), hb.data_ptr(), hk.data_ptr(), hks, vb.data_ptr(), vk.data_ptr(), vks, st)),
                ("erasing 0.5", lambda: lib.gsw_box_mask(img.data_ptr(), B, 512, 512, er.data_ptr(), 0, o.data_ptr(), md, st)),
                ("randomcrop 0.3", lambda: lib.gsw_box_mask(img.data_ptr(), B, 512, 512, cr.data_ptr(), 1, o.data_ptr(), md, st)),
            ]
            for name, fn in cases:
                assert fn() == N.GSW_OK, name
                t = timeit(fn, a.iters, a.reps)
                rows.append({"case": name, "out": m, "us_median": statistics.median(t), "us_min": min(t), "us_max": max(t)})
    med = {(r["case"], r["out"]): r["us_median"] for r in rows}
    bars = [("rotate 180", "flip (yardstick)", 1.25), ("erasing 0.5", "flip (yardstick)", 1.25), ("randomcrop 0.3", "flip (yardstick)", 1.25),
            ("rotate 17.3", "flip (yardstick)", 2.0), ("rotate 45", "flip (yardstick)", 2.0),
            (f"resizedcrop 0.5 ({ch}^2->512^2)", "lanczos 380^2->512^2 (yardstick)", 1.1)]
    print(f"B = {B}, 512^2 RGB, median of {a.reps} x {a.iters} launches; board: {json.dumps(board.summary())}")
    print(f"{'case':40s} {'out':4s} {'median us':>10s} {'min':>9s} {'max':>9s} {'GB/s (u8 in+out)':>17s}")
    for r in rows:
        print(f"{r['case']:40s} {r['out']:4s} {r['us_median']:10.1f} {r['us_min']:9.1f} {r['us_max']:9.1f} {B * 512 * 512 * 6 / r['us_median'] / 1e3:17.0f}")
    print("bars (new / yardstick, same output kind):")
    ok_all = True
    for m in ("u8", "f16"):
        for case, ref, lim in bars:
            q = med[(case, m)] / med[(ref, m)]
            ok_all &= q <= lim
            print(f"  {case:36s} {m:4s} {q:6.3f}  (bar {lim:.2f} x {ref}) {'ok' if q <= lim else 'MISSED'}")
    print("all bars hold" if ok_all else "a bar is missed")

    if a.parent_lib:
        P = C.CDLL(a.parent_lib)
        res, args = N._PROTOTYPES["gsw_resize_lanczos"]
        P.gsw_resize_lanczos.restype, P.gsw_resize_lanczos.argtypes = res, args
        print(f"gsw_resize_lanczos, this tree vs {a.parent_lib}, B = {B}, u8, interleaved: median us per launch over {a.reps} loops, 5 rounds")
        for key in ((512, 256), (380, 512)):
            o = imaging._alloc_out(B, key[1], key[1], "u8", img.device)
            per = {"branch": [], "parent": []}
            for _ in range(5):
                for who, L in (("parent", P), ("branch", lib)):
                    per[who].append(statistics.median(timeit(lanczos(L, key, o), a.iters, a.reps)))
            for who in ("parent", "branch"):
                v = per[who]
                print(f"  {key[0]}^2->{key[1]}^2 {who:7s} median of rounds {statistics.median(v):8.1f} us  rounds {' '.join(f'{x:.1f}' for x in v)}  "
                      f"spread {max(v) - min(v):.1f} us")

    if a.pil:
        from PIL import Image
        torch.set_num_threads(1)
        x = Image.fromarray(img[0].cpu().numpy())
        arr = img[0].cpu().numpy()
        i, j, h, w = rc[0]
        pil_cases = [("rotate 180", lambda: x.rotate(180.0)), ("rotate 17.3", lambda: x.rotate(17.3)), ("rotate 45", lambda: x.rotate(45.0)),
                     ("resizedcrop 0.5", lambda: x.crop((j, i, j + w, i + h)).resize((512, 512), Image.Resampling.BILINEAR)),
                     ("erasing 0.5 (numpy)", lambda: arr.copy().__setitem__((slice(10, 372), slice(10, 372)), 0)),
                     ("randomcrop 0.3", lambda: Image.new("RGB", x.size).paste(x.crop((20, 20, 448, 448)), (20, 20))),
                     ("flip", lambda: x.transpose(Image.Transpose.FLIP_LEFT_RIGHT)),
                     ("lanczos 380^2->512^2", lambda: x380.resize((512, 512), Image.Resampling.LANCZOS))]
        x380 = Image.fromarray(img380[0].cpu().numpy())
        print("PIL, one core, per 512^2 image (context):")
        for name, fn in pil_cases:
            fn()
            t0 = time.perf_counter()
            for _ in range(20):
                fn()
            print(f"  {name:28s} {(time.perf_counter() - t0) / 20 * 1e3:8.2f} ms")
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"B": B, "rows": rows, "board": board.summary()}, f, indent=1)


if __name__ == "__main__":
    main()
