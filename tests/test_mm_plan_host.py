"""CPU (no GPU): the launch policy of the matmul engine is one pure function (csrc/gswm_mm_plan.h: mm_decide), and tests/golden/mm_plan_cases.tsv is its table --
one launch per row, the inputs of mm_decide and the decision the engine took for them (recorded from the engine as it was before the policy became one
function; a later change of policy shows as a diff of the table).  tests/mm_plan_cases.cpp, a host-only program, prints mm_decide's answer per row; integers and
the hex-float predicted microseconds must be equal.  The table must also cover the policy: a branch without a row would be a branch nobody can see change."""
import collections
import csv
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

TABLE = os.path.join(ROOT, "tests", "golden", "mm_plan_cases.tsv")
DECISION = ("status d_tile_rows d_tile_cols mt wide splits panel tiles_n ntiles grid epi wave12 lnf rowstats_slots colstats_rows_per_block colstats_blocks "
            "ws_need t_us").split()


@pytest.fixture(scope="module")
def table():
    with open(TABLE, newline="") as f:
        rows = list(csv.DictReader(f, delimiter="\t"))
    assert 500 <= len(rows) <= 5000
    return rows


def test_mm_decide_reproduces_the_recorded_decisions(table, tmp_path):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    if hipcc is None:
        pytest.skip("no hipcc")
    exe = tmp_path / "mm_plan_cases"
    # the library's compiler on host code only, the library's optimisation level, no fast-math: the cost model compares doubles
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O3", "-Wall", "-Werror", "-I", os.path.join(ROOT, "a-watermark-for-diffusion-models_amd", "csrc"),
                    os.path.join(ROOT, "tests", "mm_plan_cases.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe), TABLE], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(table)
    bad = []
    for line, want in zip(out, table):
        got = line.split("\t")
        assert got[0] == want["tag"] and len(got) == 1 + len(DECISION)
        diff = [(c, g, want[c]) for c, g in zip(DECISION, got[1:]) if g != want[c]]      # strings: integers exactly, hex floats exactly
        if diff:
            bad.append((want["tag"], diff))
    assert not bad, (len(bad), bad[:10])


def test_the_table_covers_the_policy(table):
    by_tag = {r["tag"]: r for r in table}
    assert len(by_tag) == len(table)
    ok = [r for r in table if r["status"] == "0"]
    n = collections.Counter()

    def has(name, pred, rows=ok):
        n[name] = sum(1 for r in rows if pred(r))

    def tag(name, **want):
        """the row with this tag exists and its recorded decision is what the tag says"""
        r = by_tag.get("cover/" + name)
        n[name] = int(r is not None and all(r[k] == str(v) for k, v in want.items()))

    has("tile rows 128", lambda r: r["d_tile_rows"] == "128")
    has("tile rows 256", lambda r: r["d_tile_rows"] == "256" and r["wide"] == "0")
    has("wide", lambda r: r["wide"] == "1" and r["d_tile_cols"] == "320" and r["mt"] == "8")
    for t in ("taken_dense", "taken_geglu", "taken_pf", "m256_does_not_bind_pf", "m_at_2048", "two_segments_pf_taken", "forced_512",
              "bound_resid_below", "bound_y_below", "bound_a_below", "bound_w_below", "pmin_dense_at", "pmin_res_at", "pmin_pf_at"):
        tag("wide/" + t, status=0, wide=1)
    for t in ("refused_mode_trans", "refused_mode_qkv", "refused_n320", "refused_m256_dense", "refused_m256_geglu", "bound_resid_at", "bound_y_at", "bound_a_at",
              "bound_w_at", "pmin_dense_below", "pmin_res_below", "pmin_pf_below", "refused_fewer_tiles_than_cus", "refused_rounds", "refused_m_below_2048",
              "refused_two_segments", "forced_512_illegal", "forced_256", "forced_128"):
        tag("wide/" + t, status=0, wide=0)
    tag("wide/two_segments_forced_512", status=2)
    auto = [r for r in ok if r["max_splits"] == "0" and r["tile_rows"] == "0"]
    has("automatic splits of 2", lambda r: r["splits"] == "2", auto)
    has("automatic splits of 32", lambda r: r["splits"] == "32", auto)
    n["automatic splits between"] = len({r["splits"] for r in auto if 2 < int(r["splits"]) < 32})
    assert n["automatic splits between"] >= 3
    has("forced splits", lambda r: int(r["max_splits"]) > 1 and int(r["splits"]) > 1 and r["epi"] == "4")
    has("forced splits, 256-row tile", lambda r: int(r["max_splits"]) > 1 and int(r["splits"]) > 1 and r["d_tile_rows"] == "256")
    has("split plan too big for its workspace", lambda r: r["splits"] == "1" and 0 < int(r["ws_bytes"]) < int(r["ws_need"]) and r["ws_ptr"] == "1")
    tag("split/workspace_one_byte_short", splits=1)
    tag("split/workspace_exact", splits=30, epi=4, wave12=1)
    tag("split/no_workspace_null", splits=1, ws_need=0)
    tag("split/no_workspace_zero_bytes", splits=1, ws_need=0)
    tag("split/max_splits_1", splits=1, ws_need=0)
    tag("split/ln_stat_never_splits", splits=1, ws_need=0, lnf=1)
    tag("panel/8", panel=8, wide=0)
    tag("panel/all_narrow_tiles", panel=10, tiles_n=10, wide=0)
    tag("panel/narrow_over_budget", panel=8, tiles_n=10, wide=0)
    tag("panel/4", panel=4, wide=1)
    tag("panel/all_wide_tiles", panel=8, tiles_n=8, wide=1)
    for e in (0, 1, 2, 3, 5, 4):
        has(f"epilogue {e}", lambda r: r["epi"] == str(e))
    for e in (0, 1, 2, 3):
        has(f"epilogue {e} 12-wave by the mask", lambda r: r["epi"] == str(e) and r["wave12"] == "1" and (int(r["split_mask"]) >> e) & 1)
        has(f"epilogue {e} 8-wave by the mask", lambda r: r["epi"] == str(e) and r["wave12"] == "0" and r["wide"] == "0" and r["lnf"] == "0" and not (int(r["split_mask"]) >> e) & 1)
    has("dense rows, 256-row tile, mask bit set: 8-wave", lambda r: r["epi"] == "0" and r["mt"] == "4" and r["wave12"] == "0" and r["lnf"] == "0" and int(r["split_mask"]) & 1)
    has("epilogue 5 is 8-wave whatever the mask", lambda r: r["epi"] == "5" and r["wave12"] == "0" and int(r["split_mask"]) == 15)
    for mt in (2, 4, 8):
        has(f"LayerNorm-folded at mt {mt}", lambda r: r["lnf"] == "1" and r["mt"] == str(mt) and r["wave12"] == "0")
    tag("rowstats/narrow_granted", rowstats_slots=8)
    tag("rowstats/narrow_one_short", rowstats_slots=0)
    tag("rowstats/wide_granted", rowstats_slots=16, wide=1)
    tag("rowstats/wide_one_short", rowstats_slots=0, wide=1)
    tag("colstats/narrow128_granted", colstats_rows_per_block=32, colstats_blocks=128)
    tag("colstats/narrow128_one_short", colstats_rows_per_block=0, colstats_blocks=0)
    tag("colstats/narrow256_granted", colstats_rows_per_block=64, colstats_blocks=1024)
    tag("colstats/narrow256_one_short", colstats_rows_per_block=0)
    tag("colstats/wide_granted", colstats_rows_per_block=128, colstats_blocks=512, wide=1)
    tag("colstats/wide_one_short", colstats_rows_per_block=0, wide=1)
    # every early error return of gsw_mm_launch, and the pairs that fix which code wins
    errors = {"dtype": 1, "dtype_f64": 1, "colstats_capacity_negative": 1, "rowstats_capacity_negative": 1, "workspace_bytes_negative": 1, "max_splits_negative": 1,
              "max_splits_above_64": 1, "colstats_misaligned": 1, "rowstats_misaligned": 1, "workspace_misaligned": 1, "unknown_flag_bits": 1, "n_mod_8": 2,
              "geglu_n_mod_160": 2, "m_zero": 2, "p_zero": 2, "qkv_n_rows_zero": 2, "qkv_n_rows_mod_160": 2, "qkv_n_rows_all": 2, "qkv_no_y2": 2,
              "bias_misaligned_dense": 1, "bias_misaligned_geglu": 1, "ln_stat_mode": 2, "ln_stat_rowbias": 2, "wide_forced_two_segments": 2, "too_many_tiles": 2,
              "order/dtype_before_n_mod_8": 1, "order/extras_before_n_mod_8": 1, "order/n_mod_8_before_bias": 2, "order/bias_before_ln_stat_rowbias": 1,
              "order/bias_ok_for_pf_rows": 0}
    for name, status in errors.items():
        r = by_tag.get("err/" + name)
        n["err/" + name] = int(r is not None and r["status"] == str(status))
    # the real launches: an SD 2.1 forward at 1, 2, 8, 16, 64 and 128 images over its four levels, the VAE decoder at 1 and 8 images
    for B in (1, 2, 8, 16, 64, 128):
        for level in ("64x64x320", "32x32x640", "16x16x1280", "8x8x1280"):
            pre = f"sd21/b{B}/{level}/"
            for kind in ("proj_in", "geglu_ln", "v_trans", "proj_out_scatter", "qkv", "ffout_proj_out_2seg", "conv3x3/pad", "conv3x3/int",
                         "conv1x1/pad", "conv1x1/int", "shortcut_2seg/pad", "shortcut_2seg/int", "shortcut_3seg/pad", "shortcut_3seg/int"):
                n[pre + kind] = int(pre + kind in by_tag)
            if not level.startswith("8x8"):
                n[pre + "down_stride2"] = int(pre + "down_stride2/int" in by_tag and pre + "down_stride2/pad" in by_tag)
            if not level.startswith("64x64"):
                n[pre + "up2x"] = int(pre + "up2x/int" in by_tag and pre + "up2x/pad" in by_tag)
    for B in (1, 8):
        for N in (128, 256, 512):
            has(f"vae b{B} {N} channels", lambda r: r["tag"].startswith(f"vae/b{B}/") and r["N"] == str(N))
    missing = sorted(k for k, v in n.items() if v == 0)
    print({k: v for k, v in n.items() if not k.startswith(("sd21/", "err/"))})
    assert not missing, missing
