// gswm_mm_plan.h -- the launch policy of the matmul engine (csrc/gswm_mm.hip) as ONE pure function: mm_decide maps (launch arguments, extras, knobs) to the
// complete decision of a launch -- status, tile, split-K, panel, grid, kernel form, records granted.  Host code only, plain C++17, no HIP: it compiles with the host
// compiler alone, so the policy can be tabulated without a GPU (tests/test_mm_plan_host.py against tests/golden/mm_plan_cases.tsv).
#pragma once
#include <stdint.h>
#include <algorithm>

#include "../../include/gswm.h"
#include "gswm_mm.h"

// Everything outside the arguments that the policy reads.  gswm_mm.hip fills it (mm_knobs): the environment once per process, the two atomics per call.
//   tile_rows     GSW_MM_BM / gsw_mm_config: 0 auto; 128 / 256 force a narrow tiling, 512 the wide tile wherever it is legal
//   split_mask    GSW_MM_SPLIT / gsw_mm_config: bit e set = epilogue kind e runs the 12-wave form whose waves 8-11 own the LDS-DMA (default 10: EPI 1 and EPI 3)
//   cus           compute units the grid, the plan's "rounds" and its half-chip threshold are counted in (mm_cus(): 256, GSW_MM_CUS)
//   panel         GSW_MM_PANEL: > 0 fixes the panel of the narrow tile order (A/B switch: 8 = the fixed panel of ABI < 0.4.0); default 0
//   wide_mask     GSW_MM_WIDE: bit e: epilogue kind e (0 dense rows, 1 PF rows, 2 GEGLU) may take the wide tile; 0 = never (A/B); default 7
//   wide_pmin     GSW_MM_WIDE_PMIN: stages from which the dense-row / GEGLU launches take the wide tile; default 5
//   wide_pmin_pf  GSW_MM_WIDE_PMIN_PF: ... the PF-row launches; default 64
//   wide_pmin_res GSW_MM_WIDE_PMIN_RES: ... dense rows with a residual operand; default 8
struct MMKnobs {
    int tile_rows, split_mask;
    int cus;
    int panel, wide_mask, wide_pmin, wide_pmin_pf, wide_pmin_res;
};

// The complete decision for one launch.  status != GSW_OK: the launch returns it and every other field is zero.
struct MMLaunch {
    int status;
    int tile_rows, tile_cols, mt;      // 128 / 256 x 160, or 256 x 320 (wide); mt = 2 / 4 / 8 (wide): the kernel's MT
    bool wide, wave12, lnf;            // the 256 x 320 tile; the 12-wave form; LayerNorm folded into the epilogue
    int splits, panel;                 // splits > 1: split-K; panel: column tiles per panel of the tile order
    int32_t tiles_n, ntiles;
    uint32_t grid;
    int epi;                           // 0 dense rows, 1 PF rows, 2 GEGLU, 3 transposed, 5 QKV; 4 = split-K (the reduce kernel runs the epilogue)
    int rowstats_slots, colstats_rows_per_block, colstats_blocks;      // records granted (0: refused / not requested)
    int64_t ws_need;                   // bytes of workspace the split plan needs (0: the plan does not split); splits == 1 with ws_need > 0: it did not fit
    double t_us;                       // what the cost model predicts for the tiling taken (narrow-tile model)
};

// Tiling and split-K plan of a launch, with the time the cost model predicts for it (microseconds).  The model is fitted to tools/splitk_tile_sweep.py
// (profiles/r04i_splitk_tile_sweep.txt: 35 shapes x tile rows x split counts, HBM-cold weights, graph-captured; rms error 6 %, mean regret of its choices 1 %):
//   a stage of a 128-row tile costs 0.56 us while at most half the CUs work and 0.67 with all of them; a stage of a 256-row tile 0.79-0.81 and 1.13 (the chip is
//   power- and L2-bound when every CU multiplies: section 4.8 of DESIGN.md); an unsplit launch pays 2.5 us on top, a split one 12.5 (its reduce kernel) and 0.014 per
//   80 KiB of slab.
// Unsplit tile: for long K (>= 40 stages) and at most one round of 256-row tiles the model decides -- 128-row tiles when 256-row ones would leave half the chip idle
// (4096 x 1280 outputs: 127 vs 162 us at K = 11520; 52 vs 69 at K = 5120; the round-3 rule kept 256 rows there from a sweep whose weights were L2-hot).  Short K keeps
// the measured rule of round 3 (128-row tiles whenever 256-row ones do not fill the chip: a short-K weight matrix stays in L2 and all CUs win), more than one round
// keeps 256-row tiles (a half tile re-fetches the weight tile twice as often).
// Split: at most 128 tiles, at least 8 stages, up to 32 ways (one image at 8 x 8: 8 tiles x 32 = the whole chip, 19.9 vs 21.1 us at 16 ways) and 256 workgroups, 128- or 256-row tiles, taken for a predicted gain of 5 % or more.  Forced splits
// (max_splits > 1: tests) use 128 rows unless gsw_mm_config forces the 256-row tile.
// bm0 / t0_us: the tile and the time of the UNSPLIT launch (also taken when a split plan does not fit the workspace).
struct MMPlan { int bm; int splits; double t_us; int bm0; double t0_us; };
// (the stage costs were fitted on ONE box of the pool in round 4 -- profiles/r04i_splitk_tile_sweep.txt: MI355X, 256 CUs, 1400 W board limit, HBM-cold weights,
// the deep levels at 4-64 images, board at 1.1-1.3 kW; boxes of the pool differ by +-4 %.  W = busy workgroups; the costs are functions of the busy FRACTION
// of the chip, so a different CU count rescales W, not the constants.)
inline double mm_stage_us(int bm, double W, int64_t CU) {
    const double half = 0.5 * (double)CU;
    const double over = W > half ? (W - half) / half : 0.0;
    return bm == 128 ? 0.56 + 0.11 * over : 0.79 + 0.02 * std::min(1.0, W / half) + 0.32 * over;
}
inline MMPlan mm_plan(int64_t M, int64_t tiles_n, int32_t P, bool can_split, int max_splits, const MMKnobs& k) {
    const int bm_env = k.tile_rows;          // GSW_MM_BM / gsw_mm_config: 128 / 256 forces a tiling (A/B runs, tests)
    const int64_t CU = k.cus;
    const int64_t nt256 = ((M + 255) / 256) * tiles_n, nt128 = ((M + 127) / 128) * tiles_n;
    auto t_unsplit = [&](int bm) {
        const int64_t nt = bm == 256 ? nt256 : nt128, rounds = (nt + CU - 1) / CU;
        return 2.5 + mm_stage_us(bm, rounds == 1 ? (double)nt : (double)CU, CU) * (double)P * (double)rounds;
    };
    int BM;
    if (bm_env == 128 || bm_env == 256) BM = bm_env;
    else if (M <= 128) BM = 256;
    else if (P >= 40 && nt256 <= CU) BM = t_unsplit(128) < t_unsplit(256) ? 128 : 256;
    else BM = nt256 < (P >= 64 ? CU / 2 : CU) ? 128 : 256;
    MMPlan pl{BM, 1, t_unsplit(BM), BM, 0.0};
    pl.t0_us = pl.t_us;
    if (!can_split) return pl;
    if (max_splits > 1) {
        const int bm_s = bm_env == 256 && M > 128 ? 256 : 128;
        const int64_t nt_f = ((M + bm_s - 1) / bm_s) * tiles_n;
        const int sp = (int)std::min<int64_t>(std::min<int64_t>(max_splits, P), CU / std::max<int64_t>(nt_f, 1));
        if (sp >= 2) { pl.bm = bm_s; pl.splits = sp; }
        return pl;
    }
    if (P < 8) return pl;
    double best = pl.t_us / 1.05;
    for (int bm_c = 128; bm_c <= 256; bm_c += 128) {
        if (bm_c == 256 && (M <= 128 || bm_env == 128)) continue;
        if (bm_c == 128 && bm_env == 256) continue;
        const int64_t nt_c = bm_c == 256 ? nt256 : nt128;
        if (nt_c > CU / 2) continue;
        for (int s_ = 2; s_ <= 32 && s_ * nt_c <= CU && 2 * s_ <= P; ++s_) {
            const double t = 12.5 + mm_stage_us(bm_c, (double)(s_ * nt_c), CU) * (double)((P + s_ - 1) / s_) + 0.014 * (double)(s_ * nt_c * (bm_c / 128));
            if (t < best) { best = t; pl.bm = bm_c; pl.splits = s_; pl.t_us = t; }
        }
    }
    return pl;
}

// May the launch take the wide tile (256 x 320, MT = 8)?  Launches with enough of those tiles to keep every CU busy for several rounds and a K loop long enough to
// amortise the longer fill (two 72 KiB stages).  Fewer operand bytes per MFMA is what pays under the board's power limit.
// GSW_MM_WIDE=0 / gsw_mm_config(tile_rows = 256 or 128) keep the narrower tiles (A/B, tests); tile_rows = 512 forces the wide tile wherever it is legal.
// Returns 1 (wide), 0 (narrow) or -1: the caller FORCES the wide tile on a launch whose A operand lies in several K segments (GSW_ERR_UNSUPPORTED).
inline int mm_wide(const MMArgs& a, int epi, int64_t tiles_n, const MMKnobs& k) {
    const int epi_k = epi == 2 ? 2 : epi == 0 ? 0 : 1;
    const int wide_env = (k.wide_mask >> epi_k) & 1;
    const bool mode_ok = a.mode == MM_MODE_DENSE || a.mode == MM_MODE_PF || a.mode == MM_MODE_TOK2PF || a.mode == MM_MODE_UP2X || a.mode == MM_MODE_GEGLU;
    const int64_t tn_w = (a.N + 319) / 320, tm_w = ((int64_t)a.M + 255) / 256;
    // buffer addressing of the wide producer: no weight-row clamp (N % 320 == 0), every activation segment below 4 GiB
    int64_t rows_in = a.M;
    if (a.mode == MM_MODE_PF || a.mode == MM_MODE_UP2X) {
        const int64_t per_img = (a.flags & MM_FLAG_COMPACT) ? (int64_t)std::max(1, (a.Hp - 2) * (a.Wp - 2)) : (int64_t)a.Hp * a.Wp;
        rows_in = ((int64_t)a.M / per_img + 1) * (int64_t)a.in_Hp * a.in_Wp + 2 * (int64_t)a.in_Wp + 4;
    }
    int64_t ld_max = 0;
    for (int i = 0; i < a.nseg; ++i) ld_max = std::max<int64_t>(ld_max, a.seg[i].ld);
    // rows of the output / residual row space (the residual touches address it through a buffer descriptor too)
    int64_t rows_out = a.M;
    if (a.mode == MM_MODE_PF || a.mode == MM_MODE_TOK2PF) rows_out = ((int64_t)a.M / std::max<int64_t>(1, (a.mode == MM_MODE_TOK2PF ? a.S : ((a.flags & MM_FLAG_COMPACT) ? (int64_t)(a.Hp - 2) * (a.Wp - 2) : (int64_t)a.Hp * a.Wp))) + 1) * (int64_t)a.Hp * a.Wp;
    if (a.mode == MM_MODE_UP2X) rows_out = rows_in * 4 + 8;
    const int64_t lim = ((int64_t)1 << 32) - (1 << 20);
    const bool res_ok = !a.resid || rows_out * (int64_t)a.ldr * 2 < lim;
    // (the dense-row epilogue of the wide tile addresses its OUTPUT by a 32-bit byte offset too)
    const bool y_ok = epi != 0 || (int64_t)a.M * a.ldy * 2 < lim;
    const bool legal = mode_ok && res_ok && y_ok && a.N >= 320 && a.N % 320 == 0 && (!(epi == 2 || epi == 0) || a.M % 256 == 0) && rows_in * ld_max * 2 < lim && (int64_t)a.N * a.ldw * 2 < lim;
    // a partial last column tile costs a whole one: at most 1/8 of the column tiles' work wasted
    // measured per shape at 128 rows (profiles/r05g_unet_forward_b128_wide_thresholds.txt): the dense-row and GEGLU launches win at every K of the eps model,
    // K = 320 included (-5 ... -24 %: a 320-column tile reads the activations once where two 160-column tiles read them twice) -- except the K = 320 launches
    // WITH a residual operand (+6 %: five stages do not pay for the longer epilogue), which stay narrow; the PF-row epilogue (convolutions, token scatter:
    // per-row residual / row-bias fetches, twice as long per wave on the wide tile) needs a longer K loop -- 3 x 3 convolutions win from K = 5760 on
    // (-3 ... -7 %) and lose 2-6 % at K = 2880
    const int p_min = epi_k == 1 ? k.wide_pmin_pf : (a.resid ? std::max(k.wide_pmin, k.wide_pmin_res) : k.wide_pmin);
    // rounds of 256 workgroups: a stage of a wide tile costs 1.77 x a stage of a 256 x 160 tile for 2 x its outputs (1.70 vs 0.96 us, the slopes of time against K on
    // the 64 x 64 convolutions) -- wide wins when its rounds, at that price, are fewer than the narrow tiling's (a half-empty last round can eat the gain:
    // 4.5 rounds of wide tiles against 9 of narrow ones still win, 2.25 against 4.5 do not)
    const int64_t cus = k.cus, t_w = tm_w * tn_w, t_n = (((int64_t)a.M + 255) / 256) * tiles_n;
    const double cost_w = 1.77 * (double)((t_w + cus - 1) / cus), cost_n = (double)((t_n + cus - 1) / cus);
    const bool fits = t_w >= cus && cost_w <= 0.995 * cost_n && a.P >= p_min && a.M >= 2048;
    // the wide dense-row / GEGLU producer (AFF in the kernel) steps from one 64-row piece to the next by seg[0]'s row stride, pinned in a scalar register for
    // the whole launch: an A operand in several K segments stays on the narrow tiles there, and a caller that FORCES the wide tile is told so
    // (a launch the plan split along K never gets here: the split kernels are narrow and segment-aware)
    const bool aff_multi = epi_k != 1 && a.nseg > 1;
    if (aff_multi && legal && k.tile_rows == 512) return -1;
    return legal && !aff_multi && (k.tile_rows == 512 || (k.tile_rows == 0 && wide_env != 0 && fits));
}

// The decision.  Pure: writes nothing, calls no HIP function and no getenv, does not allocate.  The order of the error returns is part of the behaviour
// (tests/test_cabi_and_host.py).
inline MMLaunch mm_decide(const MMArgs& a, int dtype, const GswMmExtras& ex, const MMKnobs& k) {
    MMLaunch d{};
    auto fail = [](int status) { MMLaunch f{}; f.status = status; return f; };
    if (dtype != GSW_F16 && dtype != GSW_BF16) return fail(GSW_ERR_BAD_ARG);
    if (ex.colstats_capacity < 0 || ex.rowstats_capacity < 0 || ex.workspace_bytes < 0 || ex.max_splits < 0 || ex.max_splits > 64
        || ((uintptr_t)ex.colstats_dev & 15) || ((uintptr_t)ex.rowstats_dev & 7) || ((uintptr_t)ex.workspace_dev & 15)
        || (ex.flags & ~GSW_MM_GN_ONLY)) return fail(GSW_ERR_BAD_ARG);      // (unknown flag bits: a caller that filled the struct field by field without zeroing it)
    const int64_t ws_bytes = ex.workspace_bytes > 0 && ex.workspace_dev ? ex.workspace_bytes : 0;
    // N: any multiple of 8 (the last 160-column tile may be partial: weight rows are clamped, stores masked); GEGLU pairs columns inside a tile
    if (a.N % 8 || (a.mode == MM_MODE_GEGLU && a.N % 160) || a.M <= 0 || a.P <= 0) return fail(GSW_ERR_UNSUPPORTED);
    if (a.mode == MM_MODE_QKV && (a.n_rows <= 0 || a.n_rows % 160 || a.n_rows >= a.N || !a.y2)) return fail(GSW_ERR_UNSUPPORTED);
    // the dense-row / GEGLU epilogues fetch the bias by 16-byte LDS-DMA pieces (STG in the kernel)
    if ((a.mode == MM_MODE_DENSE || a.mode == MM_MODE_GEGLU) && ((uintptr_t)a.bias & 15u)) return fail(GSW_ERR_BAD_ARG);
    if (a.ln_stat && (a.mode != MM_MODE_DENSE && a.mode != MM_MODE_GEGLU && a.mode != MM_MODE_TRANS)) return fail(GSW_ERR_UNSUPPORTED);
    if (a.ln_stat && a.rowbias) return fail(GSW_ERR_UNSUPPORTED);
    constexpr int BN = 160;
    const int64_t tiles_n = (a.N + BN - 1) / BN;
    d.epi = a.mode == MM_MODE_QKV ? 5 : a.mode == MM_MODE_TRANS ? 3 : a.mode == MM_MODE_GEGLU ? 2 : (a.mode == MM_MODE_DENSE && !a.rowbias) ? 0 : 1;
    // panel of the tile order: 8 column tiles, or all of them when their weight tiles (tiles_n x 160 rows x K) stay under ~2 MiB of an XCD's 4 MiB L2
    d.panel = 8;
    if (tiles_n > 8 && tiles_n <= 32 && tiles_n * BN * (int64_t)a.P * 64 * 2 <= (2 << 20)) d.panel = (int32_t)tiles_n;
    if (k.panel > 0) d.panel = k.panel;
    const MMPlan plan = mm_plan(a.M, tiles_n, a.P, ws_bytes > 0 && ex.max_splits != 1 && !a.ln_stat, ex.max_splits, k);
    d.splits = 1; d.t_us = plan.t0_us;
    // Split-K for launches that cannot fill the chip with output tiles (the deep levels at small batch: 8 x 8 pixels of one image are ONE row tile
    // against 180-360 K stages): `splits` workgroups share a tile's stages, fp32 partials go through the caller's workspace, a second small kernel
    // adds them in a fixed order and runs the epilogue.  Needs a workspace (GswMmExtras); without one, or with one too small, the launch runs unsplit.
    if (plan.splits >= 2) {
        const int64_t nt = (((int64_t)a.M + plan.bm - 1) / plan.bm) * tiles_n;
        d.ws_need = (int64_t)plan.splits * nt * 8 * 5 * (plan.bm / 64) * 64 * 16;      // [splits][ntiles][8 waves][5 * MT accumulators][64 lanes] float4
        if (d.ws_need <= ws_bytes) {
            d.tile_rows = plan.bm; d.tile_cols = BN; d.mt = plan.bm / 64;      // both fit the 168 registers of the 12-wave form (152 / 100) without scratch
            d.splits = plan.splits; d.t_us = plan.t_us;
            d.tiles_n = (int32_t)tiles_n; d.ntiles = (int32_t)nt;
            d.grid = (uint32_t)((nt * plan.splits + 7) / 8 * 8);
            d.epi = 4; d.wave12 = true;
            return d;
        }
    }
    const int w = mm_wide(a, d.epi, tiles_n, k);
    if (w < 0) return fail(GSW_ERR_UNSUPPORTED);
    d.wide = w != 0;
    d.tile_rows = d.wide ? 256 : plan.bm0; d.tile_cols = d.wide ? 320 : BN; d.mt = d.wide ? 8 : plan.bm0 / 64;
    const int64_t tiles_nt = (a.N + d.tile_cols - 1) / d.tile_cols;
    const int64_t tiles_m = ((int64_t)a.M + d.tile_rows - 1) / d.tile_rows;
    if (tiles_m * tiles_nt > 0x7FFFFFFF) return fail(GSW_ERR_UNSUPPORTED);
    d.tiles_n = (int32_t)tiles_nt; d.ntiles = (int32_t)(tiles_m * tiles_nt);
    if (d.wide) {          // panel of the tile order for 320-column tiles: 4 (the same 1280 columns), or all of them under the same L2 budget
        d.panel = 4;
        if (tiles_nt > 4 && tiles_nt <= 16 && tiles_nt * 320 * (int64_t)a.P * 64 * 2 <= (2 << 20)) d.panel = (int32_t)tiles_nt;
    }
    d.grid = (uint32_t)std::min<int64_t>(k.cus, (d.ntiles + 7) / 8 * 8);
    // kernel form: LayerNorm-folded launches, the wide tile and the QKV epilogue run the 8-wave form; elsewhere the split mask's bit chooses -- except dense rows
    // on the 256-row tile, whose 12-wave form does not fit its 168 registers (32-40 bytes of scratch per lane) and is not instantiated
    d.lnf = a.ln_stat != nullptr;
    d.wave12 = !d.lnf && !d.wide && d.epi != 5 && !(d.epi == 0 && d.mt == 4) && ((k.split_mask >> d.epi) & 1);
    const int ngrp = d.wide ? 4 : 2, wmv = d.wide ? 2 : 4;        // 80-column groups per tile, waves along M
    // row statistics: plain dense-row launches (EPI 0), unsplit
    if (ex.rowstats_capacity > 0 && ex.rowstats_dev && d.epi == 0 && !d.lnf && (int64_t)a.M * ngrp * tiles_nt * 2 <= ex.rowstats_capacity)
        d.rowstats_slots = (int)(ngrp * tiles_nt);
    // column statistics: EPI 1 launches whose M dimension enumerates real pixels / tokens (interior enumeration or the token scatter), unsplit
    if (ex.colstats_capacity > 0 && ex.colstats_dev && (a.mode == MM_MODE_TOK2PF || ((a.mode == MM_MODE_PF || a.mode == MM_MODE_UP2X) && (a.flags & MM_FLAG_COMPACT)))
        && tiles_m * wmv * (int64_t)a.N <= ex.colstats_capacity) { d.colstats_rows_per_block = d.tile_rows / wmv; d.colstats_blocks = (int)(tiles_m * wmv); }
    return d;
}

// What the plan of a launch of M x N outputs over P stages predicts (microseconds) with these extras: the convolution front end chooses between its two row
// enumerations with it.
inline double mm_predict_us(int64_t M, int N, int P, const GswMmExtras& ex, const MMKnobs& k) {
    return mm_decide(mm_args_rows(nullptr, 0, 64 * P, nullptr, 0, nullptr, (int32_t)M, N), GSW_F16, ex, k).t_us;
}

