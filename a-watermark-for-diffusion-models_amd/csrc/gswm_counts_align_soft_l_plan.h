// gswm_counts_align_soft_l_plan.h -- level_counts_align_l_decide: the whole launch policy and every refusal of gsw_level_counts_align_l
// (gswm_counts_align_soft_l.inc).  Pure host code, integer arithmetic only; tests/level_counts_align_l_plan_cases.cpp sweeps it.  Include after
// include/gswm.h.
//
// It is level_counts_align_decide (gswm_counts_align_soft_plan.h: the paths, the widths, the LDS layout and the chunk are described there) with the row of
// Nb = n l cipher bits of a multi-bit window in place of the n bits of l = 1: once a lane holds aligned 32-bit words of the row nothing in the counting knows
// how many bits an element owns.  So the keystream is ceil(Nb / 512) blocks, msg_bits must divide Nb, V = Nb / msg_bits, a lane's largest count and the LDS
// cap are taken on Nb, and the domain is Nb (1 + P) <= 1 048 576.  At l = 1 every field equals level_counts_align_decide's; the sweep holds it to that.
//
// LDS at l = 4: a 4 x 64 x 64 lattice at P = 4 takes 40 + 8 + 32 KiB, as 4 x 128 x 128 does at l = 1; the largest accepted row is 524 288 bits at P = 1.
#pragma once
#include <stdint.h>

#include "gswm_counts_align_soft_plan.h"

// the launch decision: pure, host only.  pointers_ok as level_counts_align_decide takes it
inline LevelCountsAlignPlan level_counts_align_l_decide(bool pointers_ok, int l, int P, int B, int C, int H, int W, int A, int msg_bits, int32_t bias) {
    LevelCountsAlignPlan p{};
    p.status = GSW_ERR_BAD_ARG;
    if (!pointers_ok || (l != 1 && l != 2 && l != 4) || B < 1 || C < 1 || H < 1 || W < 1 || A < 1 || P < 1 || P > 4) return p;
    if (msg_bits < 8 || msg_bits > LCA_MSG_MAX_BITS || msg_bits % 8 != 0) return p;
    const int64_t ch = (int64_t)C * H;        // (C, H, W < 2^31 each: no product overflows before it is compared)
    const auto nb_mod = [&](int64_t m) { return (ch % m) * (W % m) % m * l % m; };         // Nb mod m, whatever the size of Nb
    if (nb_mod(8) != 0 || nb_mod(msg_bits) != 0) { p.status = GSW_ERR_RAGGED; return p; }
    p.status = GSW_ERR_UNSUPPORTED;
    if (ch > LCA_MAX_BITS || ch * W * l * (1 + P) > LCA_MAX_BITS || B > 65535) return p;   // (B: the grid's second dimension)
    const int nb = (int)(ch * W * l);
    const int rowbytes = nb / 8;
    const int padded = (rowbytes + 15) / 16 * 16;
    const int nblk = (rowbytes + 63) / 64;
    const int words = msg_bits % 32 == 0;
    const int units = words ? msg_bits / 32 : msg_bits / 8;
    const int lanes = LCA_WG / units * units;
    const uint32_t red_half = (uint32_t)lanes * (words ? 64u : 16u);                       // one uint16 per position and lane
    const uint32_t off_ks = (uint32_t)((1 + P) * padded);
    const uint32_t off_red = off_ks + 64u * (uint32_t)nblk;
    if (off_red + 2u * red_half > LCA_LDS_CAP) return p;
    const int row_units = words ? nb / 32 : nb / 8;
    const int lane_max = (row_units + lanes - 1) / lanes;
    if (lane_max > (words ? LCA_WORD_LANE_CAP : LCA_BYTE_LANE_CAP)) return p;
    const int64_t copies = nb / msg_bits;
    if ((bias < 0 ? -(int64_t)bias : (int64_t)bias) + LCA_MAX_LEVEL * copies > 2147483647ll) return p;
    p.words = words;
    p.units = units;
    p.lanes = lanes;
    p.groups = lanes / units;
    p.lane_max = lane_max;
    if (words)
        for (int v = lane_max; v; v >>= 1) ++p.cplanes;
    p.copies = (int)copies;
    p.rowbytes = rowbytes;
    p.lstride = padded;
    p.nblk = nblk;
    p.off_ks = off_ks;
    p.off_red = off_red;
    p.off_red_n = off_red + red_half;
    p.lds = off_red + 2u * red_half;
    const int64_t want = (int64_t)A * B / LCA_TARGET_WGS;
    p.chunk = (int)(want < 1 ? 1 : want > LCA_CHUNK_MAX ? LCA_CHUNK_MAX : want);
    p.grid_x = (int)(((int64_t)A + p.chunk - 1) / p.chunk);      // (A up to 2^31 - 1)
    p.grid_y = B;
    p.status = GSW_OK;
    return p;
}
