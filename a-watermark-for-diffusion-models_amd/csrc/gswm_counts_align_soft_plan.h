// gswm_counts_align_soft_plan.h -- level_counts_align_decide: the whole launch policy and every refusal of gsw_level_counts_align
// (gswm_counts_align_soft.inc).  Pure host code, integer arithmetic only; the entry point fills the kernel's arguments from the plan and
// tests/level_counts_align_plan_cases.cpp sweeps it.  Include after include/gswm.h.
//
// The paths are counts_align_decide's (gswm_counts_align_plan.h), told apart by the message length M alone:
//   words (M % 32 == 0): a lane owns whole 32-bit words of the decrypted row, all of ONE message word.  Per level plane k it keeps two sets of bit-sliced
//                        vertical counters over its 32 positions: X_k counts plane_k & d, N_k counts plane_k.  `cplanes` = the bit length of lane_max is how
//                        many counter planes are live (a lane that sees two words carries two planes, not seven).
//   bytes (any other M % 8 == 0): the same with bytes and plain int32 accumulators of level * d and of level, eight of each.
// Either way a lane combines its planes in registers, X' = sum_k 2^k X_k and N' = sum_k 2^k N_k per position, and leaves both as uint16 in the reduction
// region; lane t sums column t over the `groups` lanes that share its message unit and stores score = bias + 2 X' - N' and wsum = N' as coalesced dwords.
//
// Widths.  A lane adds at most lane_max = ceil(units of the row / lanes) to a counter: lane_max <= LCA_WORD_LANE_CAP = 127 (seven counter planes) on the word
// path, <= LCA_BYTE_LANE_CAP = 4369 on the byte path.  What a lane leaves in LDS is at most 15 lane_max: 1905 (words) and 65 535 (bytes), a uint16 either
// way, and on the word path two such values share a dword in registers without a carry between them.  The column sums are at most 15 V < 2^24; the plan
// refuses a |bias| + 15 V beyond int32.  No accepted lattice reaches a lane cap (the LDS cap binds first: at most 8192 words over 193 lanes, 32 768 bytes
// over 129); the sweep holds the plan to that.
//
// LDS: [ 1 + P rows, each padded to 16 bytes | keystream | reduction: X' then N' ], every region 16-byte aligned.  The reduction region is lanes x 128 bytes
// on the word path (32 KiB at most) and lanes x 32 bytes on the byte path.  LCA_LDS_CAP = 128 KiB: a 4 x 128 x 128 lattice at P = 4 takes 40 + 8 + 32 KiB
// (two workgroups per CU), a 4 x 64 x 64 one 10 + 2 + 32 KiB (three); the largest accepted, 4 x 256 x 256 at P = 1, takes the cap exactly.
//
// Chunk: counts_align_decide's rule, for the same reason (the rows and the keystream are staged once per workgroup).
#pragma once
#include <stdint.h>

constexpr int LCA_WG = 256;
constexpr int LCA_MSG_MAX_BITS = 2048;
constexpr int LCA_CHUNK_MAX = 16;             // alignments per workgroup, at most
constexpr int64_t LCA_TARGET_WGS = 2048;      // the chunk shrinks while the grid would have fewer workgroups than this
constexpr int LCA_PLANES = 7;                 // vertical counter planes of the word path, at most
constexpr int LCA_MAX_LEVEL = 15;             // the largest level P = 4 planes hold
constexpr int LCA_WORD_LANE_CAP = (1 << LCA_PLANES) - 1;
constexpr int LCA_BYTE_LANE_CAP = 65535 / LCA_MAX_LEVEL;      // 15 lane_max is a uint16 in the reduction region
constexpr uint32_t LCA_LDS_CAP = 131072u;
constexpr int64_t LCA_MAX_BITS = 1048576;     // GSW_ROW_MAX_BITS: n (1 + P) of the level rows

struct LevelCountsAlignPlan {
    int status;
    int words;                // 1: the word path
    int chunk;                // alignments per workgroup
    int grid_x, grid_y;       // (chunks, images)
    int rowbytes;
    int lstride;              // bytes between two rows of the image in LDS
    int nblk;                 // 64-byte keystream blocks
    int units;                // message words (word path) or message bytes
    int lanes;                // lanes that count: a multiple of units, <= LCA_WG
    int groups;               // lanes / units: the lanes that share a message unit
    int lane_max;             // the largest count one lane reaches in one plane
    int cplanes;              // word path: live counter planes, the bit length of lane_max (0 on the byte path)
    int copies;               // V = n / msg_bits
    uint32_t off_ks, off_red, off_red_n;   // byte offsets in LDS of the keystream, of X' and of N' (the rows start at 0)
    uint32_t lds;
};

// the launch decision: pure, host only.  pointers_ok: signs, planes, aligns, key, nonce and score present, aligns, score and a present wsum 4-byte aligned
inline LevelCountsAlignPlan level_counts_align_decide(bool pointers_ok, int P, int B, int C, int H, int W, int A, int msg_bits, int32_t bias) {
    LevelCountsAlignPlan p{};
    p.status = GSW_ERR_BAD_ARG;
    if (!pointers_ok || B < 1 || C < 1 || H < 1 || W < 1 || A < 1 || P < 1 || P > 4) return p;
    if (msg_bits < 8 || msg_bits > LCA_MSG_MAX_BITS || msg_bits % 8 != 0) return p;
    const int64_t ch = (int64_t)C * H;        // (C, H, W < 2^31 each: no product overflows before it is compared)
    const auto n_mod = [&](int64_t m) { return (ch % m) * (W % m) % m; };                  // n mod m, whatever the size of n
    if (n_mod(8) != 0 || n_mod(msg_bits) != 0) { p.status = GSW_ERR_RAGGED; return p; }
    p.status = GSW_ERR_UNSUPPORTED;
    if (ch > LCA_MAX_BITS || ch * W * (1 + P) > LCA_MAX_BITS || B > 65535) return p;       // (B: the grid's second dimension)
    const int n = (int)(ch * W);
    const int rowbytes = n / 8;
    const int padded = (rowbytes + 15) / 16 * 16;
    const int nblk = (rowbytes + 63) / 64;
    const int words = msg_bits % 32 == 0;
    const int units = words ? msg_bits / 32 : msg_bits / 8;
    const int lanes = LCA_WG / units * units;
    const uint32_t red_half = (uint32_t)lanes * (words ? 64u : 16u);                       // one uint16 per position and lane
    const uint32_t off_ks = (uint32_t)((1 + P) * padded);
    const uint32_t off_red = off_ks + 64u * (uint32_t)nblk;
    if (off_red + 2u * red_half > LCA_LDS_CAP) return p;
    const int row_units = words ? n / 32 : n / 8;
    const int lane_max = (row_units + lanes - 1) / lanes;
    if (lane_max > (words ? LCA_WORD_LANE_CAP : LCA_BYTE_LANE_CAP)) return p;
    const int64_t copies = n / msg_bits;
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
