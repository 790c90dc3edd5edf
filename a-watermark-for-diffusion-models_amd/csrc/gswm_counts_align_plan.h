// gswm_counts_align_plan.h -- counts_align_decide: the whole launch policy and every refusal of gsw_counts_align (gswm_counts_align.inc).  Pure host code, integer
// arithmetic only; the entry point fills the kernel's arguments from the plan and tests/counts_align_plan_cases.cpp sweeps it.  Include after include/gswm.h.
//
// Two paths, told apart by the message length M alone:
//   words (M % 32 == 0): a lane owns whole 32-bit words of the decrypted row, all of ONE message word (word w belongs to message word w mod M/32), and counts its
//                        32 positions in CA_PLANES bit-sliced vertical counters; `lanes` = the largest multiple of M/32 that a workgroup holds, so that a lane's
//                        message word never changes; the lanes past it idle (fewer than M/32 <= 64 of them)
//   bytes (any other M % 8 == 0): the same with bytes, M/8 message bytes and eight plain int32 counters per lane
// Either way the `groups` = lanes / units lanes that share a message unit leave their counts in the LDS reduction region (one uint8 per count on the word path, one
// uint16 on the byte path) and lane t sums its column: the stores of the M counts are coalesced dwords, no atomics anywhere.
//
// Counter widths.  A lane adds at most `lane_max` = ceil(units of the row / lanes) ones to a counter.  The row holds at most CA_MAX_BITS bits, so on the word path
// lane_max <= ceil(16384 / 193) = 85 <= CA_WORD_LANE_CAP (7 planes, one uint8 in LDS) and on the byte path lane_max <= ceil(65536 / 129) = 509 <= CA_BYTE_LANE_CAP
// (an int32 in registers, one uint16 in LDS); the sum over the groups is at most V = n_bits / M <= 65 536, an int32.  The plan refuses (UNSUPPORTED) a lane_max past
// its cap, which no accepted input reaches: the sweep holds it to that.
//
// LDS: [ row | keystream | reduction ], each region 16-byte aligned.  The row and its keystream are both staged (64 KiB each at most), so the longest row leaves
// one workgroup per CU (136 KiB of 160); the lattices in use (at most 4 x 128 x 128 at l = 4, 32 KiB + 32 KiB + 8 KiB) leave two, and at a 4 x 64 x 64 sign row (12 KiB)
// LDS no longer limits the occupancy.
//
// Chunk: align_decide's rule (gswm_align.inc).  A workgroup walks `chunk` alignments of one image after staging the row and generating the keystream once; the chunk
// grows to 16 only while the grid keeps 2048 workgroups (8 per CU).  The keystream costs about a quarter of one alignment's gather (about 2.5 lane operations per bit
// against about 12), so a chunk of 1 on a small grid wastes a fifth of the work of workgroups that would otherwise not exist at all.
#pragma once
#include <stdint.h>

constexpr int CA_WG = 256;
constexpr int64_t CA_MAX_BITS = 524288;       // the row and its keystream are both staged: 64 KiB each
constexpr int CA_MSG_MAX_BITS = 2048;
constexpr int CA_CHUNK_MAX = 16;              // alignments per workgroup, at most
constexpr int64_t CA_TARGET_WGS = 2048;       // the chunk shrinks while the grid would have fewer workgroups than this
constexpr int CA_PLANES = 7;                  // vertical counters of the word path
constexpr int CA_WORD_LANE_CAP = (1 << CA_PLANES) - 1;
constexpr int CA_BYTE_LANE_CAP = 65535;       // a uint16 in the reduction region
constexpr uint32_t CA_RED_BYTES = 8192;       // 256 lanes x 32 uint8 (words) >= 256 lanes x 8 uint16 (bytes)
constexpr uint32_t CA_LDS_CAP = 65536u + 65536u + CA_RED_BYTES;

struct CountsAlignPlan {
    int status;
    int words;                // 1: the word path
    int chunk;                // alignments per workgroup
    int grid_x, grid_y;       // (chunks, images)
    int rowbytes;
    int nblk;                 // 64-byte keystream blocks
    int units;                // message words (word path) or message bytes
    int lanes;                // lanes that count: a multiple of units, <= CA_WG
    int groups;               // lanes / units: the lanes that share a message unit
    int lane_max;             // the largest count one lane reaches
    int copies;               // V = n_bits / msg_bits: the largest count
    uint32_t off_ks, off_red; // byte offsets of the keystream and of the reduction region in LDS (the row is at 0)
    uint32_t lds;
};

// the launch decision: pure, host only.  pointers_ok: rows, aligns, key, nonce and counts present, aligns and counts 4-byte aligned
inline CountsAlignPlan counts_align_decide(bool pointers_ok, int B, int C, int H, int W, int l, int A, int msg_bits) {
    CountsAlignPlan p{};
    p.status = GSW_ERR_BAD_ARG;
    if (!pointers_ok || B < 1 || C < 1 || H < 1 || W < 1 || A < 1 || (l != 1 && l != 2 && l != 4)) return p;
    if (msg_bits < 8 || msg_bits > CA_MSG_MAX_BITS || msg_bits % 8 != 0) return p;
    const int64_t ch = (int64_t)C * H;        // (C, H, W < 2^31 each: no product overflows before it is compared)
    const auto n_mod = [&](int64_t m) { return (ch % m) * (W % m) % m * l % m; };          // n_bits mod m, whatever the size of n_bits
    if (n_mod(8) != 0 || n_mod(msg_bits) != 0) { p.status = GSW_ERR_RAGGED; return p; }
    p.status = GSW_ERR_UNSUPPORTED;
    if (ch > CA_MAX_BITS || ch * W > CA_MAX_BITS || ch * W * l > CA_MAX_BITS || B > 65535) return p;      // (B: the grid's second dimension)
    const int n_bits = (int)(ch * W * l);
    const int words = msg_bits % 32 == 0;
    const int units = words ? msg_bits / 32 : msg_bits / 8;
    const int lanes = CA_WG / units * units;
    const int row_units = words ? n_bits / 32 : n_bits / 8;
    const int lane_max = (row_units + lanes - 1) / lanes;
    if (lane_max > (words ? CA_WORD_LANE_CAP : CA_BYTE_LANE_CAP)) return p;
    p.words = words;
    p.units = units;
    p.lanes = lanes;
    p.groups = lanes / units;
    p.lane_max = lane_max;
    p.copies = n_bits / msg_bits;
    p.rowbytes = n_bits / 8;
    p.nblk = (p.rowbytes + 63) / 64;
    p.off_ks = (uint32_t)((p.rowbytes + 15) / 16 * 16);
    p.off_red = p.off_ks + 64u * (uint32_t)p.nblk;
    p.lds = p.off_red + CA_RED_BYTES;
    const int64_t want = (int64_t)A * B / CA_TARGET_WGS;
    p.chunk = (int)(want < 1 ? 1 : want > CA_CHUNK_MAX ? CA_CHUNK_MAX : want);
    p.grid_x = (int)(((int64_t)A + p.chunk - 1) / p.chunk);      // (A up to 2^31 - 1)
    p.grid_y = B;
    p.status = GSW_OK;
    return p;
}
