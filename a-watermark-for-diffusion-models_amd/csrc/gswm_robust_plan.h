// gswm_robust_plan.h -- the launch policy of the one-launch robust decode (csrc/gswm_tamper_soft.inc: gsw_decode_robust) as ONE pure function:
// robust_decide maps (sizes, alignment facts, null pointers) to the complete decision of a launch -- status, geometry, lanes per message bit, the LDS layout.
// Plain C++17 on the host (tests/robust_plan_cases.cpp sweeps it without a GPU); robust_isqrt is also what the kernel calls.
//
// LDS of a workgroup (one image), in bytes:  [64 nblk]      p = q ^ ks, the decrypted row, padded to whole ChaCha blocks
//                                            [P][rowbytes]  the level planes
//                                            [tiles] int32  wgt, the tile weights of the round
//                                            [tiles] int32  wtot = sum of the levels of a tile  (only when a round votes with the levels)
//                                            [tiles] int32  wsq  = sum of their squares         (only when a round votes with the levels)
//                                            [msg_bytes]    the message the round decoded, padded to a dword
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/gswm.h"
#include "gswm_record.h"   // GSW_ROW_MAX_BITS, vote_log2s

#if defined(__HIPCC__)
#define GSW_ROBUST_HD __host__ __device__
#else
#define GSW_ROBUST_HD
#endif

constexpr int RB_WG = 256;
constexpr uint32_t RB_LDS_CAP = 131072u;             // the cap every plan of the library keeps (of the CU's 160 KiB)
constexpr int RB_MAX_PLANES = 4, RB_MAX_ITERS = 8;

// floor(sqrt(v)), exactly, for every 32-bit v: the digit-by-digit method, integers only, 16 steps
GSW_ROBUST_HD inline uint32_t robust_isqrt(uint32_t v) {
    uint32_t r = 0u;
    for (uint32_t bit = 1u << 30; bit != 0u; bit >>= 2) {
        const uint32_t t = r + bit;
        r >>= 1;
        if (v >= t) {
            v -= t;
            r += bit;
        }
    }
    return r;
}

// What the entry point knows before it decides.  The *_aligned facts are those of the POINTERS (signs, planes, keys: 4 bytes).
struct RobustQuery {
    int P, B, C, h, w, l, tile, msg_bits, iters, sign_rounds;
    bool signs_aligned, planes_aligned, keys_aligned;
    bool signs_null, planes_null, keys_null, outputs_null;      // planes_null only counts when P > 0
};

// The complete decision.  status != GSW_OK: the entry point returns it and every other field is zero.
struct RobustPlan {
    int status;
    int log2l, log2t, tw, tiles;   // tiles per lattice row, per image
    int n_t, lmax;                 // bits of a tile, C T^2 l; the largest level, max(1, 2^P - 1)
    int rowbytes, nblk;            // Nb / 8 (a multiple of 8); ChaCha blocks per row, the last one possibly partial
    int msg_bytes, copies, log2s;  // Nb / msg_bits; lanes per message bit of the vote
    int level_rounds;              // 1: some round votes with the levels (P > 0 and iters >= sign_rounds), wtot and wsq live in LDS
    int grid, wg;
    uint32_t planes_off, wgt_off, wtot_off, wsq_off, msg_off;   // byte offsets in LDS, each a multiple of 4
    uint32_t lds;                  // dynamic LDS bytes
};

inline RobustPlan robust_decide(const RobustQuery& q) {
    auto refuse = [](int status) { RobustPlan r{}; r.status = status; return r; };
    // ---- the refusals of gsw_vote_tiled in its order (BAD_ARG, UNSUPPORTED, RAGGED), then those of the rounds
    if (q.signs_null || q.keys_null || q.outputs_null) return refuse(GSW_ERR_BAD_ARG);
    if (q.P < 0 || q.P > RB_MAX_PLANES || q.iters < 0 || q.iters > RB_MAX_ITERS || (q.sign_rounds != 0 && q.sign_rounds != 1)) return refuse(GSW_ERR_BAD_ARG);
    if (q.P > 0 && (q.planes_null || !q.planes_aligned)) return refuse(GSW_ERR_BAD_ARG);
    if (q.B < 1 || q.C < 1 || q.h < 1 || q.w < 1 || q.msg_bits < 1) return refuse(GSW_ERR_BAD_ARG);
    if (q.l != 1 && q.l != 2 && q.l != 4) return refuse(GSW_ERR_BAD_ARG);
    if (!q.signs_aligned || !q.keys_aligned) return refuse(GSW_ERR_BAD_ARG);
    if (q.tile != 8 && q.tile != 16 && q.tile != 32) return refuse(GSW_ERR_UNSUPPORTED);
    if (q.h % q.tile || q.w % q.tile || q.msg_bits % 8) return refuse(GSW_ERR_UNSUPPORTED);
    const int64_t nb = (int64_t)q.C * q.h * q.w * q.l;
    if (nb > GSW_ROW_MAX_BITS) return refuse(GSW_ERR_UNSUPPORTED);
    if (nb % q.msg_bits) return refuse(GSW_ERR_RAGGED);
    if (nb * (1 + q.P) > GSW_ROW_MAX_BITS) return refuse(GSW_ERR_UNSUPPORTED);
    const int64_t lmax = q.P > 0 ? (1 << q.P) - 1 : 1;
    const int64_t n_t = (int64_t)q.C * q.tile * q.tile * q.l, copies = nb / q.msg_bits;      // n_t <= nb <= 2^20
    // a bit's vote is at most lmax times a weight of at most lmax n_t: score, wsum (copies of them), excess (lmax n_t) and wsq (lmax^2 n_t) fit int32
    if (copies * lmax * lmax * n_t > (int64_t)INT32_MAX) return refuse(GSW_ERR_UNSUPPORTED);

    RobustPlan p{};                                                       // status GSW_OK
    while ((1 << p.log2l) < q.l) ++p.log2l;
    while ((1 << p.log2t) < q.tile) ++p.log2t;
    p.tw = q.w / q.tile;
    p.tiles = (q.h / q.tile) * p.tw;
    p.n_t = (int)n_t;
    p.lmax = (int)lmax;
    p.rowbytes = (int)(nb / 8);
    p.nblk = (p.rowbytes + 63) / 64;
    p.msg_bytes = q.msg_bits / 8;
    p.copies = (int)copies;
    p.log2s = vote_log2s(q.msg_bits, copies, RB_WG);
    p.level_rounds = q.P > 0 && q.iters >= q.sign_rounds;
    p.grid = q.B;
    p.wg = RB_WG;
    const uint64_t tile_words = 4ull * (uint64_t)p.tiles;
    uint64_t off = 64ull * (uint64_t)p.nblk;
    p.planes_off = (uint32_t)off;
    off += (uint64_t)q.P * (uint64_t)p.rowbytes;
    p.wgt_off = (uint32_t)off;
    off += tile_words;
    p.wtot_off = (uint32_t)off;
    off += p.level_rounds ? tile_words : 0ull;
    p.wsq_off = (uint32_t)off;
    off += p.level_rounds ? tile_words : 0ull;
    p.msg_off = (uint32_t)off;
    off += ((uint64_t)p.msg_bytes + 3ull) & ~3ull;
    if (off > RB_LDS_CAP) return refuse(GSW_ERR_UNSUPPORTED);
    p.lds = (uint32_t)off;
    return p;
}
