// gswm_tamper_plan.h -- the launch policy of the tamper family (csrc/gswm_tamper.hip: gsw_tile_agree, gsw_vote_tiled, gsw_decode_robust) as pure functions:
// tile_geometry maps a lattice to the ONE geometry all three kernels take by value, with the refusals the three entry points share in their order;
// tile_decide (map and vote) and robust_decide add their own refusals and the LDS of a launch.  Each maps (sizes, alignment facts, null pointers) to the
// complete decision -- status, geometry, LDS.  Plain C++17 on the host (tests/tamper_plan_cases.cpp sweeps it without a GPU); robust_isqrt is also what
// the kernel calls.
//
// LDS of a workgroup (one image), in bytes:  [64 nblk]      the row, padded to whole ChaCha blocks: ALL of it for the map and the vote; then, for the robust decode,
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

constexpr int TM_WG = 256;                           // the workgroup of all three kernels
constexpr uint32_t TM_LDS_CAP = 131072u;             // the cap every plan of the library keeps (of the CU's 160 KiB)
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

// The lattice as the kernels see it.  A kernel argument: plain ints, no pointers.
struct TileGeom {
    int C, h, w;
    int log2l, log2t;
    int tw, tiles;                 // tiles per lattice row, per image
    int n_t;                       // bits of a tile, C T^2 l
    int rowbytes, nblk;            // Nb / 8 (a multiple of 8); ChaCha blocks per row, the last one possibly partial
    int msg_bits, msg_bytes;
    int copies, log2s;             // Nb / msg_bits; lanes per message bit of the vote
};

inline int tile_ilog2(int v) {
    int r = 0;
    while ((1 << r) < v) ++r;
    return r;
}

// The refusals every entry point makes after its null pointers, in their order (BAD_ARG, UNSUPPORTED, RAGGED), then the geometry.  `aligned`: packed and keys
// are 4-byte aligned.  g is written only with GSW_OK.
inline int tile_geometry(TileGeom& g, int B, int C, int h, int w, int l, int tile, int msg_bits, bool aligned) {
    if (B < 1 || C < 1 || h < 1 || w < 1 || msg_bits < 1) return GSW_ERR_BAD_ARG;
    if (l != 1 && l != 2 && l != 4) return GSW_ERR_BAD_ARG;
    if (!aligned) return GSW_ERR_BAD_ARG;
    if (tile != 8 && tile != 16 && tile != 32) return GSW_ERR_UNSUPPORTED;
    if (h % tile || w % tile || msg_bits % 8) return GSW_ERR_UNSUPPORTED;
    const int64_t nb = (int64_t)C * h * w * l;
    if (nb > GSW_ROW_MAX_BITS) return GSW_ERR_UNSUPPORTED;
    if (nb % msg_bits) return GSW_ERR_RAGGED;
    g.C = C; g.h = h; g.w = w;
    g.log2l = tile_ilog2(l);
    g.log2t = tile_ilog2(tile);
    g.tw = w / tile;
    g.tiles = (h / tile) * g.tw;
    g.n_t = C * tile * tile * l;                                          // <= nb <= 2^20
    g.rowbytes = (int)(nb / 8);
    g.nblk = (g.rowbytes + 63) / 64;
    g.msg_bits = msg_bits;
    g.msg_bytes = msg_bits / 8;
    g.copies = (int)(nb / msg_bits);
    g.log2s = vote_log2s(msg_bits, g.copies, TM_WG);
    return GSW_OK;
}

// ---- the map (gsw_tile_agree) and the vote (gsw_vote_tiled): the row is all of their LDS
struct TileQuery {
    int B, C, h, w, l, tile, msg_bits;
    bool own_null;                 // the map's msg or agree; the vote's weights, bits, score or wsum
    bool weights_aligned;          // the vote's weights: 2 bytes
    bool packed_null, keys_null, packed_aligned, keys_aligned;           // 4 bytes
};

// The complete decision.  status != GSW_OK: the entry point returns it and every other field is zero.
struct TilePlan {
    int status;
    TileGeom g;
    int grid, wg;
    uint32_t lds;                  // dynamic LDS bytes: 64 nblk <= TM_LDS_CAP, the row's domain being GSW_ROW_MAX_BITS
};

inline TilePlan tile_decide(const TileQuery& q, bool vote) {
    auto refuse = [](int status) { TilePlan r{}; r.status = status; return r; };
    if (q.own_null || (vote && !q.weights_aligned)) return refuse(GSW_ERR_BAD_ARG);
    if (q.packed_null || q.keys_null) return refuse(GSW_ERR_BAD_ARG);
    TilePlan p{};                                                         // status GSW_OK
    const int rc = tile_geometry(p.g, q.B, q.C, q.h, q.w, q.l, q.tile, q.msg_bits, q.packed_aligned && q.keys_aligned);
    if (rc != GSW_OK) return refuse(rc);
    if (vote && (int64_t)p.g.copies * 65535 > (int64_t)INT32_MAX) return refuse(GSW_ERR_UNSUPPORTED);      // a message bit's score would not fit int32
    p.grid = q.B;
    p.wg = TM_WG;
    p.lds = 64u * (uint32_t)p.g.nblk;
    return p;
}

// ---- the robust decode (gsw_decode_robust)
// What the entry point knows before it decides.  The *_aligned facts are those of the POINTERS (signs, planes, keys: 4 bytes).
struct RobustQuery {
    int P, B, C, h, w, l, tile, msg_bits, iters, sign_rounds;
    bool signs_aligned, planes_aligned, keys_aligned;
    bool signs_null, planes_null, keys_null, outputs_null;      // planes_null only counts when P > 0
};

// The complete decision.  status != GSW_OK: the entry point returns it and every other field is zero.
struct RobustPlan {
    int status;
    TileGeom g;
    int lmax;                      // the largest level, max(1, 2^P - 1)
    int level_rounds;              // 1: some round votes with the levels (P > 0 and iters >= sign_rounds), wtot and wsq live in LDS
    int grid, wg;
    uint32_t planes_off, wgt_off, wtot_off, wsq_off, msg_off;   // byte offsets in LDS, each a multiple of 4
    uint32_t lds;                  // dynamic LDS bytes
};

inline RobustPlan robust_decide(const RobustQuery& q) {
    auto refuse = [](int status) { RobustPlan r{}; r.status = status; return r; };
    // ---- its own BAD_ARGs, the shared refusals in their order, then those of the rounds
    if (q.signs_null || q.keys_null || q.outputs_null) return refuse(GSW_ERR_BAD_ARG);
    if (q.P < 0 || q.P > RB_MAX_PLANES || q.iters < 0 || q.iters > RB_MAX_ITERS || (q.sign_rounds != 0 && q.sign_rounds != 1)) return refuse(GSW_ERR_BAD_ARG);
    if (q.P > 0 && (q.planes_null || !q.planes_aligned)) return refuse(GSW_ERR_BAD_ARG);
    RobustPlan p{};                                                       // status GSW_OK
    const int rc = tile_geometry(p.g, q.B, q.C, q.h, q.w, q.l, q.tile, q.msg_bits, q.signs_aligned && q.keys_aligned);
    if (rc != GSW_OK) return refuse(rc);
    if (8ll * p.g.rowbytes * (1 + q.P) > GSW_ROW_MAX_BITS) return refuse(GSW_ERR_UNSUPPORTED);
    const int64_t lmax = q.P > 0 ? (1 << q.P) - 1 : 1;
    // a bit's vote is at most lmax times a weight of at most lmax n_t: score, wsum (copies of them), excess (lmax n_t) and wsq (lmax^2 n_t) fit int32
    if (p.g.copies * lmax * lmax * p.g.n_t > (int64_t)INT32_MAX) return refuse(GSW_ERR_UNSUPPORTED);

    p.lmax = (int)lmax;
    p.level_rounds = q.P > 0 && q.iters >= q.sign_rounds;
    p.grid = q.B;
    p.wg = TM_WG;
    const uint64_t tile_words = 4ull * (uint64_t)p.g.tiles;
    uint64_t off = 64ull * (uint64_t)p.g.nblk;
    p.planes_off = (uint32_t)off;
    off += (uint64_t)q.P * (uint64_t)p.g.rowbytes;
    p.wgt_off = (uint32_t)off;
    off += tile_words;
    p.wtot_off = (uint32_t)off;
    off += p.level_rounds ? tile_words : 0ull;
    p.wsq_off = (uint32_t)off;
    off += p.level_rounds ? tile_words : 0ull;
    p.msg_off = (uint32_t)off;
    off += ((uint64_t)p.g.msg_bytes + 3ull) & ~3ull;
    if (off > TM_LDS_CAP) return refuse(GSW_ERR_UNSUPPORTED);
    p.lds = (uint32_t)off;
    return p;
}
