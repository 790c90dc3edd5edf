// gswm_pool_plan.h -- pool_decide: the whole launch policy and every refusal of gsw_pool_rows and gsw_trace_keyed_pooled_topk (gswm_pool.inc) as ONE pure
// function.  Host code only, plain C++17, integer arithmetic; the entry points fill the kernels' arguments from the plan and tests/pool_plan_cases.cpp sweeps it.
//
// Pooling.  The images of set g are the rows set_ptr[g] .. set_ptr[g + 1] - 1 (the caller gathered them); the pooled row has S_j = sum_b lev_bj (1 - 2 h_bj),
// sign bit S_j < 0 and level |S_j| as Q bit planes.  |S_j| <= Lmax * max_set with Lmax = 2^P - 1 (1 without planes), so Q = the bit length of that product holds
// every level; the caller states max_set, the largest set, because set_ptr lives on the device: a larger set than stated loses the bits above plane Q - 1 and
// nothing else (the kernel clips every image index to the batch).  Q <= POOL_MAX_Q = 10: 1023 images at unit levels, 68 at 15 levels.
//
// One workgroup per set; a lane owns one 32-bit word of the row (its 32 sums in registers) and the set's images are its inner loop.  The workgroup is the
// smallest power of two of lanes in 64 .. POOL_ROWS_WG that covers the row's words; longer rows are walked in steps of the workgroup.
//
// The search.  gsw_trace_keyed_soft_topk's record walk for Q planes: (1 + Q) rows per set are staged in LDS, each padded to whole 64-byte ChaCha blocks.  The set
// tile T is the largest of {1, 4, 16} that the sets fill and whose rows fit POOL_TILE_LDS = 128 KiB; T decides who computes, never what.  A lattice whose padded
// rows pass the 128 KiB at T = 1 is refused (only a ragged row within 64 (1 + Q) bytes of the domain's end: n_bits (1 + Q) > 1 048 576 is refused before it).
// Scores are exact int32: n_bits (2^Q - 1) < 2^31 is the condition, and the one under which wsum fits its int32.
//
// Refusals come in the order of the C ABI: BAD_ARG, then RAGGED, then UNSUPPORTED; a refusal decides nothing (every other field is zero).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/gswm.h"
#include "gswm_search_plan.h"   // KY_WAVES, KY_WG, SEARCH_LIST, search_grid_cap, search_workspace_bytes; gswm_record.h: records_layout_check, GSW_ROW_MAX_BITS

constexpr int POOL_MAX_Q = 10;                                   // planes of a pooled row, at most
constexpr int POOL_MAX_P = 4;                                    // planes of an image's row, at most (gsw_level_pack)
constexpr int POOL_ROWS_WG = 512;                                // lanes of a pooling workgroup, at most
constexpr uint32_t POOL_TILE_LDS = (uint32_t)(GSW_ROW_MAX_BITS / 8);   // the staged rows of one set tile: 128 KiB
constexpr int POOL_MAX_TILE = 16;

enum PoolKind { POOL_ROWS = 0, POOL_SEARCH = 1 };               // gsw_pool_rows, gsw_trace_keyed_pooled_topk

// What an entry point knows before it decides.  `G`: sets; `B`, `P`, `max_set`: pooling only; records and k: the search only.
// pointers_ok: every required pointer is present and aligned (pooling: signs, set_ptr (4), out_signs, out_planes, wsum (4), wsq (8), planes present exactly when
// P > 0; the search: signs, planes, wsum (4), idx, score, workspace); rows_aligned: signs and planes (and the outputs of pooling) are 4-byte aligned.
struct PoolQuery {
    int kind;
    bool pointers_ok, rows_aligned, records_present, records_aligned;
    int P, B, G, max_set, Q;
    int64_t n_bits, record_stride, n_records;
    int msg_bytes, k;
};

struct PoolPlan {
    int status;
    int Q;                    // planes of the pooled row
    int T;                    // search: sets per workgroup, 1, 4 or 16
    bool msg4;                // search: msg_bytes % 4 == 0
    int rowbytes, rowwords;   // n_bits / 8; its 32-bit words, the last one possibly partial
    int nblk;                 // search: ChaCha blocks per row
    int rows_aligned;         // rows are whole, 4-byte aligned dwords
    int grid_x, grid_y, wg;
    uint32_t lds;
    size_t ws_bytes;          // search: gsw_trace_keyed_workspace_bytes(G, n_records, k)
};

// the bit length of v >= 0
inline int pool_bit_length(int64_t v) {
    int q = 0;
    for (; v > 0; v >>= 1) ++q;
    return q;
}

// Q for sets of at most max_set images with P planes each (P = 0: unit levels); may pass POOL_MAX_Q, which pool_decide refuses
inline int pool_planes(int P, int64_t max_set) {
    return pool_bit_length(((int64_t)(P > 0 ? (1 << P) - 1 : 1)) * max_set);
}

inline PoolPlan pool_decide(const PoolQuery& q) {
    auto refuse = [](int status) { PoolPlan r{}; r.status = status; return r; };
    const bool search = q.kind == POOL_SEARCH;
    // ---- BAD_ARG
    if (!q.pointers_ok || q.G < 1 || q.n_bits < 1 || q.Q < 1) return refuse(GSW_ERR_BAD_ARG);
    int need = 0;
    if (!search) {
        if (q.P < 0 || q.P > POOL_MAX_P || q.B < 1 || q.G > q.B || q.max_set < 1 || q.max_set > q.B || q.n_bits % 8) return refuse(GSW_ERR_BAD_ARG);
        need = pool_planes(q.P, q.max_set);
        if (need <= POOL_MAX_Q && q.Q < need) return refuse(GSW_ERR_BAD_ARG);          // the planes would not hold the stated sets
    } else {
        if (q.k < 1 || q.k > SEARCH_LIST || q.n_records > (int64_t)INT32_MAX) return refuse(GSW_ERR_BAD_ARG);
        if (const int rc = records_layout_check(q.records_present, q.records_aligned, q.record_stride, q.msg_bytes, q.n_records); rc != GSW_OK) return refuse(rc);
        // ---- RAGGED
        if (q.n_bits % (8 * (int64_t)q.msg_bytes)) return refuse(GSW_ERR_RAGGED);
    }
    // ---- UNSUPPORTED
    if (q.Q > POOL_MAX_Q || need > POOL_MAX_Q) return refuse(GSW_ERR_UNSUPPORTED);
    if (q.n_bits * (1 + q.Q) > GSW_ROW_MAX_BITS || q.n_bits * ((1ll << q.Q) - 1) >= (1ll << 31)) return refuse(GSW_ERR_UNSUPPORTED);
    if (search && q.G > 65535) return refuse(GSW_ERR_UNSUPPORTED);                      // (the grid's second dimension)

    PoolPlan p{};
    p.Q = q.Q;
    p.rowbytes = (int)(q.n_bits / 8);
    p.rowwords = (p.rowbytes + 3) / 4;
    p.rows_aligned = p.rowbytes % 4 == 0 && q.rows_aligned;
    if (!search) {
        p.wg = 64;
        while (p.wg < POOL_ROWS_WG && p.wg < p.rowwords) p.wg <<= 1;
        p.grid_x = q.G;
        p.grid_y = 1;
        p.lds = 0;
        return p;
    }
    p.nblk = (p.rowbytes + 63) / 64;
    const uint32_t set_bytes = (uint32_t)(1 + q.Q) * (uint32_t)p.nblk * 64u;           // the rows of one set, padded to whole blocks
    if (set_bytes > POOL_TILE_LDS) return refuse(GSW_ERR_UNSUPPORTED);
    p.msg4 = q.msg_bytes % 4 == 0;
    p.T = q.G > 4 ? 16 : q.G > 1 ? 4 : 1;
    while (p.T > 1 && (uint32_t)p.T * set_bytes > POOL_TILE_LDS) p.T >>= 2;
    p.wg = KY_WG;
    p.grid_x = search_grid_cap(SEARCH_LEVEL, q.n_records);
    p.grid_y = (q.G + p.T - 1) / p.T;
    const uint32_t tail = (uint32_t)(KY_WAVES * p.T * SEARCH_LIST * sizeof(int64_t));  // what the top-k tail reuses
    p.lds = (uint32_t)p.T * set_bytes > tail ? (uint32_t)p.T * set_bytes : tail;
    p.ws_bytes = search_workspace_bytes(SEARCH_LEVEL, q.G, q.n_records, q.k);
    return p;
}
