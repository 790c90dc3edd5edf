// gswm_search_plan.h -- the launch policy of the searches over packed sign rows (csrc/gswm_keyed.hip with gswm_keyed_soft.inc and gswm_keysearch.inc) as ONE pure
// function: search_decide maps (which search, sizes, alignment facts, null pointers) to the complete decision of a launch -- status, tile, template parameters,
// grid, LDS, workspace.  Host code only, plain C++17, no HIP: it compiles with the host compiler alone, so the policy can be tabulated without a GPU
// (tests/test_search_plan_host.py against tests/golden/search_plan_cases.tsv).  The two workspace queries answer through search_workspace_bytes, which
// search_decide's grid_x is clipped by: a launch cannot use a grid the workspace was not sized for.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>

#include "../../include/gswm.h"
#include "gswm_record.h"   // GSW_REC_HEAD, GSW_ROW_MAX_BITS, records_layout_check

constexpr int SEARCH_LIST = 8;                       // entries of a running top-k list (gswm_topk.h's TR_LIST): k <= 8
// the record walks (sign and level-weighted search): one record per wave at a time
constexpr int KY_WAVES = 8;
constexpr int KY_WG = 64 * KY_WAVES;
constexpr int KY_MAX_GRID_X = 512;                   // record ranges (two rounds of one workgroup per CU at the largest tiles)
constexpr uint32_t KY_TILE_LDS = (uint32_t)(GSW_ROW_MAX_BITS / 8);   // rows of one image tile: one image of the largest lattice
// the key search: G lanes per (key, image) pair
constexpr int KS_WG = 256;
constexpr int KS_MAX_GRID_X = 512;
constexpr uint32_t KS_LDS = (uint32_t)(GSW_ROW_MAX_BITS / 8);        // sign rows of the tile + keystreams of one step

enum SearchKind { SEARCH_SIGN = 0, SEARCH_LEVEL = 1, SEARCH_KEY = 2 };   // gsw_trace_keyed_topk, gsw_trace_keyed_soft_topk, gsw_key_search_topk

// What an entry point knows before it decides.  The *_aligned facts are those of the POINTERS (signs, planes, wsum: 4 bytes; records: 16); `outputs_null`: idx, score or
// the workspace is null.  planes / wsum / levels count for SEARCH_LEVEL only.
struct SearchQuery {
    int kind, B;
    int64_t n_bits, record_stride, n_records;
    int msg_bytes, k, levels;
    bool signs_aligned, planes_aligned, wsum_aligned, records_aligned;
    bool signs_null, planes_null, wsum_null, records_null, outputs_null;
};

// The complete decision for one search.  status != GSW_OK: the entry point returns it and every other field is zero.
struct SearchPlan {
    int status;
    int T;                    // images per workgroup: 1, 4, 16 or 64
    bool msg4;                // record walks: msg_bytes % 4 == 0 (message read as dwords)
    int planes;               // level search: P = bit length of `levels`; key search: PL counter planes (0: the bit-by-bit path); sign search: 0
    bool sg;                  // key search: the row stays in global memory, LDS holds the keystream alone
    int G, kpi, srow, copies; // key search: lanes per (key, image) pair, keys per step, words between two sign rows in LDS, V
    int rowbytes, nblk;       // n_bits / 8; ChaCha blocks per row, the last one possibly partial
    int signs_aligned;        // the rows (sign and plane) are whole, 4-byte aligned dwords
    int grid_x, grid_y, wg;
    uint32_t lds;             // dynamic LDS bytes: the staged rows (and keystreams), at least what the top-k tail reuses
    size_t ws_bytes;          // what the workspace query answers for (B, n_records, k)
};

// record ranges a launch may use at most: what the workspace is sized for
inline int search_grid_cap(int kind, int64_t n_records) {
    if (kind == SEARCH_KEY) return (int)std::min<int64_t>(n_records, KS_MAX_GRID_X);
    return (int)std::min<int64_t>((n_records + KY_WAVES - 1) / KY_WAVES, KY_MAX_GRID_X);
}

// [B, grid cap, k] int64 keys; 0: a bad argument
inline size_t search_workspace_bytes(int kind, int B, int64_t n_records, int k) {
    if (B < 1 || n_records < 1 || n_records > (int64_t)INT32_MAX || k < 1 || k > SEARCH_LIST) return 0;
    return (size_t)B * (size_t)search_grid_cap(kind, n_records) * (size_t)k * sizeof(int64_t);
}

// images per workgroup: the smallest tile that holds the batch (at most 64), divided by four until its `image_bytes` per image fit `budget`
inline int search_tile_images(int B, uint32_t image_bytes, uint32_t budget) {
    int t = B > 16 ? 64 : B > 4 ? 16 : B > 1 ? 4 : 1;
    while (t > 1 && (uint32_t)t * image_bytes > budget) t >>= 2;
    return t;
}

inline SearchPlan search_decide(const SearchQuery& q) {
    auto refuse = [](int status) { SearchPlan r{}; r.status = status; return r; };
    const bool key = q.kind == SEARCH_KEY, level = q.kind == SEARCH_LEVEL;
    // ---- the refusals, in the order of the C ABI: BAD_ARG, then RAGGED, then UNSUPPORTED
    if (q.signs_null || q.outputs_null || (key && q.records_null) || (level && (q.planes_null || q.wsum_null))) return refuse(GSW_ERR_BAD_ARG);
    if (q.B < 1 || q.k < 1 || q.k > SEARCH_LIST || q.n_bits < 1 || q.n_records > (int64_t)INT32_MAX) return refuse(GSW_ERR_BAD_ARG);
    if (level && (q.levels < 1 || q.levels > 15 || !q.wsum_aligned)) return refuse(GSW_ERR_BAD_ARG);
    if (key) {                                                            // a key row is a record's head: no message, so the stride need not hold one
        if (q.n_records < 1 || q.msg_bytes < 1 || q.msg_bytes > GSW_MSG_INLINE_MAX) return refuse(GSW_ERR_BAD_ARG);
        if (q.record_stride < (int64_t)GSW_REC_HEAD || q.record_stride % 16 || !q.records_aligned) return refuse(GSW_ERR_BAD_ARG);
    } else if (const int rc = records_layout_check(!q.records_null, q.records_aligned, q.record_stride, q.msg_bytes, q.n_records); rc != GSW_OK) return refuse(rc);
    if (q.n_bits % (8 * (int64_t)q.msg_bytes)) return refuse(GSW_ERR_RAGGED);
    const int P = !level ? 0 : q.levels < 2 ? 1 : q.levels < 4 ? 2 : q.levels < 8 ? 3 : 4;      // the bit length of `levels`
    if (q.n_bits * (1 + P) > GSW_ROW_MAX_BITS || q.B > 65535) return refuse(GSW_ERR_UNSUPPORTED);

    SearchPlan p{};                                                       // status GSW_OK
    p.rowbytes = (int)(q.n_bits / 8);
    p.nblk = (p.rowbytes + 63) / 64;
    p.signs_aligned = (p.rowbytes % 4 == 0) && q.signs_aligned && (!level || q.planes_aligned);
    const uint32_t rowpad = (uint32_t)p.nblk * 64u;                       // a row padded to whole blocks
    if (!key) {
        // the record walks: the tile's (1 + P) rows per image fit the 128 KiB; T decides who computes, never what
        p.msg4 = q.msg_bytes % 4 == 0;
        p.planes = P;
        p.T = search_tile_images(q.B, (uint32_t)(1 + P) * rowpad, KY_TILE_LDS);
        p.wg = KY_WG;
        p.grid_x = search_grid_cap(q.kind, q.n_records);
        p.lds = std::max<uint32_t>((uint32_t)(1 + P) * (uint32_t)p.T * rowpad, (uint32_t)(KY_WAVES * p.T * SEARCH_LIST * sizeof(int64_t)));
    } else {
        p.copies = (int)(q.n_bits / (8 * (int64_t)q.msg_bytes));
        p.sg = 2u * (rowpad + 128u) > KS_LDS;                             // a (padded) row and one keystream of it do not fit together
        const bool fast = q.msg_bytes % 4 == 0 && (!p.sg || p.signs_aligned);   // (from global memory the words are read in place)
        p.planes = !fast ? 0 : p.copies < 16 ? 4 : p.copies < 256 ? 8 : p.copies < 4096 ? 12 : 16;
        const int units = fast ? q.msg_bytes / 4 : 8 * q.msg_bytes;       // message words or message positions per (key, image) pair
        p.T = p.sg ? 1 : search_tile_images(q.B, rowpad + 128u, KS_LDS / 2);
        p.G = 1;
        while (p.G < 64 && p.G < units) p.G <<= 1;
        while (KS_WG / p.G < p.T) p.G >>= 1;
        p.srow = p.nblk * 16;
        if (!p.sg && p.G < 32)
            while (p.srow % 32 != p.G) ++p.srow;                          // groups of one 32-lane half read different banks
        const uint32_t sign_bytes = p.sg ? 0u : (uint32_t)p.T * (uint32_t)p.srow * 4u;
        int64_t kpi = KS_WG / p.G / p.T;
        kpi = std::min<int64_t>(kpi, (KS_LDS - sign_bytes) / rowpad);
        kpi = std::min<int64_t>(kpi, q.n_records);
        p.kpi = (int)kpi;
        p.wg = KS_WG;
        p.grid_x = (int)std::min<int64_t>((q.n_records + kpi - 1) / kpi, search_grid_cap(q.kind, q.n_records));
        p.lds = std::max<uint32_t>(sign_bytes + (uint32_t)kpi * rowpad, (uint32_t)(KS_WG / p.G * SEARCH_LIST * sizeof(int64_t)));
    }
    p.grid_y = (q.B + p.T - 1) / p.T;
    p.ws_bytes = search_workspace_bytes(q.kind, q.B, q.n_records, q.k);
    return p;
}
