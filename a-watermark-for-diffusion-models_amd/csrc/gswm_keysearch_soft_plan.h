// gswm_keysearch_soft_plan.h -- the launch policy of the level-weighted blind key search (csrc/gswm_keysearch_soft.inc) as ONE pure function:
// key_soft_decide maps (sizes, alignment facts, null pointers) to the complete decision of a launch -- status, tile, template parameters, grid, the LDS
// layout, workspace.  Host code only, plain C++17, no HIP: tests/key_search_soft_plan_cases.cpp sweeps it without a GPU.  The workspace query answers through
// gswm_search_plan.h's search_workspace_bytes for the key search, which the grid is clipped by.
//
// LDS of a workgroup, in words:  [T][istride] the sign row and the P plane rows of every image of the tile (not with SG)
//                                [kpi][16 nblk] the keystreams of one step
//                                [T][nb][W]     W_t = sum of the levels at message position t, bit-sliced per message word (word path only)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>

#include "gswm_search_plan.h"   // KS_WG, KS_LDS, SEARCH_LIST, search_grid_cap, search_workspace_bytes, search_tile_images; gswm.h and gswm_record.h

// What the entry point knows before it decides.  The *_aligned facts are those of the POINTERS (signs, planes: 4 bytes; keys: 16).
struct KeySoftQuery {
    int B, P;                 // images; level planes (1 .. 4)
    int64_t n_bits, key_stride, n_keys;
    int msg_bytes, k;
    bool signs_aligned, planes_aligned, keys_aligned;
    bool signs_null, planes_null, keys_null, outputs_null;
};

// The complete decision.  status != GSW_OK: the entry point returns it and every other field is zero.
struct KeySoftPlan {
    int status;
    int T;                    // images per workgroup: 1, 4, 16 or 64
    int cp;                   // counter planes of the word path: 4, 8, 12, 16 or 18, the smallest class with (2^P - 1) V < 2^cp; 0: the bit-by-bit path
    int nb;                   // planes of W_t kept in LDS: the bit length of (2^P - 1) V (word path), else 0
    bool sg;                  // the rows stay in global memory: LDS holds the keystreams and W_t alone, T = 1
    int G, kpi, istride, copies;   // lanes per (key, image) pair, keys per step, words between two images' rows in LDS, V
    int rowbytes, nblk;       // n_bits / 8; ChaCha blocks per row, the last one possibly partial
    int rows_aligned;         // the sign and plane rows are whole, 4-byte aligned dwords
    int grid_x, grid_y, wg;
    uint32_t ks_off, w_off;   // byte offsets of the keystreams and of W_t in LDS
    uint32_t lds;             // dynamic LDS bytes, at least what the top-k tail reuses
    size_t ws_bytes;
};

inline int key_soft_counter_planes(int64_t amax) {
    return amax < 16 ? 4 : amax < 256 ? 8 : amax < 4096 ? 12 : amax < 65536 ? 16 : 18;
}

inline KeySoftPlan key_soft_decide(const KeySoftQuery& q) {
    auto refuse = [](int status) { KeySoftPlan r{}; r.status = status; return r; };
    // ---- the refusals, in the order of the C ABI: BAD_ARG, then RAGGED, then UNSUPPORTED
    if (q.signs_null || q.planes_null || q.keys_null || q.outputs_null) return refuse(GSW_ERR_BAD_ARG);
    if (q.B < 1 || q.k < 1 || q.k > SEARCH_LIST || q.n_bits < 1 || q.n_keys < 1 || q.n_keys > (int64_t)INT32_MAX) return refuse(GSW_ERR_BAD_ARG);
    if (q.P < 1 || q.P > 4 || q.msg_bytes < 1 || q.msg_bytes > GSW_MSG_INLINE_MAX) return refuse(GSW_ERR_BAD_ARG);
    if (q.key_stride < (int64_t)GSW_REC_HEAD || q.key_stride % 16 || !q.keys_aligned) return refuse(GSW_ERR_BAD_ARG);
    if (q.n_bits % (8 * (int64_t)q.msg_bytes)) return refuse(GSW_ERR_RAGGED);
    if (q.n_bits * (1 + q.P) > GSW_ROW_MAX_BITS || q.B > 65535) return refuse(GSW_ERR_UNSUPPORTED);

    KeySoftPlan p{};                                                      // status GSW_OK
    const int P = q.P;
    p.rowbytes = (int)(q.n_bits / 8);
    p.nblk = (p.rowbytes + 63) / 64;
    p.rows_aligned = (p.rowbytes % 4 == 0) && q.signs_aligned && q.planes_aligned;
    p.copies = (int)(q.n_bits / (8 * (int64_t)q.msg_bytes));
    const uint32_t rowpad = (uint32_t)p.nblk * 64u;                       // a row padded to whole blocks
    const int64_t amax = (int64_t)((1 << P) - 1) * p.copies;              // the largest sum of levels at one message position
    int nb = 0;
    while ((amax >> nb) != 0) ++nb;
    const bool word = q.msg_bytes % 4 == 0;
    const uint32_t wbytes = word ? (uint32_t)q.msg_bytes * (uint32_t)nb : 0u;   // W_t of one image: nb planes of msg_bytes / 4 words
    const uint32_t image_bytes = (uint32_t)(1 + P) * rowpad + 128u + wbytes;    // (128: the bank offset of istride)
    p.sg = image_bytes + rowpad > KS_LDS;                                 // an image's rows, its W_t and one keystream do not fit together
    const bool fast = word && (!p.sg || p.rows_aligned);                  // (from global memory the words are read in place)
    p.cp = fast ? key_soft_counter_planes(amax) : 0;
    p.nb = fast ? nb : 0;
    const int units = fast ? q.msg_bytes / 4 : 8 * q.msg_bytes;           // message words or message positions per (key, image) pair
    p.T = p.sg ? 1 : search_tile_images(q.B, image_bytes, KS_LDS / 2);
    p.G = 1;
    while (p.G < 64 && p.G < units) p.G <<= 1;
    while (KS_WG / p.G < p.T) p.G >>= 1;
    p.istride = (1 + P) * p.nblk * 16;
    if (!p.sg && p.G < 32)
        while (p.istride % 32 != p.G) ++p.istride;                        // groups of one 32-lane half read different banks
    const uint32_t row_bytes = p.sg ? 0u : (uint32_t)p.T * (uint32_t)p.istride * 4u;
    const uint32_t w_bytes = fast ? (uint32_t)p.T * wbytes : 0u;
    int64_t kpi = KS_WG / p.G / p.T;
    kpi = std::min<int64_t>(kpi, (KS_LDS - row_bytes - w_bytes) / rowpad);
    kpi = std::min<int64_t>(kpi, q.n_keys);
    p.kpi = (int)kpi;
    p.wg = KS_WG;
    p.grid_x = (int)std::min<int64_t>((q.n_keys + kpi - 1) / kpi, search_grid_cap(SEARCH_KEY, q.n_keys));
    p.grid_y = (q.B + p.T - 1) / p.T;
    p.ks_off = row_bytes;
    p.w_off = row_bytes + (uint32_t)kpi * rowpad;
    p.lds = std::max<uint32_t>(p.w_off + w_bytes, (uint32_t)(KS_WG / p.G * SEARCH_LIST * sizeof(int64_t)));
    p.ws_bytes = search_workspace_bytes(SEARCH_KEY, q.B, q.n_keys, q.k);
    return p;
}
