// gswm_attn_plan.h -- the launch policy of the flash-attention kernel (csrc/gswm_attn.hip) as ONE pure function: attn_decide maps (shape, workspace size, switches)
// to the complete decision of a launch -- status, query blocks per wave, kernel form, key split, grid, dynamic LDS, workspace needed.  Host code only, plain C++17,
// no HIP: it compiles with the host compiler alone, so the policy can be tabulated without a GPU (tests/test_attn_plan_host.py against
// tests/golden/attn_plan_cases.tsv).  gsw_attention_ws checks what the policy cannot see (pointers, dtype, row strides), calls attn_decide and launches what it says.
#pragma once
#include <stdint.h>
#include <algorithm>

#include "../../include/gswm.h"

// The environment values the policy reads (gswm_attn.hip reads each once per process; A/B switches for profiling and tests).
//   qb    GSW_ATTN_QB: 2 (default) 256-query workgroups where the rule below takes them; 1 never; 3 wherever the shape allows
//   pair  GSW_ATTN_PAIR: 0 switches the four-stage loop off (default 1)
//   dma   GSW_ATTN_DMA: 0 selects the register staging at head_dim 64 (default 1)
//   kvs   GSW_ATTN_KVS: 0 switches the key-split form off; k > 1 forces k ways from 8 key tiles up (default 1)
struct AttnSwitches {
    int qb, pair, dma, kvs;
};

// The complete decision for one launch.  status != GSW_OK: the launch returns it and every other field is zero.
struct AttnLaunch {
    int status;
    int QB;                   // 32-query blocks per wave: 1 = 128 queries per workgroup, 2 = 256
    bool ragged;              // Sq off the 128-query tile and / or Sk off the 64-key tile: clamped loads, masked keys, guarded stores (QB 1, two stages)
    bool pair;                // four LDS stages, one barrier per two key tiles
    bool dma;                 // pair + K / V^T tiles by LDS-DMA into four static stages (head_dim 64, a multiple of four key tiles)
    uint32_t ksplit;          // > 1: key-split form, `ksplit` workgroups per query tile + the combine kernel (QB 1, two stages)
    uint32_t nqt, total;      // query tiles per (batch, head); nqt * B * H
    uint32_t grid;            // workgroups of the forward kernel: total * ksplit
    uint32_t lds_bytes;       // dynamic LDS of the forward kernel (0 for the DMA form: its stages are static)
    int64_t ws_need;          // bytes of workspace the key-split plan needs (0: no such plan); ksplit == 1 with ws_need > 0: it did not fit
};

// one LDS stage: a 64-key K tile (row pitch: the head's 32-byte k-slices + 16 B) and a V^T tile (head rows in blocks of 32, + a 16-row tail; pitch 144 B)
inline uint32_t attn_stage_bytes(int head_dim) {
    const int DU = head_dim / 8, KC = (DU + 1) / 2, DBF = head_dim / 32, TR = head_dim % 32;
    return (uint32_t)(64 * (KC * 32 + 16) + (DBF * 32 + (TR ? 16 : 0)) * 144);
}

// q [B, Sq, >= H*head_dim], k [B, Sk, >= H*head_dim], vt [B, H*head_dim, Sk]; head_dim 40 / 64 / 80 / 160; any Sq; Sk % 8 == 0; keys in [Sk_valid, Sk) are padding.
// workspace_bytes: what the caller offers for the key-split form (0: none).
inline AttnLaunch attn_decide(int B, int H, int head_dim, int Sq, int Sk, int Sk_valid, int64_t workspace_bytes, const AttnSwitches& sw) {
    AttnLaunch d{};
    if (workspace_bytes < 0 || B <= 0 || H <= 0 || Sq <= 0 || Sk <= 0 || Sk_valid <= 0 || Sk_valid > Sk) { d.status = GSW_ERR_BAD_ARG; return d; }
    if ((head_dim != 40 && head_dim != 64 && head_dim != 80 && head_dim != 160) || (Sk & 7)) { d.status = GSW_ERR_UNSUPPORTED; return d; }
    const bool ragged = (Sq & 127) || (Sk & 63);
    // 256-query workgroups once there are plenty of them (7-12 % faster from ~1000 workgroups up); below ~400 of them the 128-query form keeps more CUs
    // busy (one image at 64 x 64: 62 vs 91 us; profiles/r03y_attention_query_tile_sweep.txt)
    const int64_t wg256 = (int64_t)(Sq / 256) * B * H;
    const int QB = ((Sq & 255) == 0 && Sq >= 512 && sw.qb >= 2 && head_dim < 80 && !ragged && (wg256 > 400 || sw.qb == 3)) ? 2 : 1;
    const int64_t nqt = ((int64_t)Sq + 128 * QB - 1) / (128 * QB), total = nqt * B * H;      // (64-bit: Sq + 255 overflows an int from Sq = 2^31 - 255 up)
    if (total > 0x7FFFFFFF) { d.status = GSW_ERR_UNSUPPORTED; return d; }
    d.status = GSW_OK;
    d.QB = QB; d.ragged = ragged;
    d.nqt = (uint32_t)nqt; d.total = (uint32_t)total; d.grid = d.total; d.ksplit = 1;
    const uint32_t stage = attn_stage_bytes(head_dim);
    const int32_t nt = Sk >> 6;
    // Key-split form: few query tiles against many key tiles (one image's self-attention at 64 x 64: 62 -> 49 us).  As many splits as keep every workgroup
    // resident at once (2 per CU); only from 32 key tiles up -- the second launch and the partial results cost ~12 us, and at 16 tiles (32 x 32: 17.6 -> 21.4 us)
    // that is more than the split saves.  Needs the caller's workspace; kvs = 0 switches it off (A/B), k > 1 forces k ways from 8 tiles up.
    if (QB == 1 && (head_dim == 64 || head_dim == 40) && !ragged && sw.kvs && workspace_bytes > 0 && Sk_valid == Sk && total <= 256 && nt >= (sw.kvs > 1 ? 8 : 32)) {
        uint32_t ksplit = (uint32_t)std::min<int64_t>(std::min<int64_t>(512 / total, nt / 4), 8);
        if (sw.kvs > 1) ksplit = (uint32_t)std::min<int>(sw.kvs, nt);                                   // (tests: force a split count)
        if (ksplit >= 2) {
            const int nacc = head_dim / 32 * 16 + (head_dim % 32 ? 8 : 0);      // accumulator registers per lane; a partial record adds the running maximum and the row sum
            d.ws_need = total * ksplit * 4 * (nacc + 2) * 64 * (int64_t)sizeof(float);
            if (d.ws_need <= workspace_bytes) {
                d.ksplit = ksplit; d.grid = d.total * ksplit; d.lds_bytes = 2 * stage;
                return d;
            }
        }
    }
    d.pair = !ragged && sw.pair && 4 * stage <= 80 * 1024 && nt >= 16;      // long key sequences only: +2 % at 4096 keys, a loss at 256
    d.dma = d.pair && head_dim == 64 && sw.dma && (nt & 3) == 0;            // K / V^T tiles by LDS-DMA into four static stages (64 KiB)
    d.lds_bytes = d.dma ? 0u : (d.pair ? 4u : 2u) * stage;
    return d;
}
