// gswm_viterbi_list_plan.h -- viterbi_list_decide: the sizes, the LDS slice of a wave, the launch policy and every refusal of gsw_viterbi_list_decode
// (gswm_viterbi_list.inc) as ONE pure function.  Host code only, plain C++17, integer arithmetic; the entry point fills the kernel's arguments from the plan
// and tests/viterbi_list_plan_cases.cpp sweeps it.  Included after gswm_viterbi_plan.h, whose code sizes and interleaver it reuses unchanged.
//
// The code is section 4.29's: M message bits, T = M / 2 steps, I = T - 6 info bits, M / 16 info bytes, the interleaver's S and Sinv.  New is the
// list size L in {1, 2, 4, 8} (section 4.30): every trellis state keeps its L best paths.
//
// One wavefront per image.  A wave's LDS slice, in this order:
//   x     4 M          the de-interleaved scores, int32
//   ex    256 L        the exchange buffer: the wave's 64 L metrics, written once per step and read back as two runs of L (both predecessors are adjacent)
//   dec   4 M L        the survivor records: L bits per state per step (8 L bytes a step, T steps), bit s L + k = the d of output rank k of state s
//   ub    M L / 2      the decoded inputs of the L traced ranks, a byte per step
//   cw    M            the re-encoded message, a byte per bit
//   ib    M / 16       the packed info word of the selected rank
// rounded up to 16 bytes:  wave_lds(M, L) = M (5 + 1/16 + 9 L / 2) + 256 L.
//
// The bound.  A launch is served whenever ONE wave's slice fits the LDS of a compute unit, VITERBI_LIST_LDS = 160 KiB = 163 840 bytes: a workgroup may declare
// all of it on this part, and the kernel has no static LDS.  The project's other kernels stop at 128 KiB because they want two workgroups resident; here a
// refusal is worse than a lone wave on a CU (the survivor records are the decode, there is no smaller form of it without a global workspace), so the limit is
// the hardware's.  That gives M <= 17 104 at L = 1, 11 600 at L = 2, 7 056 at L = 4 and 3 936 at L = 8; every multiple of 16 in 64 .. 2048 is served at every L.
// Beyond it: GSW_ERR_UNSUPPORTED.
//
// A workgroup holds the largest of {4, 2, 1} waves that the batch fills and whose slices together stay within HALF the LDS (80 KiB), so that two such
// workgroups are resident; one wave alone may take up to all of it.
//
// Refusals come in the order of the C ABI: BAD_ARG, then UNSUPPORTED; a refusal decides nothing (every other field is zero).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/gswm.h"
#include "gswm_viterbi_plan.h"

constexpr uint32_t VITERBI_LIST_LDS = 160u * 1024u;              // one wave's slice: the LDS of a CU
constexpr uint32_t VITERBI_LIST_WG_LDS = 80u * 1024u;            // workgroups of 2 and 4 waves: half of it
constexpr int VITERBI_LIST_MAX_L = 8;

// What the entry point knows before it decides.  pointers_ok: the eight pointers are present; score, metric, flips, ok, rank and n_ok are 4-byte aligned.
struct ViterbiListQuery {
    bool pointers_ok;
    int B, L;
    int64_t M, stride;
};

struct ViterbiListPlan {
    int status;
    int M, T, I;              // message bits, trellis steps, info bits
    int info_bytes;           // M / 16
    int payload_bytes;        // M / 16 - 3
    int S, Sinv;              // the interleaver's step and its inverse mod M
    int L;                    // list size
    int full_from;            // 6 + log2 L: from this step to the tail every state's list is full
    int waves, wg, grid;
    uint32_t wave_lds, lds;
};

inline bool viterbi_list_size_ok(int L) { return L == 1 || L == 2 || L == 4 || L == 8; }

// bytes of one wave's slice; 64-bit, so that no M of the ABI's int overflows it
inline uint64_t viterbi_list_wave_lds(int64_t M, int L) {
    const uint64_t m = (uint64_t)M, l = (uint64_t)L;
    const uint64_t raw = 4u * m + 256u * l + 4u * m * l + m * l / 2u + m + m / 16u;
    return (raw + 15u) & ~(uint64_t)15u;
}

inline ViterbiListPlan viterbi_list_decide(const ViterbiListQuery& q) {
    auto refuse = [](int status) { ViterbiListPlan r{}; r.status = status; return r; };
    // ---- BAD_ARG: what viterbi_decide refuses, and the list size
    if (!q.pointers_ok || q.B < 1 || q.M < VITERBI_MIN_M || q.M % 16 || q.stride < q.M || !viterbi_list_size_ok(q.L)) return refuse(GSW_ERR_BAD_ARG);
    // ---- UNSUPPORTED: one wave's slice does not fit the LDS of a CU
    if (q.M > (int64_t)VITERBI_LIST_LDS || viterbi_list_wave_lds(q.M, q.L) > VITERBI_LIST_LDS) return refuse(GSW_ERR_UNSUPPORTED);

    ViterbiListPlan p{};
    p.M = (int)q.M;
    p.T = p.M / 2;
    p.I = p.T - VITERBI_TAIL;
    p.info_bytes = p.M / 16;
    p.payload_bytes = p.info_bytes - 3;
    p.S = viterbi_step(p.M);
    for (p.Sinv = 1; (int64_t)p.Sinv * p.S % p.M != 1; p.Sinv += 2) {}      // S is odd and coprime to M: an odd inverse below M exists
    p.L = q.L;
    p.full_from = VITERBI_TAIL + (q.L == 1 ? 0 : q.L == 2 ? 1 : q.L == 4 ? 2 : 3);
    p.wave_lds = (uint32_t)viterbi_list_wave_lds(p.M, p.L);
    p.waves = VITERBI_MAX_WAVES;
    while (p.waves > 1 && ((uint32_t)p.waves * p.wave_lds > VITERBI_LIST_WG_LDS || p.waves / 2 >= q.B)) p.waves >>= 1;
    p.wg = 64 * p.waves;
    p.grid = (int)(((int64_t)q.B + p.waves - 1) / p.waves);
    p.lds = (uint32_t)p.waves * p.wave_lds;
    return p;
}
