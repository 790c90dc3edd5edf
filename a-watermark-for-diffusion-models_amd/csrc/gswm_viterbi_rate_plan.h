// gswm_viterbi_rate_plan.h -- viterbi_rate_decide: the sizes of the punctured convolutional codes, the interleaver, the LDS slice of a wave, the launch
// policy and every refusal of gsw_viterbi_decode_rate (gswm_viterbi.inc) and gsw_viterbi_list_decode_rate (gswm_viterbi_list.inc) as ONE pure function.
// Host code only, plain C++17, integer arithmetic; the entry points fill the kernels' arguments from the plan and tests/viterbi_rate_plan_cases.cpp sweeps
// it.  Included after gswm_viterbi_plan.h and gswm_viterbi_list_plan.h, which stay as they are: at rate 0 this plan equals theirs field for field.
//
// The codes.  The mother code is section 4.29's: rate 1/2, constraint length 7, generators 0o171 (c0) and 0o133 (c1).  A rate in
// {0, 1, 2} = {1/2, 2/3, 3/4} ("conv", "conv23", "conv34") punctures it with a pattern of period P = rate + 1; step t of phase t mod P keeps
//   phase 0: c0 c1      phase 1: c1      phase 2: c0                                                  (the DVB / 802.11 patterns of this generator pair)
// in this order -- which outputs a phase keeps does not depend on the rate, only how many phases there are.  N(t), the kept bits of the first t steps, is
// V (t div P) + (0, 2, 3)[t mod P] with V = rate + 2 kept bits per period.  M message bits, a multiple of 16 from 64 up; T is the largest multiple of 8 with
// N(T) <= M; I = T - 6 info bits in T / 8 bytes: payload (T / 8 - 3 bytes), CRC-16, 2 pad bits, the tail.  Kept bit j sits at message position (j S) mod M
// for j < N = N(T), S and Sinv as in section 4.29; the M - N spare positions carry 0 and are never read.
//
// One wavefront per image.  A wave's LDS slice, rounded up to 16 bytes:
//   plain read   4 M (the N staged votes) + 8 T (a survivor ballot per step) + T (decoded inputs) + M (the message, a byte per bit) + T / 8 (info word);
//                a workgroup holds the largest of {4, 2, 1} waves whose slices fit VITERBI_LDS = 96 KiB and that the batch fills; M <= 8192 is served
//                at every rate (the largest slice: 97 024 bytes at rate 2, M = 8192), beyond it GSW_ERR_UNSUPPORTED
//   list read    4 M + 256 L (the exchange buffer) + 8 T L (L survivor bits per state and step) + T L (decoded inputs of L ranks) + M + T / 8;
//                served while ONE wave's slice fits VITERBI_LIST_LDS = 160 KiB; workgroups of 2 and 4 waves stay within VITERBI_LIST_WG_LDS = 80 KiB
//
// Refusals come in the order of the C ABI: BAD_ARG (what the two older plans refuse, and a rate outside {0, 1, 2}), then UNSUPPORTED; a refusal decides
// nothing (every other field is zero).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/gswm.h"
#include "gswm_viterbi_plan.h"
#include "gswm_viterbi_list_plan.h"

constexpr int VITERBI_RATES = 3;

constexpr bool viterbi_rate_ok(int rate) { return rate >= 0 && rate < VITERBI_RATES; }
constexpr int viterbi_rate_period(int rate) { return rate + 1; }                  // P: steps per period
constexpr int viterbi_rate_votes(int rate) { return rate + 2; }                   // V: kept bits per period
// which outputs a phase keeps: bit 0 = c0 (0o171), bit 1 = c1 (0o133), c0 before c1
constexpr int viterbi_rate_kept(int phase) { return phase == 0 ? 3 : phase == 1 ? 2 : 1; }
// the kept bits of the phases before `phase` within one period
constexpr int viterbi_rate_phase_offset(int phase) { return phase == 0 ? 0 : phase == 1 ? 2 : 3; }
// N(t): the kept bits of the first t steps
constexpr int64_t viterbi_rate_kept_bits(int rate, int64_t t) {
    return viterbi_rate_votes(rate) * (t / viterbi_rate_period(rate)) + viterbi_rate_phase_offset((int)(t % viterbi_rate_period(rate)));
}
// T: the largest multiple of 8 with N(T) <= M (M >= 64, so T >= 32).  N(T) >= T V / P - 1, so the answer lies at most one step of 8 below the first guess.
constexpr int64_t viterbi_rate_steps(int rate, int64_t M) {
    int64_t T = (M * viterbi_rate_period(rate) / viterbi_rate_votes(rate) + 8) / 8 * 8;
    while (viterbi_rate_kept_bits(rate, T) > M) T -= 8;
    return T;
}

// What an entry point knows before it decides.  list: gsw_viterbi_list_decode_rate asks, L is its list size and pointers_ok covers its eight pointers; else
// gsw_viterbi_decode_rate asks, L is not read and pointers_ok covers its six.
struct ViterbiRateQuery {
    bool pointers_ok, list;
    int B, L, rate;
    int64_t M, stride;
};

struct ViterbiRatePlan {
    int status;
    int M, T, I, N;           // message bits, trellis steps, info bits, code bits kept (M - N spare positions)
    int info_bytes;           // T / 8
    int payload_bytes;        // T / 8 - 3
    int S, Sinv;              // the interleaver's step and its inverse mod M
    int rate;                 // 0, 1, 2
    int L;                    // list size; 1 for the plain read
    int full_from;            // 6 + log2 L: from this step to the tail every state's list is full
    int waves, wg, grid;
    uint32_t wave_lds, lds;
};

// bytes of one wave's slice, 64-bit so that no M of the ABI's int overflows it
inline uint64_t viterbi_rate_wave_lds(int64_t M, int64_t T, bool list, int L) {
    const uint64_t m = (uint64_t)M, t = (uint64_t)T, l = (uint64_t)L;
    const uint64_t raw = list ? 4u * m + 256u * l + 9u * t * l + m + t / 8u : 4u * m + 8u * t + t + m + t / 8u;
    return (raw + 15u) & ~(uint64_t)15u;
}

inline ViterbiRatePlan viterbi_rate_decide(const ViterbiRateQuery& q) {
    auto refuse = [](int status) { ViterbiRatePlan r{}; r.status = status; return r; };
    // ---- BAD_ARG: what viterbi_decide and viterbi_list_decide refuse, and the rate
    if (!q.pointers_ok || q.B < 1 || q.M < VITERBI_MIN_M || q.M % 16 || q.stride < q.M || (q.list && !viterbi_list_size_ok(q.L)) || !viterbi_rate_ok(q.rate))
        return refuse(GSW_ERR_BAD_ARG);
    // ---- UNSUPPORTED: the plain read beyond 8192 bits, the list read when one wave's slice does not fit the LDS of a CU
    const int L = q.list ? q.L : 1;
    if (q.list ? q.M > (int64_t)VITERBI_LIST_LDS : q.M > VITERBI_MAX_M) return refuse(GSW_ERR_UNSUPPORTED);
    const int64_t T = viterbi_rate_steps(q.rate, q.M);
    const uint64_t slice = viterbi_rate_wave_lds(q.M, T, q.list, L);
    if (q.list && slice > VITERBI_LIST_LDS) return refuse(GSW_ERR_UNSUPPORTED);

    ViterbiRatePlan p{};
    p.M = (int)q.M;
    p.T = (int)T;
    p.I = p.T - VITERBI_TAIL;
    p.N = (int)viterbi_rate_kept_bits(q.rate, T);
    p.info_bytes = p.T / 8;
    p.payload_bytes = p.info_bytes - 3;
    p.S = viterbi_step(p.M);
    for (p.Sinv = 1; (int64_t)p.Sinv * p.S % p.M != 1; p.Sinv += 2) {}      // S is odd and coprime to M: an odd inverse below M exists
    p.rate = q.rate;
    p.L = L;
    p.full_from = VITERBI_TAIL + (L == 1 ? 0 : L == 2 ? 1 : L == 4 ? 2 : 3);
    p.wave_lds = (uint32_t)slice;
    const uint32_t wg_lds = q.list ? VITERBI_LIST_WG_LDS : VITERBI_LDS;
    p.waves = VITERBI_MAX_WAVES;
    while (p.waves > 1 && ((uint32_t)p.waves * p.wave_lds > wg_lds || p.waves / 2 >= q.B)) p.waves >>= 1;
    p.wg = 64 * p.waves;
    p.grid = (int)(((int64_t)q.B + p.waves - 1) / p.waves);
    p.lds = (uint32_t)p.waves * p.wave_lds;
    return p;
}
