// gswm_viterbi_plan.h -- viterbi_decide: the sizes of the convolutional code, the interleaver, the launch policy and every refusal of gsw_viterbi_decode
// (gswm_viterbi.inc) as ONE pure function.  Host code only, plain C++17, integer arithmetic; the entry point fills the kernel's arguments from the plan and
// tests/viterbi_plan_cases.cpp sweeps it.
//
// The code.  M message bits, a multiple of 16 in 64 .. 8192; T = M / 2 trellis steps of the rate-1/2, constraint-length-7 code
// (generators 0o171, 0o133), of which the last 6 are the zero tail: I = T - 6 info bits in M / 16 bytes, the last byte holding the 2 pad bits and the tail.
// The info word is payload (M / 16 - 3 bytes), CRC-16/CCITT-FALSE (2 bytes), pad.  Code bit i sits at message position (i S) mod M, S the smallest odd
// integer >= (isqrt(M) | 1) coprime to M; Sinv is its inverse mod M: message position p holds code bit (p Sinv) mod M.
//
// One wavefront per image.  A wave's LDS: the de-interleaved scores (4 M bytes), the survivor ballots (8 T = 4 M bytes), the decoded inputs as bytes (T), the
// re-encoded message as bytes (M) and the packed info word (M / 16), rounded up to 16 bytes.  A workgroup holds the largest of {4, 2, 1} waves whose rows fit
// VITERBI_LDS = 96 KiB and that the batch fills (4 waves up to M = 2048, 2 up to 4096, 1 beyond).
//
// Refusals come in the order of the C ABI: BAD_ARG, then UNSUPPORTED; a refusal decides nothing (every other field is zero).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/gswm.h"

constexpr int VITERBI_MIN_M = 64;
constexpr int VITERBI_MAX_M = 8192;
constexpr int VITERBI_TAIL = 6;                                  // constraint length 7
constexpr int VITERBI_MAX_WAVES = 4;
constexpr uint32_t VITERBI_LDS = 96u * 1024u;

// What the entry point knows before it decides.  pointers_ok: score, info, message, metric, flips and ok are present; score, metric, flips and ok are 4-byte aligned.
struct ViterbiQuery {
    bool pointers_ok;
    int B;
    int64_t M, stride;
};

struct ViterbiPlan {
    int status;
    int M, T, I;              // message bits, trellis steps, info bits
    int info_bytes;           // M / 16
    int payload_bytes;        // M / 16 - 3
    int S, Sinv;              // the interleaver's step and its inverse mod M
    int waves, wg, grid;
    uint32_t wave_lds, lds;
};

inline int viterbi_gcd(int a, int b) {
    while (b) { const int t = a % b; a = b; b = t; }
    return a;
}

// the smallest odd integer >= (isqrt(M) | 1) that is coprime to M
inline int viterbi_step(int M) {
    int r = 0;
    while ((int64_t)(r + 1) * (r + 1) <= M) ++r;
    int S = r | 1;
    while (viterbi_gcd(S, M) != 1) S += 2;
    return S;
}

inline uint32_t viterbi_wave_lds(int M) {
    const uint32_t raw = 4u * M + 4u * M + (uint32_t)M / 2u + (uint32_t)M + (uint32_t)M / 16u;
    return (raw + 15u) & ~15u;
}

inline ViterbiPlan viterbi_decide(const ViterbiQuery& q) {
    auto refuse = [](int status) { ViterbiPlan r{}; r.status = status; return r; };
    // ---- BAD_ARG
    if (!q.pointers_ok || q.B < 1 || q.M < VITERBI_MIN_M || q.M % 16 || q.stride < q.M) return refuse(GSW_ERR_BAD_ARG);
    // ---- UNSUPPORTED
    if (q.M > VITERBI_MAX_M) return refuse(GSW_ERR_UNSUPPORTED);

    ViterbiPlan p{};
    p.M = (int)q.M;
    p.T = p.M / 2;
    p.I = p.T - VITERBI_TAIL;
    p.info_bytes = p.M / 16;
    p.payload_bytes = p.info_bytes - 3;
    p.S = viterbi_step(p.M);
    for (p.Sinv = 1; (int64_t)p.Sinv * p.S % p.M != 1; p.Sinv += 2) {}      // S is odd and coprime to M: an odd inverse below M exists
    p.wave_lds = viterbi_wave_lds(p.M);
    p.waves = VITERBI_MAX_WAVES;
    while (p.waves > 1 && ((uint32_t)p.waves * p.wave_lds > VITERBI_LDS || p.waves / 2 >= q.B)) p.waves >>= 1;
    p.wg = 64 * p.waves;
    p.grid = (int)(((int64_t)q.B + p.waves - 1) / p.waves);
    p.lds = (uint32_t)p.waves * p.wave_lds;
    return p;
}
