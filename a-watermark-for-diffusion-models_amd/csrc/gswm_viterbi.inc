// gswm_viterbi.inc -- the read of an error-corrected payload: a maximum-correlation Viterbi decode of the votes score[B, M] under the rate-1/2,
// constraint-length-7 convolutional code (generators 0o171, 0o133, zero tail, CRC-16, interleaved), B images in one launch (gfx950).  Included at the end of
// gswm_kernels.hip, after gswm_codec_soft_l.inc; viterbi_decide (gswm_viterbi_plan.h) refuses or plans, the entry point fills the arguments and launches.
//
// Definition (DESIGN.md section 4.29; tests/ecc_reference.py restates it in NumPy, and every output equals that restatement bit for bit).
//   x[i]       = score[(i S) mod M]                       the vote of code bit i (positive: 1); staged through p -> (p Sinv) mod M
//   state s    : the last 6 inputs, the newest at bit 5; input u moves s to (u << 5) | (s >> 1) and emits c0 = parity(r & 0o171), c1 = parity(r & 0o133)
//                with r = (u << 6) | s
//   step t     : state s is reached from 2 (s & 31) + d, d in {0, 1}, with input u = s >> 5; the branch adds (2 c0 - 1) x[2t] + (2 c1 - 1) x[2t + 1].
//                Both generators have bit 0 set, so the d = 1 branch carries the complemented labels: its metric is the negative of d = 0's.
//                Only state 0 is reachable before step 0; an unreachable predecessor never wins; in the last 6 steps only u = 0 exists; on equal
//                metrics d = 0 (the lower state) wins.  int32 path metrics: sum_t |score[t]| < 2^30 is the caller's bound.
//   traceback  : from state 0 after step T - 1.  info = the first I inputs, packed MSB first; message = the re-encoded, re-interleaved codeword;
//                metric = the winning path's correlation; flips = #{ p : message bit p != (score[p] > 0) }; ok = CRC-16/CCITT-FALSE of the payload bytes
//                equals the two bytes after them and the last info byte (2 pad bits, the tail) is zero.
//
// Kernel.  One wavefront per image, lane = state, VITERBI waves per workgroup, each with its own slice of dynamic LDS and no data shared between them; the
// barriers are workgroup barriers that every wave reaches the same number of times (a wave past the batch decodes the last image again and stores nothing).
// The forward pass keeps the path metric of state `lane` in a register, fetches the two predecessors' metrics with two ds_bpermute and holds reachability as
// a wave-uniform 64-bit mask; the survivor decisions of a step are one ballot, written to LDS by lane 0.  Lane 0 then walks the T ballots back (a serial,
// latency-bound walk of T <= 4096 dependent LDS reads), and the wave re-encodes, counts, packs and stores in parallel; lane 0 runs the CRC over at most 509
// bytes.  No scratch, no atomics, no workspace, every output element written.
//
// Punctured codes (DESIGN.md section 4.31; tests/ecc_rate_reference.py).  The kernel takes the rate as a compile-time parameter: RATE = 0 is the code above,
// instruction for instruction; RATE = 1, 2 (rates 2/3, 3/4) puncture it with period P = RATE + 1 (gswm_viterbi_rate_plan.h: phase 0 keeps c0 c1, phase 1 c1,
// phase 2 c0).  A punctured output adds nothing to a branch metric, so the complement property holds as it is.  The N kept votes are staged compactly --
// x[j] = score[(j S) mod M] for j < N, the spare positions are not read -- and step t reads its one or two votes at N(t).  Between the first 6 steps and the
// tail the loop runs whole periods: one wave-uniform LDS read of the period's 3 or 4 votes, the P branch metrics, then the P dependent add-compare-selects, so
// that neither the fetch nor the labels sit on the path-metric chain; the steps before the first period boundary (the loop is entered at phase 6 mod P) and
// after the last (it is left at phase I mod P) take one step at a time.  Re-encoding is lane per step: a step's kept bits go to the positions of N(t), N(t) + 1,
// and the M - N spare positions of the message are written 0.

namespace viterbi {

struct ViterbiArgs {
    const int32_t* score;   // [B][stride]
    uint8_t* info;          // [B][info_bytes]
    uint8_t* message;       // [B][M / 8]
    int32_t* metric;        // [B]
    int32_t* flips;         // [B]
    int32_t* ok;            // [B]
    int64_t stride;         // elements
    int B, M, T, I, info_bytes, payload_bytes, S, Sinv;
    uint32_t wave_lds;
    int N;                  // code bits kept (M at rate 1/2, where it is not read)
};

__device__ __forceinline__ uint32_t parity7(uint32_t v) { return (uint32_t)__popc(v) & 1u; }

template <int RATE>
__global__ __launch_bounds__(64 * VITERBI_MAX_WAVES) void gsw_viterbi_decode_kernel(ViterbiArgs a) {
    constexpr int P = viterbi_rate_period(RATE), V = viterbi_rate_votes(RATE);
    extern __shared__ __attribute__((aligned(16))) uint8_t vit_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves = blockDim.x >> 6;
    const int64_t img = (int64_t)blockIdx.x * waves + wave;
    const bool stores = img < a.B;
    const int b = stores ? (int)img : a.B - 1;
    const int M = a.M, T = a.T, I = a.I;

    uint8_t* base = vit_lds + (size_t)wave * a.wave_lds;
    int32_t* x = (int32_t*)base;                                    // [M] de-interleaved scores, the first N of them staged
    unsigned long long* dec = (unsigned long long*)(base + 4 * (size_t)M);   // [T] survivor ballots
    uint8_t* ub = base + 4 * (size_t)M + 8 * (size_t)T;             // [T] decoded inputs
    uint8_t* cw = ub + T;                                           // [M] the message, a byte per bit
    uint8_t* ib = cw + M;                                           // [info_bytes] the packed info word

    // ---- stage the row through the interleaver: coalesced global reads, the permutation on the LDS side
    const int32_t* row = a.score + (int64_t)b * a.stride;
    if constexpr (RATE == 0) {
        for (int p = lane; p < M; p += 64) x[(uint32_t)(p * a.Sinv) % (uint32_t)M] = row[p];
    } else {
        for (int p = lane; p < M; p += 64) {
            const uint32_t j = (uint32_t)(p * a.Sinv) % (uint32_t)M;
            if (j < (uint32_t)a.N) x[j] = row[p];                    // a spare position holds no code bit: its vote is not read
        }
    }
    __syncthreads();

    // ---- forward pass.  The labels of the d = 0 branch into state `lane` are constants of the lane.
    const int p0 = 2 * (lane & 31), u = lane >> 5;
    const uint32_t r0w = ((uint32_t)u << 6) | (uint32_t)p0;
    const bool l0 = parity7(r0w & 0171u) != 0u, l1 = parity7(r0w & 0133u) != 0u;
    int pm = 0;
    unsigned long long reach = 1ull;                                 // state 0 alone
    const int2* xx = (const int2*)x;
    // One step.  `general`: the form of the definition, for the first 6 steps (states become reachable) and the 6 tail steps (states cease to be).  In between
    // every state is reachable through both predecessors and both inputs exist, so the step is an add, a subtract, a compare and a maximum: the loop is bound
    // by the instructions it issues per step as much as by the latency of the exchange, and this form issues about a dozen fewer.
    auto advance = [&](int t, int bm, auto general) {
        const int m0 = __shfl(pm, p0, 64), m1 = __shfl(pm, p0 + 1, 64);
        const int c0 = m0 + bm, c1 = m1 - bm;
        unsigned long long ball;
        if constexpr (decltype(general)::value) {
            const bool r0 = (reach >> p0) & 1ull, r1 = (reach >> (p0 + 1)) & 1ull;
            const bool d = r1 && (!r0 || c1 > c0);
            const bool live = (r0 || r1) && (t < I || u == 0);
            pm = live ? (d ? c1 : c0) : 0;
            ball = __ballot(d);
            reach = __ballot(live);
        } else {
            const bool d = c1 > c0;
            pm = d ? c1 : c0;
            ball = __ballot(d);
        }
        if (lane == 0) dec[t] = ball;
    };
    // the branch metric of a step of phase `ph` whose first kept vote is x[o]
    auto bm_of = [&](int ph, int o) {
        if (ph == 0) return (l0 ? x[o] : -x[o]) + (l1 ? x[o + 1] : -x[o + 1]);
        const int v = x[o];
        return ph == 1 ? (l1 ? v : -v) : (l0 ? v : -v);
    };
    auto step = [&](int t, auto general) {
        if constexpr (RATE == 0) {
            const int2 ab = xx[t];
            advance(t, (l0 ? ab.x : -ab.x) + (l1 ? ab.y : -ab.y), general);
        } else {
            const int ph = t % P;
            advance(t, bm_of(ph, V * (t / P) + viterbi_rate_phase_offset(ph)), general);
        }
    };
    for (int t = 0; t < VITERBI_TAIL; ++t) step(t, std::true_type{});
    if constexpr (RATE == 0) {
        for (int t = VITERBI_TAIL; t < I; ++t) step(t, std::false_type{});   // (after 6 steps `reach` is all ones and stays so until the tail)
    } else {
        int t = VITERBI_TAIL;
        for (; t < I && t % P; ++t) step(t, std::false_type{});              // to the first period boundary
        for (int o = V * (t / P); t + P <= I; t += P, o += V) {              // whole periods: the votes and the metrics first, then the chain
            int bm[P];
#pragma unroll
            for (int ph = 0; ph < P; ++ph) bm[ph] = bm_of(ph, o + viterbi_rate_phase_offset(ph));
#pragma unroll
            for (int ph = 0; ph < P; ++ph) advance(t + ph, bm[ph], std::false_type{});
        }
        for (; t < I; ++t) step(t, std::false_type{});                       // the period the tail cuts
    }
    for (int t = I; t < T; ++t) step(t, std::true_type{});
    __syncthreads();

    // ---- traceback from state 0: one lane, T dependent reads.  (Measured against a walk that loads 64 ballots per block into registers and fetches each step's
    // with v_readlane: that form was SLOWER, 254 against 207 us at M = 2048, B = 1; DESIGN.md section 4.29 has the figures.)
    if (lane == 0) {
        int s = 0;
        for (int t = T - 1; t >= 0; --t) {
            const unsigned long long w = dec[t];
            ub[t] = (uint8_t)(s >> 5);
            s = 2 * (s & 31) + (int)((w >> s) & 1ull);
        }
    }
    __syncthreads();

    // ---- re-encode into message positions, count the disagreements with the hard decisions
    int nflip = 0;
    for (int t = lane; t < T; t += 64) {
        uint32_t r = 0u;                                             // bit 6 - k = the input k steps back
#pragma unroll
        for (int k = 0; k <= VITERBI_TAIL; ++k)
            if (t - k >= 0) r |= (uint32_t)ub[t - k] << (6 - k);
        const uint32_t c0 = parity7(r & 0171u), c1 = parity7(r & 0133u);
        if constexpr (RATE == 0) {
            const int2 ab = xx[t];
            nflip += (int)(c0 != (uint32_t)(ab.x > 0)) + (int)(c1 != (uint32_t)(ab.y > 0));
            const uint32_t q0 = (uint32_t)(2 * t) * (uint32_t)a.S % (uint32_t)M;
            const uint32_t q1 = (uint32_t)(2 * t + 1) * (uint32_t)a.S % (uint32_t)M;
            cw[q0] = (uint8_t)c0;
            cw[q1] = (uint8_t)c1;
        } else {
            const int ph = t % P, kept = viterbi_rate_kept(ph);
            int j = V * (t / P) + viterbi_rate_phase_offset(ph);    // N(t): the step's first kept bit
            if (kept & 1) {
                nflip += (int)(c0 != (uint32_t)(x[j] > 0));
                cw[(uint32_t)j * (uint32_t)a.S % (uint32_t)M] = (uint8_t)c0;
                ++j;
            }
            if (kept & 2) {
                nflip += (int)(c1 != (uint32_t)(x[j] > 0));
                cw[(uint32_t)j * (uint32_t)a.S % (uint32_t)M] = (uint8_t)c1;
            }
        }
    }
    if constexpr (RATE != 0)
        for (int j = a.N + lane; j < M; j += 64) cw[(uint32_t)j * (uint32_t)a.S % (uint32_t)M] = 0;       // the spare positions
    for (int k = lane; k < a.info_bytes; k += 64) {                 // T = 8 info_bytes: the tail's zeros fill the last byte
        uint32_t v = 0u;
#pragma unroll
        for (int i = 0; i < 8; ++i) v |= (uint32_t)ub[8 * k + i] << (7 - i);
        ib[k] = (uint8_t)v;
        if (stores) a.info[(int64_t)b * a.info_bytes + k] = (uint8_t)v;
    }
    for (int s = 32; s > 0; s >>= 1) nflip += __shfl_xor(nflip, s, 64);
    __syncthreads();

    for (int k = lane; k < M / 8; k += 64) {
        uint32_t v = 0u;
#pragma unroll
        for (int i = 0; i < 8; ++i) v |= (uint32_t)cw[8 * k + i] << (7 - i);
        if (stores) a.message[(int64_t)b * (M / 8) + k] = (uint8_t)v;
    }
    if (lane == 0 && stores) {
        uint32_t crc = 0xFFFFu;
        for (int k = 0; k < a.payload_bytes; ++k) {
            crc ^= (uint32_t)ib[k] << 8;
#pragma unroll
            for (int i = 0; i < 8; ++i) crc = (crc & 0x8000u) ? ((crc << 1) ^ 0x1021u) & 0xFFFFu : (crc << 1) & 0xFFFFu;
        }
        const uint32_t got = ((uint32_t)ib[a.payload_bytes] << 8) | (uint32_t)ib[a.payload_bytes + 1];
        a.metric[b] = pm;                                            // lane 0 is state 0
        a.flips[b] = nflip;
        a.ok[b] = (crc == got && ib[a.payload_bytes + 2] == 0) ? 1 : 0;
    }
}

static bool aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0; }

}  // namespace viterbi

namespace viterbi {

template <int RATE>
static int launch(const ViterbiRatePlan& p, const ViterbiArgs& a, hipStream_t stream) {
    GSW_HIP(allow_dynamic_lds((const void*)gsw_viterbi_decode_kernel<RATE>, p.lds));
    hipLaunchKernelGGL(gsw_viterbi_decode_kernel<RATE>, dim3((uint32_t)p.grid), dim3((uint32_t)p.wg), p.lds, stream, a);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

}  // namespace viterbi

int gsw_viterbi_decode_rate(const int32_t* score_dev, int64_t score_stride, int B, int message_bits, int rate, uint8_t* info_dev, uint8_t* message_dev,
                            int32_t* metric_dev, int32_t* flips_dev, int32_t* ok_dev, void* stream) {
    using namespace viterbi;
    ViterbiRateQuery q{};
    q.pointers_ok = score_dev && info_dev && message_dev && metric_dev && flips_dev && ok_dev && aligned4(score_dev) && aligned4(metric_dev) &&
                    aligned4(flips_dev) && aligned4(ok_dev);
    q.list = false;
    q.B = B;
    q.rate = rate;
    q.M = message_bits;
    q.stride = score_stride;
    const ViterbiRatePlan p = viterbi_rate_decide(q);
    if (p.status != GSW_OK) return p.status;
    const ViterbiArgs a{score_dev, info_dev, message_dev, metric_dev, flips_dev, ok_dev, score_stride, B, p.M, p.T, p.I, p.info_bytes, p.payload_bytes, p.S, p.Sinv,
                        p.wave_lds, p.N};
    switch (p.rate) {
        case 0: return launch<0>(p, a, (hipStream_t)stream);
        case 1: return launch<1>(p, a, (hipStream_t)stream);
        default: return launch<2>(p, a, (hipStream_t)stream);
    }
}

// rate 1/2: the entry point of section 4.29, its plan and its kernel instantiation
int gsw_viterbi_decode(const int32_t* score_dev, int64_t score_stride, int B, int message_bits, uint8_t* info_dev, uint8_t* message_dev, int32_t* metric_dev,
                       int32_t* flips_dev, int32_t* ok_dev, void* stream) {
    using namespace viterbi;
    ViterbiQuery q{};
    q.pointers_ok = score_dev && info_dev && message_dev && metric_dev && flips_dev && ok_dev && aligned4(score_dev) && aligned4(metric_dev) &&
                    aligned4(flips_dev) && aligned4(ok_dev);
    q.B = B;
    q.M = message_bits;
    q.stride = score_stride;
    const ViterbiPlan p = viterbi_decide(q);
    if (p.status != GSW_OK) return p.status;
    const ViterbiArgs a{score_dev, info_dev, message_dev, metric_dev, flips_dev, ok_dev, score_stride, B, p.M, p.T, p.I, p.info_bytes, p.payload_bytes, p.S, p.Sinv,
                        p.wave_lds, p.M};
    GSW_HIP(allow_dynamic_lds((const void*)gsw_viterbi_decode_kernel<0>, p.lds));
    hipLaunchKernelGGL(gsw_viterbi_decode_kernel<0>, dim3((uint32_t)p.grid), dim3((uint32_t)p.wg), p.lds, (hipStream_t)stream, a);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}
