// gswm_viterbi_list.inc -- the list read of an error-corrected payload: a parallel list Viterbi decode of the votes score[B, M] that keeps the L best paths of
// every trellis state and returns the best-ranked path through state 0 whose CRC holds (gfx950).  Included at the end of gswm_kernels.hip, after
// gswm_viterbi.inc, whose kernel and entry point it leaves as they are; viterbi_list_decide (gswm_viterbi_list_plan.h) refuses or plans.
//
// Definition (DESIGN.md section 4.30; tests/ecc_list_reference.py restates it twice, and every output equals both bit for bit).  Code, interleaver, info
// word, branch metrics, tail and the int32 bound are gswm_viterbi.inc's.  New: every state s holds a list of at most L (metric, path) entries, best first.
//   before step 0 : state 0 holds one entry of metric 0, every other list is empty
//   step t        : the list of s is the merge of the lists of 2 (s & 31) + d, d in {0, 1}, the d = 0 entries + bm, the d = 1 entries - bm, cut to L.
//                   Higher metric first; on equal metrics a d = 0 entry before a d = 1 entry; entries of one predecessor keep their order.  An empty slot
//                   never precedes a filled one.  In the last 6 steps only states with s >> 5 == 0 hold anything.
//   after T - 1   : state 0 holds L paths.  ok_r: rank r's info word passes the CRC and ends in a zero byte.  rank = the lowest r with ok_r, 0 when there
//                   is none; n_ok = #{ r : ok_r }; info, message, metric, flips, ok describe path `rank` as gsw_viterbi_decode describes its single path.
//
// Kernel.  One wavefront per image, lane = state, the L metrics of a lane sorted in registers; an empty slot is the metric INT32_MIN, which no arithmetic
// ever touches (a filled metric stays above -2^30).  A step fetches the 2 L metrics of the two predecessors -- through the wave's exchange buffer in LDS
// (LDSX: 4 L bytes written, 8 L contiguous bytes read: the predecessors are adjacent lanes) or with 2 L ds_bpermute -- and merges them by L rounds of
// "compare the heads, take one, shift its list": the strict compare IS the tie rule.  The survivor record of a step is the d bit of every output rank, L bits
// per state, packed over neighbouring lanes with quad permutes (L = 2, 4), a byte per lane (L = 8) or one ballot (L = 1).  The predecessor's rank is not
// stored: it is the number of lower output ranks with the same d.  Steps 0 .. 5 + log2 L and the tail run the form that knows empty slots; in between every
// list is full and the step is adds, compares and selects only.  Lanes 0 .. L - 1 then walk one rank each back through the records in parallel (T dependent
// LDS reads per lane), each runs the CRC over its own candidate bit-serially, and a ballot gives rank and n_ok.  The wave re-encodes the selected path, counts
// flips, packs and stores as gswm_viterbi.inc does.  No scratch, no atomics, no workspace; every output element written; the barriers are workgroup barriers
// that every wave reaches the same number of times (a wave past the batch decodes the last image again and stores nothing).
//
// Punctured codes (DESIGN.md section 4.31).  RATE is a compile-time parameter as in gswm_viterbi.inc, with the same three changes and nothing else: the N kept
// votes staged compactly, the mask-free steps run as whole periods (votes and branch metrics first, then the P merges; entered at phase full_from mod P, left at
// phase I mod P), and the re-encode writing a step's kept bits at N(t) and zeros at the spare positions.  RATE = 0 is the code above, instruction for
// instruction.  Exchange, merge, records, traceback and CRC do not know the rate.

namespace viterbi_list {

constexpr int EMPTY = INT32_MIN;

struct ListArgs {
    const int32_t* score;   // [B][stride]
    uint8_t* info;          // [B][info_bytes]
    uint8_t* message;       // [B][M / 8]
    int32_t* metric;        // [B]
    int32_t* flips;         // [B]
    int32_t* ok;            // [B]
    int32_t* rank;          // [B]
    int32_t* n_ok;          // [B]
    int64_t stride;         // elements
    int B, M, T, I, info_bytes, payload_bytes, S, Sinv, full_from;
    uint32_t wave_lds;
    int N;                  // code bits kept (M at rate 1/2, where it is not read)
};

// lane i of a quad reads lane sel[i] of its quad
template <int CTRL>
__device__ __forceinline__ uint32_t quad_perm(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, true);
}

template <int L, bool LDSX, int RATE = 0>
__global__ __launch_bounds__(64 * VITERBI_MAX_WAVES) void gsw_viterbi_list_kernel(ListArgs a) {
    constexpr int P = viterbi_rate_period(RATE), V = viterbi_rate_votes(RATE);
    extern __shared__ __attribute__((aligned(16))) uint8_t vl_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waves = blockDim.x >> 6;
    const int64_t img = (int64_t)blockIdx.x * waves + wave;
    const bool stores = img < a.B;
    const int b = stores ? (int)img : a.B - 1;
    const int M = a.M, T = a.T, I = a.I;

    uint8_t* base = vl_lds + (size_t)wave * a.wave_lds;
    int32_t* x = (int32_t*)base;                                    // [M] de-interleaved scores
    int32_t* ex = (int32_t*)(base + 4 * (size_t)M);                 // [64][L] the exchange buffer
    uint8_t* dec = base + 4 * (size_t)M + 256 * L;                  // [T][8 L] survivor records
    uint8_t* ub = dec + (size_t)T * (8 * L);                        // [L][T] decoded inputs of every rank
    uint8_t* cw = ub + (size_t)L * T;                               // [M] the message, a byte per bit
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
    const bool l0 = viterbi::parity7(r0w & 0171u) != 0u, l1 = viterbi::parity7(r0w & 0133u) != 0u;
    int m[L];
#pragma unroll
    for (int j = 0; j < L; ++j) m[j] = EMPTY;
    if (lane == 0) m[0] = 0;                                         // state 0 alone, one path
    const int2* xx = (const int2*)x;

    // One step.  `general`: lists may hold empty slots (the first 6 + log2 L steps, the tail); `tail`: states with u = 1 end empty.
    auto advance = [&](int t, int bm, auto general, auto tail) {
        int A[L], Bv[L];
        if constexpr (LDSX) {
            // 16-byte accesses where the list allows: a lane's run starts at 4 L lane bytes, the predecessors' at 8 L (lane & 31) bytes
            if constexpr (L >= 4) {
#pragma unroll
                for (int q = 0; q < L / 4; ++q) ((int4*)ex)[lane * (L / 4) + q] = make_int4(m[4 * q], m[4 * q + 1], m[4 * q + 2], m[4 * q + 3]);
            } else if constexpr (L == 2) {
                ((int2*)ex)[lane] = make_int2(m[0], m[1]);
            } else {
                ex[lane] = m[0];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // one wave: the LDS serves its instructions in order; this only pins the compiler
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if constexpr (L >= 4) {
                int both[2 * L];
#pragma unroll
                for (int q = 0; q < L / 2; ++q) {
                    const int4 v = ((const int4*)ex)[p0 * (L / 4) + q];
                    both[4 * q] = v.x; both[4 * q + 1] = v.y; both[4 * q + 2] = v.z; both[4 * q + 3] = v.w;
                }
#pragma unroll
                for (int j = 0; j < L; ++j) { A[j] = both[j]; Bv[j] = both[L + j]; }
            } else if constexpr (L == 2) {
                const int4 v = ((const int4*)ex)[lane & 31];
                A[0] = v.x; A[1] = v.y; Bv[0] = v.z; Bv[1] = v.w;
            } else {
                const int2 v = ((const int2*)ex)[lane & 31];
                A[0] = v.x; Bv[0] = v.y;
            }
        } else {
#pragma unroll
            for (int j = 0; j < L; ++j) { A[j] = __shfl(m[j], p0, 64); Bv[j] = __shfl(m[j], p0 + 1, 64); }
        }
#pragma unroll
        for (int j = 0; j < L; ++j) {
            if constexpr (decltype(general)::value) {
                A[j] = A[j] == EMPTY ? EMPTY : A[j] + bm;
                Bv[j] = Bv[j] == EMPTY ? EMPTY : Bv[j] - bm;
            } else {
                A[j] += bm;
                Bv[j] -= bm;
            }
        }
        uint32_t dm = 0u;                                            // bit k: output rank k came from d = 1
#pragma unroll
        for (int k = 0; k < L; ++k) {
            const bool tb = Bv[0] > A[0];                            // strict: on equal metrics d = 0 goes first; two empty heads give an empty slot
            m[k] = tb ? Bv[0] : A[0];
            dm |= (uint32_t)tb << k;
#pragma unroll
            for (int j = 0; j + k + 1 < L; ++j) {
                A[j] = tb ? A[j] : A[j + 1];
                Bv[j] = tb ? Bv[j + 1] : Bv[j];
            }
        }
        if constexpr (decltype(tail)::value) {
#pragma unroll
            for (int k = 0; k < L; ++k) m[k] = u ? EMPTY : m[k];
        }
        // the record: bit lane L + k of the step's 8 L bytes
        if constexpr (L == 8) {
            dec[(size_t)t * 64 + lane] = (uint8_t)dm;
        } else if constexpr (L == 4) {
            const uint32_t v = dm | (quad_perm<0xF5>(dm) << 4);     // [1, 1, 3, 3]: an even lane reads its right neighbour
            if (!(lane & 1)) dec[(size_t)t * 32 + (lane >> 1)] = (uint8_t)v;
        } else if constexpr (L == 2) {
            uint32_t v = dm | (quad_perm<0xF5>(dm) << 2);
            v |= quad_perm<0xEE>(v) << 4;                            // [2, 3, 2, 3]: lane 0 of a quad reads lane 2
            if (!(lane & 3)) dec[(size_t)t * 16 + (lane >> 2)] = (uint8_t)v;
        } else {
            const unsigned long long ball = __ballot(dm != 0u);
            if (lane == 0) ((unsigned long long*)dec)[t] = ball;
        }
    };
    // the branch metric of a step of phase `ph` whose first kept vote is x[o]
    auto bm_of = [&](int ph, int o) {
        if (ph == 0) return (l0 ? x[o] : -x[o]) + (l1 ? x[o + 1] : -x[o + 1]);
        const int v = x[o];
        return ph == 1 ? (l1 ? v : -v) : (l0 ? v : -v);
    };
    auto step = [&](int t, auto general, auto tail) {
        if constexpr (RATE == 0) {
            const int2 ab = xx[t];
            advance(t, (l0 ? ab.x : -ab.x) + (l1 ? ab.y : -ab.y), general, tail);
        } else {
            const int ph = t % P;
            advance(t, bm_of(ph, V * (t / P) + viterbi_rate_phase_offset(ph)), general, tail);
        }
    };
    const int full_from = a.full_from;
    for (int t = 0; t < full_from; ++t) step(t, std::true_type{}, std::false_type{});
    if constexpr (RATE == 0) {
        for (int t = full_from; t < I; ++t) step(t, std::false_type{}, std::false_type{});
    } else {
        int t = full_from;
        for (; t < I && t % P; ++t) step(t, std::false_type{}, std::false_type{});      // to the first period boundary
        for (int o = V * (t / P); t + P <= I; t += P, o += V) {                          // whole periods: the votes and the metrics first, then the merges
            int bm[P];
#pragma unroll
            for (int ph = 0; ph < P; ++ph) bm[ph] = bm_of(ph, o + viterbi_rate_phase_offset(ph));
#pragma unroll
            for (int ph = 0; ph < P; ++ph) advance(t + ph, bm[ph], std::false_type{}, std::false_type{});
        }
        for (; t < I; ++t) step(t, std::false_type{}, std::false_type{});               // the period the tail cuts
    }
    for (int t = I; t < T; ++t) step(t, std::true_type{}, std::true_type{});
    __syncthreads();

    // ---- traceback from state 0: lane r walks rank r, T dependent reads each, and runs the CRC of its own candidate over its bits
    bool okr = false;
    if (lane < L) {
        uint8_t* mine = ub + (size_t)lane * T;
        int s = 0, k = lane;
        for (int t = T - 1; t >= 0; --t) {
            const int o = s * L;
            const uint32_t rec = ((uint32_t)dec[(size_t)t * (8 * L) + (o >> 3)] >> (o & 7)) & ((1u << L) - 1u);
            const int d = (int)((rec >> k) & 1u);
            const int same1 = __popc(rec & ((1u << k) - 1u));      // lower output ranks that came from d = 1
            mine[t] = (uint8_t)(s >> 5);
            k = d ? same1 : k - same1;
            s = 2 * (s & 31) + d;
        }
        uint32_t crc = 0xFFFFu;
        const int pbits = 8 * a.payload_bytes;
        for (int i = 0; i < pbits; ++i) {
            const uint32_t top = ((crc >> 15) & 1u) ^ (uint32_t)mine[i];
            crc = (crc << 1) & 0xFFFFu;
            if (top) crc ^= 0x1021u;
        }
        uint32_t got = 0u, rest = 0u;
        for (int i = 0; i < 16; ++i) got = (got << 1) | (uint32_t)mine[pbits + i];
        for (int i = pbits + 16; i < T; ++i) rest |= (uint32_t)mine[i];   // the 2 pad bits and the tail: the last info byte
        okr = crc == got && rest == 0u;
    }
    const unsigned long long okm = __ballot(okr);
    const int n_ok = __popcll(okm);
    const int rank = okm ? (int)__builtin_ctzll(okm) : 0;
    int pm = m[0];
#pragma unroll
    for (int j = 1; j < L; ++j) pm = rank == j ? m[j] : pm;         // lane 0 is state 0: its metric of the selected rank
    __syncthreads();

    // ---- re-encode the selected path into message positions, count the disagreements with the hard decisions
    const uint8_t* sel = ub + (size_t)rank * T;
    int nflip = 0;
    for (int t = lane; t < T; t += 64) {
        uint32_t r = 0u;                                             // bit 6 - k = the input k steps back
#pragma unroll
        for (int k = 0; k <= VITERBI_TAIL; ++k)
            if (t - k >= 0) r |= (uint32_t)sel[t - k] << (6 - k);
        const uint32_t c0 = viterbi::parity7(r & 0171u), c1 = viterbi::parity7(r & 0133u);
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
        for (int i = 0; i < 8; ++i) v |= (uint32_t)sel[8 * k + i] << (7 - i);
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
        a.metric[b] = pm;
        a.flips[b] = nflip;
        a.ok[b] = (int)((okm >> rank) & 1ull);
        a.rank[b] = rank;
        a.n_ok[b] = n_ok;
    }
}

// The exchange each list size ships with (tools/ecc_list_bench.py measures both forms; profiles/ecc_list_bench.txt has the figures): through LDS from L = 2 on,
// where it was the faster form at every size measured (by 3 to 19 %); at L = 1 neither form wins everywhere and the two ds_bpermute of gswm_viterbi.inc stay.
template <int L> constexpr bool lds_exchange() { return L >= 2; }

template <int L, int RATE>
static int launch(int grid, int wg, uint32_t lds, const ListArgs& a, hipStream_t stream) {
    const void* k = (const void*)gsw_viterbi_list_kernel<L, lds_exchange<L>(), RATE>;
    GSW_HIP(allow_dynamic_lds(k, lds));
    hipLaunchKernelGGL((gsw_viterbi_list_kernel<L, lds_exchange<L>(), RATE>), dim3((uint32_t)grid), dim3((uint32_t)wg), lds, stream, a);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

template <int RATE>
static int launch_rate(const ViterbiRatePlan& p, const ListArgs& a, hipStream_t stream) {
    switch (p.L) {
        case 1: return launch<1, RATE>(p.grid, p.wg, p.lds, a, stream);
        case 2: return launch<2, RATE>(p.grid, p.wg, p.lds, a, stream);
        case 4: return launch<4, RATE>(p.grid, p.wg, p.lds, a, stream);
        default: return launch<8, RATE>(p.grid, p.wg, p.lds, a, stream);
    }
}

}  // namespace viterbi_list

int gsw_viterbi_list_decode_rate(const int32_t* score_dev, int64_t score_stride, int B, int message_bits, int rate, int list_size, uint8_t* info_dev,
                                 uint8_t* message_dev, int32_t* metric_dev, int32_t* flips_dev, int32_t* ok_dev, int32_t* rank_dev, int32_t* n_ok_dev, void* stream) {
    using namespace viterbi_list;
    using viterbi::aligned4;
    ViterbiRateQuery q{};
    q.pointers_ok = score_dev && info_dev && message_dev && metric_dev && flips_dev && ok_dev && rank_dev && n_ok_dev && aligned4(score_dev) &&
                    aligned4(metric_dev) && aligned4(flips_dev) && aligned4(ok_dev) && aligned4(rank_dev) && aligned4(n_ok_dev);
    q.list = true;
    q.B = B;
    q.L = list_size;
    q.rate = rate;
    q.M = message_bits;
    q.stride = score_stride;
    const ViterbiRatePlan p = viterbi_rate_decide(q);
    if (p.status != GSW_OK) return p.status;
    const ListArgs a{score_dev, info_dev, message_dev, metric_dev, flips_dev, ok_dev, rank_dev, n_ok_dev, score_stride, B, p.M, p.T, p.I, p.info_bytes,
                     p.payload_bytes, p.S, p.Sinv, p.full_from, p.wave_lds, p.N};
    switch (p.rate) {
        case 0: return launch_rate<0>(p, a, (hipStream_t)stream);
        case 1: return launch_rate<1>(p, a, (hipStream_t)stream);
        default: return launch_rate<2>(p, a, (hipStream_t)stream);
    }
}

// rate 1/2: the entry point of section 4.30, its plan and its kernel instantiations
int gsw_viterbi_list_decode(const int32_t* score_dev, int64_t score_stride, int B, int message_bits, int list_size, uint8_t* info_dev, uint8_t* message_dev,
                            int32_t* metric_dev, int32_t* flips_dev, int32_t* ok_dev, int32_t* rank_dev, int32_t* n_ok_dev, void* stream) {
    using namespace viterbi_list;
    using viterbi::aligned4;
    ViterbiListQuery q{};
    q.pointers_ok = score_dev && info_dev && message_dev && metric_dev && flips_dev && ok_dev && rank_dev && n_ok_dev && aligned4(score_dev) &&
                    aligned4(metric_dev) && aligned4(flips_dev) && aligned4(ok_dev) && aligned4(rank_dev) && aligned4(n_ok_dev);
    q.B = B;
    q.L = list_size;
    q.M = message_bits;
    q.stride = score_stride;
    const ViterbiListPlan p = viterbi_list_decide(q);
    if (p.status != GSW_OK) return p.status;
    const ListArgs a{score_dev, info_dev, message_dev, metric_dev, flips_dev, ok_dev, rank_dev, n_ok_dev, score_stride, B, p.M, p.T, p.I, p.info_bytes,
                     p.payload_bytes, p.S, p.Sinv, p.full_from, p.wave_lds, p.M};
    switch (p.L) {
        case 1: return launch<1, 0>(p.grid, p.wg, p.lds, a, (hipStream_t)stream);
        case 2: return launch<2, 0>(p.grid, p.wg, p.lds, a, (hipStream_t)stream);
        case 4: return launch<4, 0>(p.grid, p.wg, p.lds, a, (hipStream_t)stream);
        default: return launch<8, 0>(p.grid, p.wg, p.lds, a, (hipStream_t)stream);
    }
}
