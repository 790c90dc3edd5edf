// gswm_tamper_soft.inc -- the robust decode in one launch, tile weights times reliability levels (DESIGN.md section 4.24).  Included at the end of
// gswm_tamper.hip, whose stage_row, TamperArgs and TM_WG it uses.
//
//   p_j    = q_j ^ ks_j                                           the decrypted bit (stage_row<false>)
//   lev_j  = sum_k 2^k plane_k[j]                                 the reliability level of cipher bit j, 1 everywhere when there are no planes
//   L_j    = 1 in round r < sign_rounds, else lev_j
//   round r = 0 .. iters:
//     score[t]    = sum over j = t (mod M) of L_j wgt[tile(j / l)] (2 p_j - 1),  wsum[t] the same sum without the sign,  bit_t = score[t] > 0
//     excess[tau] = sum over j in tau of L_j (1 - 2 (p_j ^ bit_{j mod M}))
//     wsq[tau]    = sum over j in tau of L_j^2
//     wgt[tau]   <- max(0, excess[tau] - isqrt(wsq[tau]))         wgt = 1 in round 0
//
// One workgroup per image.  The decrypted row, the planes, the int32 tile weights and the decoded message bytes stay in LDS from the first
// round to the last; only the last round stores to global memory, and it stores every element of every output.
//
// Vote: gsw_vote_tiled_kernel's walk -- S adjacent lanes own message bit t and its copies -- with the level gathered from the planes (the
// bit position inside a byte is the same for every copy of t, msg_bits being whole bytes) and the weight read from LDS.  A lane's copies are
// S M bits apart, a whole number of elements: an element's lattice row and column are divided out once, for the first copy and for the stride,
// and then move by carries.  The byte of decoded bits goes to LDS from the wave's ballot.
// Map: gsw_tile_agree_kernel's ownership -- eight adjacent lanes per tile, lane g on the row segments g, g + 8, .. -- in the popcount form
// of the keyed soft search: with d = p ^ message,  excess = wtot - 2 sum_k 2^k popc(plane_k & d),  wtot = sum_k 2^k popc(plane_k); a round
// at unit levels has excess = n_t - 2 popc(d) and wsq = n_t.  wtot and wsq do not change between rounds: one pass before the first round
// leaves them in LDS (wsq = sum_k 4^k popc(plane_k) + sum_{k < m} 2^(k + m + 1) popc(plane_k & plane_m)).
//
// Control flow around the barriers and the shuffles is workgroup-uniform (trip counts depend on the arguments alone), there are no atomics,
// and each output is a sum of a fixed set of integers formed by one owner: the result does not depend on the launch geometry.
// gswm_robust_plan.h decides the launch: the LDS layout, the lanes per message bit, the int32 and LDS refusals.
//
// Kernel
//   gsw_decode_robust_kernel : [B] workgroups of 256
#include "gswm_robust_plan.h"

namespace {

static_assert(RB_WG == TM_WG, "the robust decode stages its row with stage_row");

struct RobustArgs {
    TamperArgs t;             // packed, keys, the lattice, msg_bits / msg_bytes / copies / log2s; bits, score, wsum of the LAST round
    const uint8_t* planes;    // [B, P, rowbytes]
    int32_t* excess;          // [B, tiles]
    int32_t* wsq;             // [B, tiles]
    int32_t* weights;         // [B, tiles]
    int P, iters, sign_rounds;
    int n_t;
    int level_rounds;
    uint32_t planes_off, wgt_off, wtot_off, wsq_off, msg_off;
};

template <bool WORD>
__device__ __forceinline__ uint32_t lds_unit(const uint8_t* base, uint32_t off) {
    if constexpr (WORD) return *(const uint32_t*)(base + off);
    else return (uint32_t)base[off];
}

// byte offset in the row of segment s of tile (ty, tx): the T l bits the tile owns of lattice row y = ty T + s % T of channel s / T
__device__ __forceinline__ uint32_t segment_offset(const TamperArgs& a, int ty, int tx, int s) {
    const int T = 1 << a.log2t;
    const int c = s >> a.log2t, y = (ty << a.log2t) + (s & (T - 1));
    return (uint32_t)(((((c * a.h + y) * a.w) + (tx << a.log2t)) << a.log2l) >> 3);           // < rowbytes <= 128 Ki
}

// wtot[tau] and wsq[tau] of the levels, once for all rounds.  WORD: a segment is whole dwords.
template <bool WORD>
__device__ __forceinline__ void level_sums(const RobustArgs& r, const uint8_t* pl, int32_t* wtot, int32_t* wsq) {
    const TamperArgs& a = r.t;
    const int tid = threadIdx.x, g = tid & (TM_TILE_LANES - 1);
    const int seg_bytes = ((1 << a.log2t) << a.log2l) >> 3, segs = a.C << a.log2t;
    constexpr uint32_t U = WORD ? 4u : 1u;
    for (int tile0 = 0; tile0 < a.tiles; tile0 += TM_WG / TM_TILE_LANES) {            // the same trip count for every lane: the shuffles run with all lanes on
        const int tile = tile0 + tid / TM_TILE_LANES;
        int tot = 0, sq = 0;
        if (tile < a.tiles) {
            const int ty = tile / a.tw, tx = tile - ty * a.tw;
            for (int s = g; s < segs; s += TM_TILE_LANES) {
                const uint32_t off = segment_offset(a, ty, tx, s);
                for (uint32_t i = 0; i < (uint32_t)seg_bytes; i += U) {
                    uint32_t v[RB_MAX_PLANES];
#pragma unroll
                    for (int k = 0; k < RB_MAX_PLANES; ++k) v[k] = k < r.P ? lds_unit<WORD>(pl + (uint32_t)k * (uint32_t)a.rowbytes, off + i) : 0u;
#pragma unroll
                    for (int k = 0; k < RB_MAX_PLANES; ++k) {
                        const int n = __popc(v[k]);
                        tot += n << k;
                        sq += n << (2 * k);
#pragma unroll
                        for (int m = k + 1; m < RB_MAX_PLANES; ++m) sq += __popc(v[k] & v[m]) << (k + m + 1);
                    }
                }
            }
        }
        tot += __shfl_xor(tot, 1); sq += __shfl_xor(sq, 1);
        tot += __shfl_xor(tot, 2); sq += __shfl_xor(sq, 2);
        tot += __shfl_xor(tot, 4); sq += __shfl_xor(sq, 4);
        if (g == 0 && tile < a.tiles) {
            wtot[tile] = tot;
            wsq[tile] = sq;
        }
    }
}

// The map of one round against the message in LDS, and what follows from it: the next weights (in LDS), or the three tile outputs of the
// last round.  UNIT: the round votes at unit levels.  WORD: a segment and the message are whole dwords.
template <bool UNIT, bool WORD>
__device__ __forceinline__ void map_round(const RobustArgs& r, int b, bool last, const uint8_t* row, const uint8_t* pl, const uint8_t* msg, int32_t* wgt,
                                          const int32_t* wtot, const int32_t* wsq) {
    const TamperArgs& a = r.t;
    const int tid = threadIdx.x, g = tid & (TM_TILE_LANES - 1);
    const int seg_bytes = ((1 << a.log2t) << a.log2l) >> 3, segs = a.C << a.log2t;
    const uint32_t mb = (uint32_t)a.msg_bytes;
    constexpr uint32_t U = WORD ? 4u : 1u;
    for (int tile0 = 0; tile0 < a.tiles; tile0 += TM_WG / TM_TILE_LANES) {            // uniform trip count, as above
        const int tile = tile0 + tid / TM_TILE_LANES;
        int diff = 0;                                                                  // sum over the tile's bits with d_j = 1 of L_j
        if (tile < a.tiles) {
            const int ty = tile / a.tw, tx = tile - ty * a.tw;
            for (int s = g; s < segs; s += TM_TILE_LANES) {
                const uint32_t off = segment_offset(a, ty, tx, s);
                uint32_t mo = off % mb;                                                // WORD: off and mb are multiples of 4, and so is mo
                for (uint32_t i = 0; i < (uint32_t)seg_bytes; i += U) {
                    const uint32_t d = lds_unit<WORD>(row, off + i) ^ lds_unit<WORD>(msg, mo);
                    mo = mo + U == mb ? 0u : mo + U;
                    if constexpr (UNIT) {
                        diff += __popc(d);
                    } else {
#pragma unroll
                        for (int k = 0; k < RB_MAX_PLANES; ++k)
                            if (k < r.P) diff += __popc(lds_unit<WORD>(pl + (uint32_t)k * (uint32_t)a.rowbytes, off + i) & d) << k;
                    }
                }
            }
        }
        diff += __shfl_xor(diff, 1);
        diff += __shfl_xor(diff, 2);
        diff += __shfl_xor(diff, 4);
        if (g == 0 && tile < a.tiles) {
            const int tot = UNIT ? r.n_t : wtot[tile], sq = UNIT ? r.n_t : wsq[tile];
            const int ex = tot - 2 * diff;
            if (last) {
                const int64_t o = (int64_t)b * a.tiles + tile;
                r.excess[o] = ex;
                r.wsq[o] = sq;
                r.weights[o] = wgt[tile];                                              // what the last vote used
            } else {
                const int nw = ex - (int)robust_isqrt((uint32_t)sq);
                wgt[tile] = nw > 0 ? nw : 0;
            }
        }
    }
}

// The vote of one round: score, wsum and the bits of every message bit; the message bytes to LDS, and in the last round all three to global memory.
template <bool UNIT>
__device__ __forceinline__ void vote_round(const RobustArgs& r, int b, bool last, const uint8_t* row, const uint8_t* pl, uint8_t* msg, const int32_t* wgt) {
    const TamperArgs& a = r.t;
    const int tid = threadIdx.x, lane = tid & 63;
    const int S = 1 << a.log2s, s = tid & (S - 1);
    const uint32_t M = (uint32_t)a.msg_bits, w = (uint32_t)a.w, h = (uint32_t)a.h;
    const int per_pass = TM_WG >> a.log2s;             // message bits per pass of the workgroup, a multiple of 8 per wave
    for (int t0 = 0; t0 < a.msg_bits; t0 += per_pass) {
        const int t = t0 + (tid >> a.log2s);
        int sc = 0, ws = 0;
        if (t < a.msg_bits) {
            const uint32_t sh = 7u - ((uint32_t)t & 7u);                               // msg_bits % 8 == 0: every copy of t sits at this bit of its byte
            // copy k of t is bit j = k M + t < Nb <= 2^20, element e = j / l, lattice row q = e / w, x = e % w, y = q % h.  The lane's copies are S M bits apart,
            // a whole number of elements: the two divisions are paid once for the first copy and once for the stride, then (x, y) move by carries
            const uint32_t stride = (uint32_t)S * M, de = stride >> a.log2l, dq = de / w, dx = de - dq * w, dy = dq % h;
            const uint32_t j0 = (uint32_t)s * M + (uint32_t)t, e0 = j0 >> a.log2l, q0 = e0 / w;
            uint32_t x = e0 - q0 * w, y = q0 % h, idx = j0 >> 3;
            for (int k = s; k < a.copies; k += S) {
                const int p = (row[idx] >> sh) & 1;
                int wv = wgt[(y >> a.log2t) * (uint32_t)a.tw + (x >> a.log2t)];
                if constexpr (!UNIT) {
                    int lev = 0;
#pragma unroll
                    for (int i = 0; i < RB_MAX_PLANES; ++i)
                        if (i < r.P) lev |= ((pl[(uint32_t)i * (uint32_t)a.rowbytes + idx] >> sh) & 1) << i;
                    wv *= lev;
                }
                sc += p ? wv : -wv;
                ws += wv;
                idx += stride >> 3;
                x += dx;                                                               // x, dx < w: one carry at most
                const uint32_t carry = x >= w ? 1u : 0u;
                x -= carry ? w : 0u;
                y += dy + carry;                                                       // y, dy < h: y + dy + carry < 2 h
                y -= y >= h ? h : 0u;
            }
        }
        for (int step = 1; step < S; step <<= 1) {
            sc += __shfl_xor(sc, step);
            ws += __shfl_xor(ws, step);
        }
        const bool one = t < a.msg_bits && sc > 0;
        const uint64_t ball = __ballot(one);           // bit (i S) of the wave's ballot: message bit (t of lane 0) + i
        if (t < a.msg_bits && s == 0) {
            const bool head = (t & 7) == 0;            // the seven bits after t are this wave's as well
            const uint8_t byte = head ? (uint8_t)ballot_byte(ball, (uint32_t)lane, (uint32_t)a.log2s) : (uint8_t)0;
            if (head) msg[t >> 3] = byte;
            if (last) {
                a.score[(int64_t)b * a.msg_bits + t] = sc;
                a.wsum[(int64_t)b * a.msg_bits + t] = ws;
                if (head) a.bits[(int64_t)b * a.msg_bytes + (t >> 3)] = byte;
            }
        }
    }
}

__global__ __launch_bounds__(TM_WG) void gsw_decode_robust_kernel(RobustArgs r) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const TamperArgs& a = r.t;
    const int b = blockIdx.x, tid = threadIdx.x;
    uint8_t* pl = lds_raw + r.planes_off;
    int32_t* wgt = (int32_t*)(lds_raw + r.wgt_off);
    int32_t* wtot = (int32_t*)(lds_raw + r.wtot_off);
    int32_t* wsq = (int32_t*)(lds_raw + r.wsq_off);
    uint8_t* msg = lds_raw + r.msg_off;

    stage_row<false>(a, b, (uint32_t*)lds_raw);        // p = q ^ ks
    const int pwords = r.P * (a.rowbytes >> 2);        // rowbytes is a multiple of 8: the planes of an image are whole, 4-byte aligned dwords
    const uint32_t* src = (const uint32_t*)(r.planes + (int64_t)b * r.P * a.rowbytes);
    for (int i = tid; i < pwords; i += TM_WG) ((uint32_t*)pl)[i] = src[i];
    for (int i = tid; i < a.tiles; i += TM_WG) wgt[i] = 1;
    __syncthreads();

    const int seg_bytes = ((1 << a.log2t) << a.log2l) >> 3;                           // 1, 2, 4, 8 or 16, a segment aligned to its own size
    const bool seg_words = seg_bytes >= 4, map_words = seg_words && (a.msg_bytes & 3) == 0;
    if (r.level_rounds) {                              // (its results are first read after the barrier that ends the first vote)
        if (seg_words) level_sums<true>(r, pl, wtot, wsq);
        else level_sums<false>(r, pl, wtot, wsq);
    }
    for (int round = 0; round <= r.iters; ++round) {
        const bool last = round == r.iters, unit = r.P == 0 || round < r.sign_rounds;
        if (unit) vote_round<true>(r, b, last, lds_raw, pl, msg, wgt);
        else vote_round<false>(r, b, last, lds_raw, pl, msg, wgt);
        __syncthreads();
        if (unit) {
            if (map_words) map_round<true, true>(r, b, last, lds_raw, pl, msg, wgt, wtot, wsq);
            else map_round<true, false>(r, b, last, lds_raw, pl, msg, wgt, wtot, wsq);
        } else {
            if (map_words) map_round<false, true>(r, b, last, lds_raw, pl, msg, wgt, wtot, wsq);
            else map_round<false, false>(r, b, last, lds_raw, pl, msg, wgt, wtot, wsq);
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int gsw_decode_robust(const uint8_t* signs_dev, const uint8_t* planes_dev, int P, int B, int C, int h, int w, int l, int tile, const uint8_t* keys_dev,
                                 int msg_bits, int iters, int sign_rounds, uint8_t* bits_dev, int32_t* score_dev, int32_t* wsum_dev, int32_t* excess_dev,
                                 int32_t* wsq_dev, int32_t* weights_dev, void* stream) {
    RobustQuery q{};
    q.P = P; q.B = B; q.C = C; q.h = h; q.w = w; q.l = l; q.tile = tile; q.msg_bits = msg_bits; q.iters = iters; q.sign_rounds = sign_rounds;
    q.signs_aligned = ((uintptr_t)signs_dev & 3) == 0;
    q.planes_aligned = ((uintptr_t)planes_dev & 3) == 0;
    q.keys_aligned = ((uintptr_t)keys_dev & 3) == 0;
    q.signs_null = !signs_dev;
    q.planes_null = !planes_dev;
    q.keys_null = !keys_dev;
    q.outputs_null = !bits_dev || !score_dev || !wsum_dev || !excess_dev || !wsq_dev || !weights_dev;
    const RobustPlan p = robust_decide(q);
    if (p.status != GSW_OK) return p.status;
    RobustArgs r{};
    r.t.packed = signs_dev;
    r.t.keys = keys_dev;
    r.t.bits = bits_dev;
    r.t.score = score_dev;
    r.t.wsum = wsum_dev;
    r.t.C = C; r.t.h = h; r.t.w = w;
    r.t.log2l = p.log2l;
    r.t.log2t = p.log2t;
    r.t.tw = p.tw;
    r.t.tiles = p.tiles;
    r.t.rowbytes = p.rowbytes;
    r.t.nblk = p.nblk;
    r.t.msg_bits = msg_bits;
    r.t.msg_bytes = p.msg_bytes;
    r.t.copies = p.copies;
    r.t.log2s = p.log2s;
    r.planes = planes_dev;
    r.excess = excess_dev;
    r.wsq = wsq_dev;
    r.weights = weights_dev;
    r.P = P; r.iters = iters; r.sign_rounds = sign_rounds;
    r.n_t = p.n_t;
    r.level_rounds = p.level_rounds;
    r.planes_off = p.planes_off; r.wgt_off = p.wgt_off; r.wtot_off = p.wtot_off; r.wsq_off = p.wsq_off; r.msg_off = p.msg_off;
    GSW_HIP(allow_dynamic_lds((const void*)gsw_decode_robust_kernel, p.lds));
    hipLaunchKernelGGL(gsw_decode_robust_kernel, dim3(p.grid), dim3(p.wg), p.lds, (hipStream_t)stream, r);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}
