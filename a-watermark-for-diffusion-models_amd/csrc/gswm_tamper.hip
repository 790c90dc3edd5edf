// gswm_tamper.hip -- where an image still agrees with a codeword, a vote that listens to those places, and the robust decode that alternates the two, gfx950.
//
//   q        the image's quantised bits, packed MSB first (gsw_sign_pack / gsw_quant_pack): element i = (c, y, x) of the [C, h, w]
//            lattice owns bits [i l, i l + l)
//   ks       the keystream of the image's own (key, nonce16), initial counter and carry as gsw_keystream
//   cw_j     = ks_j ^ m[j mod M]                                  the cipher bits gsw_embed[_l] plants for message m (its codeword)
//   agree[b, ty, tx] = #{ j in tile (ty, tx) : q_j == cw_j }      tile = the elements of ALL channels with y / T == ty, x / T == tx
//   p_j      = q_j ^ ks_j                                         the decrypted bit
//   score[b, t] = sum_{j = t (mod M)} wgt[tile(j / l)] (2 p_j - 1),   wsum[b, t] = sum_{j = t (mod M)} wgt[tile(j / l)]
//   bit_t    = score > 0                                          (a tie or no weight at all -> 0, the reference's tie rule)
// and the robust decode, with
//   lev_j    = sum_k 2^k plane_k[j]                               the reliability level of cipher bit j, 1 everywhere when there are no planes
//   L_j      = 1 in round r < sign_rounds, else lev_j
//   round r = 0 .. iters:
//     score[t]    = sum over j = t (mod M) of L_j wgt[tile(j / l)] (2 p_j - 1),  wsum[t] the same sum without the sign,  bit_t = score[t] > 0
//     excess[tau] = sum over j in tau of L_j (1 - 2 (p_j ^ bit_{j mod M}))
//     wsq[tau]    = sum over j in tau of L_j^2
//     wgt[tau]   <- max(0, excess[tau] - isqrt(wsq[tau]))         wgt = 1 in round 0
//
// One workgroup per image, every image under its own key.  Every kernel starts the same way (stage_row): the quads of the workgroup compute the
// ChaCha20 blocks of the image's keystream with gswm_chacha.h's chacha20_block and, still in registers, XOR them with
// the packed row (and, for the map, the message): what reaches LDS is the row of differences d = q ^ cw (map) or of decrypted bits p
// (vote, robust decode), in the row's own byte order.  No keystream and no codeword exists in memory.  h and w are multiples of T and T of 8, so a
// row is a whole number of dwords and the T l bits a tile owns of one lattice row are T l / 8 whole bytes, aligned to their own size.
//
// Tile walk (tile_walk).  Eight adjacent lanes own a tile: lane g takes the row segments g, g + 8, .. of its C T segments, adds up what the caller
// counts in each dword (or byte) of them, and the eight partial sums meet in three __shfl_xor steps (distances 1, 2, 4: inside a row of eight lanes,
// DPP moves).  The lane with g == 0 hands the sums to the caller.  Every tile has exactly one owner: no atomics, nothing to zero first.
// Vote walk (vote_walk).  S adjacent lanes (a power of two up to 8, chosen on the host so that small messages still fill the workgroup) own a message
// bit t and walk its copies j = t + k M, k = s, s + S, ..: the bit comes from the LDS row (its position inside a byte is the same for every copy,
// msg_bits being whole bytes), the weight from the element's tile, the level, if any, from the planes.  A lane's copies are S M bits apart, a whole
// number of elements: an element's lattice row and column are divided out once, for the first copy and for the stride, and then move by carries.
// The S partial sums meet by __shfl_xor, and the eight sign bits of a byte of the message are collected from the wave's ballot.
//
// Control flow around the barriers and the shuffles is workgroup-uniform (trip counts depend on the arguments alone), all sums are exact int32 (the
// plan refuses what could overflow), and each output is a sum of a fixed set of integers formed by one owner: no result depends on the launch
// geometry.  gswm_tamper_plan.h decides every launch: the geometry the kernels take by value, the LDS layout, the refusals.
//
// Kernels, each [B] workgroups of 256
//   gsw_tile_agree_kernel    : LDS = the row d.  tile_walk counts its set bits; agree = n_t - that.
//   gsw_vote_tiled_kernel    : LDS = the row p.  vote_walk with the caller's uint16 [th, tw] weights in global memory (a few KiB, served by the vector
//                              cache); bits, score and wsum go straight out.
//   gsw_decode_robust_kernel : LDS = the row p, the planes, the int32 tile weights, the decoded message bytes, from the first round to the last; only the
//                              last round stores to global memory, and it stores every element of every output.  vote_walk with weights and message
//                              in LDS; tile_walk in the popcount form of the keyed soft search: with d = p ^ message,
//                              excess = wtot - 2 sum_k 2^k popc(plane_k & d), wtot = sum_k 2^k popc(plane_k); a round at unit levels has
//                              excess = n_t - 2 popc(d) and wsq = n_t.  wtot and wsq do not change between rounds: one tile_walk before the first
//                              round leaves them in LDS (wsq = sum_k 4^k popc(plane_k) + sum_{k < m} 2^(k + m + 1) popc(plane_k & plane_m)).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gswm.h"
#include "gswm_host.h"          // GSW_HIP, allow_dynamic_lds
#include "gswm_record.h"        // the record head (a row of `keys`), repeated_msg_word, ballot_byte
#include "gswm_tamper_plan.h"   // TileGeom, TM_WG, the three decisions, robust_isqrt

namespace {

constexpr int TM_TILE_LANES = 8;                     // lanes per tile of the tile walk

struct MapArgs {
    TileGeom g;
    const uint8_t* packed;    // [B, rowbytes]
    const uint8_t* keys;      // [B, 48]
    const uint8_t* msg;       // [B, msg_bytes]
    int32_t* agree;           // [B, tiles]
    int msg_aligned;          // message rows are whole, 4-byte aligned dwords
};

struct VoteOut {
    uint8_t* bits;            // [B, msg_bytes]
    int32_t* score;           // [B, msg_bits]
    int32_t* wsum;            // [B, msg_bits]
};

struct VoteArgs {
    TileGeom g;
    const uint8_t* packed;
    const uint8_t* keys;
    const uint16_t* weights;  // [B, tiles]
    VoteOut out;
};

struct RobustArgs {
    TileGeom g;
    const uint8_t* packed;
    const uint8_t* keys;
    const uint8_t* planes;    // [B, P, rowbytes]
    VoteOut out;              // of the LAST round, as the three below
    int32_t* excess;          // [B, tiles]
    int32_t* wsq;             // [B, tiles]
    int32_t* weights;         // [B, tiles]
    int P, iters, sign_rounds;
    int level_rounds;
    uint32_t planes_off, wgt_off, wtot_off, wsq_off, msg_off;
};

// LDS row <- packed row ^ keystream (^ message repeated, when WITH_MSG), dword w of the row at word w.  Words of the last block that
// lie past the row are written as zero and never read.
template <bool WITH_MSG>
__device__ __forceinline__ void stage_row(const TileGeom& g, const uint8_t* packed, const uint8_t* keys, const uint8_t* msgs, bool msg_aligned, int b, uint32_t* row_lds) {
    const int tid = threadIdx.x, col = tid & 3;
    const CipherLane ck = cipher_lane_of_record((const uint32_t*)(keys + (int64_t)b * GSW_REC_HEAD), (uint32_t)col);
    const uint8_t* q = packed + (int64_t)b * g.rowbytes;
    const uint8_t* msg = WITH_MSG ? msgs + (int64_t)b * g.msg_bytes : nullptr;
    for (int blk = tid >> 2; blk < g.nblk; blk += TM_WG >> 2) {
        uint32_t ks[4];
        chacha20_block(ck, (uint64_t)blk, (uint32_t)col, ks);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int byte0 = 64 * blk + 16 * r + 4 * col;
            uint32_t v = 0u;
            if (byte0 < g.rowbytes) {
                v = ks[r] ^ *(const uint32_t*)(q + byte0);
                if constexpr (WITH_MSG) v ^= repeated_msg_word(msg, (uint32_t)(byte0 % g.msg_bytes), (uint32_t)g.msg_bytes, msg_aligned);
            }
            row_lds[16 * blk + 4 * r + col] = v;
        }
    }
}

template <bool WORD>
__device__ __forceinline__ uint32_t lds_unit(const uint8_t* base, uint32_t off) {
    if constexpr (WORD) return *(const uint32_t*)(base + off);
    else return (uint32_t)base[off];
}

// The tile walk.  For every unit (WORD: dword, else byte) of every segment of a tile, unit(at, mo, acc) adds to the lane's N sums: `at` is the unit's byte
// offset in the row and, when MSG, `mo` its offset in the message repeated over the row (MSG false: the message is already folded into the row, mo = 0).
// done(tile, acc) runs in the tile's lane 0 with the tile's sums.  WORD needs whole-dword segments and, with MSG, a whole-dword message.
template <bool WORD, bool MSG, int N, typename Unit, typename Done>
__device__ __forceinline__ void tile_walk(const TileGeom& g, Unit unit, Done done) {
    const int tid = threadIdx.x, lane = tid & (TM_TILE_LANES - 1), T = 1 << g.log2t;
    const int seg_bytes = (T << g.log2l) >> 3;         // 1, 2, 4, 8 or 16: the bits one tile owns of one lattice row
    const int segs = g.C << g.log2t;                   // C T of them per tile
    const uint32_t mb = (uint32_t)g.msg_bytes;
    constexpr uint32_t U = WORD ? 4u : 1u;
    // the trip count is the same for every lane of a wave: the shuffles below run with all lanes on
    for (int tile0 = 0; tile0 < g.tiles; tile0 += TM_WG / TM_TILE_LANES) {
        const int tile = tile0 + tid / TM_TILE_LANES;
        int acc[N] = {};
        if (tile < g.tiles) {
            const int ty = tile / g.tw, tx = tile - ty * g.tw;
            for (int s = lane; s < segs; s += TM_TILE_LANES) {
                // segment s: the T l bits the tile owns of lattice row y = ty T + s % T of channel s / T
                const int c = s >> g.log2t, y = (ty << g.log2t) + (s & (T - 1));
                const uint32_t off = (uint32_t)(((((c * g.h + y) * g.w) + (tx << g.log2t)) << g.log2l) >> 3);           // < rowbytes <= 128 Ki
                uint32_t mo = MSG ? off % mb : 0u;     // WORD: off and mb are multiples of 4, and so is mo
                for (uint32_t i = 0; i < (uint32_t)seg_bytes; i += U) {
                    unit(off + i, mo, acc);
                    if constexpr (MSG) mo = mo + U == mb ? 0u : mo + U;
                }
            }
        }
#pragma unroll
        for (int d = 1; d < TM_TILE_LANES; d <<= 1) {
#pragma unroll
            for (int n = 0; n < N; ++n) acc[n] += __shfl_xor(acc[n], d);
        }
        if (lane == 0 && tile < g.tiles) done(tile, acc);
    }
}

// The vote walk: score, wsum and bit of every message bit of the image whose row is `row`.  wgt: the image's tile weights, uint16 in global memory or
// int32 in LDS.  UNIT: unit levels, else the level of a copy is gathered from the P planes at `pl`.  KEEP: the decoded bytes also go to msg (LDS).
// store: score, wsum and bits go to `out`, the image's own rows.
template <bool UNIT, bool KEEP, typename W>
__device__ __forceinline__ void vote_walk(const TileGeom& g, int P, const uint8_t* row, const uint8_t* pl, const W* wgt, uint8_t* msg, bool store, const VoteOut& out) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int S = 1 << g.log2s, s = tid & (S - 1);
    const uint32_t M = (uint32_t)g.msg_bits, w = (uint32_t)g.w, h = (uint32_t)g.h;
    const int per_pass = TM_WG >> g.log2s;             // message bits per pass of the workgroup, a multiple of 8 per wave
    for (int t0 = 0; t0 < g.msg_bits; t0 += per_pass) {
        const int t = t0 + (tid >> g.log2s);
        int sc = 0, ws = 0;
        if (t < g.msg_bits) {
            const uint32_t sh = 7u - ((uint32_t)t & 7u);                               // msg_bits % 8 == 0: every copy of t sits at this bit of its byte
            // copy k of t is bit j = k M + t < Nb <= 2^20, element e = j / l, lattice row q = e / w, x = e % w, y = q % h.  The lane's copies are S M bits apart,
            // a whole number of elements: the two divisions are paid once for the first copy and once for the stride, then (x, y) move by carries
            const uint32_t stride = (uint32_t)S * M, de = stride >> g.log2l, dq = de / w, dx = de - dq * w, dy = dq % h;
            const uint32_t j0 = (uint32_t)s * M + (uint32_t)t, e0 = j0 >> g.log2l, q0 = e0 / w;
            uint32_t x = e0 - q0 * w, y = q0 % h, idx = j0 >> 3;
            for (int k = s; k < g.copies; k += S) {
                const int p = (row[idx] >> sh) & 1;
                int wv = (int)wgt[(y >> g.log2t) * (uint32_t)g.tw + (x >> g.log2t)];
                if constexpr (!UNIT) {
                    int lev = 0;
#pragma unroll
                    for (int i = 0; i < RB_MAX_PLANES; ++i)
                        if (i < P) lev |= ((pl[(uint32_t)i * (uint32_t)g.rowbytes + idx] >> sh) & 1) << i;
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
        const bool one = t < g.msg_bits && sc > 0;
        const uint64_t ball = __ballot(one);           // bit (i S) of the wave's ballot: message bit (t of lane 0) + i
        if (t < g.msg_bits && s == 0) {
            const bool head = (t & 7) == 0;            // the seven bits after t are this wave's as well
            const uint8_t byte = head ? (uint8_t)ballot_byte(ball, (uint32_t)lane, (uint32_t)g.log2s) : (uint8_t)0;
            if (KEEP && head) msg[t >> 3] = byte;
            if (store) {
                out.score[t] = sc;
                out.wsum[t] = ws;
                if (head) out.bits[t >> 3] = byte;
            }
        }
    }
}

__device__ __forceinline__ VoteOut vote_out_of_image(const VoteOut& o, const TileGeom& g, int b) {
    return VoteOut{o.bits + (int64_t)b * g.msg_bytes, o.score + (int64_t)b * g.msg_bits, o.wsum + (int64_t)b * g.msg_bits};
}

__global__ __launch_bounds__(TM_WG) void gsw_tile_agree_kernel(MapArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const TileGeom& g = a.g;
    const int b = blockIdx.x;
    stage_row<true>(g, a.packed, a.keys, a.msg, a.msg_aligned != 0, b, (uint32_t*)lds_raw);       // d = q ^ cw
    __syncthreads();

    int32_t* out = a.agree + (int64_t)b * g.tiles;
    const uint8_t* row = lds_raw;
    auto done = [&](int tile, const int* acc) { out[tile] = g.n_t - acc[0]; };
    const bool seg_words = ((1 << g.log2t) << g.log2l) >> 3 >= 4;                                  // a segment is whole dwords
    if (seg_words) tile_walk<true, false, 1>(g, [&](uint32_t at, uint32_t, int* acc) { acc[0] += __popc(lds_unit<true>(row, at)); }, done);
    else tile_walk<false, false, 1>(g, [&](uint32_t at, uint32_t, int* acc) { acc[0] += __popc(lds_unit<false>(row, at)); }, done);
}

__global__ __launch_bounds__(TM_WG) void gsw_vote_tiled_kernel(VoteArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const TileGeom& g = a.g;
    const int b = blockIdx.x;
    stage_row<false>(g, a.packed, a.keys, nullptr, false, b, (uint32_t*)lds_raw);                  // p = q ^ ks
    __syncthreads();
    vote_walk<true, false>(g, 0, lds_raw, nullptr, a.weights + (int64_t)b * g.tiles, nullptr, true, vote_out_of_image(a.out, g, b));
}

// wtot[tau] and wsq[tau] of the levels, once for all rounds.  WORD: a segment is whole dwords.
template <bool WORD>
__device__ __forceinline__ void level_sums(const RobustArgs& r, const uint8_t* pl, int32_t* wtot, int32_t* wsq) {
    tile_walk<WORD, false, 2>(
        r.g,
        [&](uint32_t at, uint32_t, int* acc) {
            uint32_t v[RB_MAX_PLANES];
#pragma unroll
            for (int k = 0; k < RB_MAX_PLANES; ++k) v[k] = k < r.P ? lds_unit<WORD>(pl + (uint32_t)k * (uint32_t)r.g.rowbytes, at) : 0u;
#pragma unroll
            for (int k = 0; k < RB_MAX_PLANES; ++k) {
                const int n = __popc(v[k]);
                acc[0] += n << k;
                acc[1] += n << (2 * k);
#pragma unroll
                for (int m = k + 1; m < RB_MAX_PLANES; ++m) acc[1] += __popc(v[k] & v[m]) << (k + m + 1);
            }
        },
        [&](int tile, const int* acc) {
            wtot[tile] = acc[0];
            wsq[tile] = acc[1];
        });
}

// The map of one round against the message in LDS, and what follows from it: the next weights (in LDS), or the three tile outputs of the
// last round.  UNIT: the round votes at unit levels.  WORD: a segment and the message are whole dwords.
template <bool UNIT, bool WORD>
__device__ __forceinline__ void map_round(const RobustArgs& r, int b, bool last, const uint8_t* row, const uint8_t* pl, const uint8_t* msg, int32_t* wgt,
                                          const int32_t* wtot, const int32_t* wsq) {
    tile_walk<WORD, true, 1>(
        r.g,
        [&](uint32_t at, uint32_t mo, int* acc) {                                      // acc[0]: sum over the tile's bits with d_j = 1 of L_j
            const uint32_t d = lds_unit<WORD>(row, at) ^ lds_unit<WORD>(msg, mo);
            if constexpr (UNIT) {
                acc[0] += __popc(d);
            } else {
#pragma unroll
                for (int k = 0; k < RB_MAX_PLANES; ++k)
                    if (k < r.P) acc[0] += __popc(lds_unit<WORD>(pl + (uint32_t)k * (uint32_t)r.g.rowbytes, at) & d) << k;
            }
        },
        [&](int tile, const int* acc) {
            const int tot = UNIT ? r.g.n_t : wtot[tile], sq = UNIT ? r.g.n_t : wsq[tile];
            const int ex = tot - 2 * acc[0];
            if (last) {
                const int64_t o = (int64_t)b * r.g.tiles + tile;
                r.excess[o] = ex;
                r.wsq[o] = sq;
                r.weights[o] = wgt[tile];                                              // what the last vote used
            } else {
                const int nw = ex - (int)robust_isqrt((uint32_t)sq);
                wgt[tile] = nw > 0 ? nw : 0;
            }
        });
}

__global__ __launch_bounds__(TM_WG) void gsw_decode_robust_kernel(RobustArgs r) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const TileGeom& g = r.g;
    const int b = blockIdx.x, tid = threadIdx.x;
    uint8_t* pl = lds_raw + r.planes_off;
    int32_t* wgt = (int32_t*)(lds_raw + r.wgt_off);
    int32_t* wtot = (int32_t*)(lds_raw + r.wtot_off);
    int32_t* wsq = (int32_t*)(lds_raw + r.wsq_off);
    uint8_t* msg = lds_raw + r.msg_off;

    stage_row<false>(g, r.packed, r.keys, nullptr, false, b, (uint32_t*)lds_raw);                  // p = q ^ ks
    const int pwords = r.P * (g.rowbytes >> 2);        // rowbytes is a multiple of 8: the planes of an image are whole, 4-byte aligned dwords
    const uint32_t* src = (const uint32_t*)(r.planes + (int64_t)b * r.P * g.rowbytes);
    for (int i = tid; i < pwords; i += TM_WG) ((uint32_t*)pl)[i] = src[i];
    for (int i = tid; i < g.tiles; i += TM_WG) wgt[i] = 1;
    __syncthreads();

    const int seg_bytes = ((1 << g.log2t) << g.log2l) >> 3;                           // 1, 2, 4, 8 or 16, a segment aligned to its own size
    const bool seg_words = seg_bytes >= 4, map_words = seg_words && (g.msg_bytes & 3) == 0;
    if (r.level_rounds) {                              // (its results are first read after the barrier that ends the first vote)
        if (seg_words) level_sums<true>(r, pl, wtot, wsq);
        else level_sums<false>(r, pl, wtot, wsq);
    }
    const VoteOut out = vote_out_of_image(r.out, g, b);
    for (int round = 0; round <= r.iters; ++round) {
        const bool last = round == r.iters, unit = r.P == 0 || round < r.sign_rounds;
        if (unit) vote_walk<true, true>(g, r.P, lds_raw, pl, wgt, msg, last, out);
        else vote_walk<false, true>(g, r.P, lds_raw, pl, wgt, msg, last, out);
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

template <typename K, typename A>
int launch(K kernel, const A& a, int grid, uint32_t lds, void* stream) {
    GSW_HIP(allow_dynamic_lds((const void*)kernel, lds));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(TM_WG), lds, (hipStream_t)stream, a);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

TileQuery tile_query(const uint8_t* packed_dev, int B, int C, int h, int w, int l, int tile, const uint8_t* keys_dev, int msg_bits, bool own_null, const void* weights_dev) {
    return TileQuery{B, C, h, w, l, tile, msg_bits, own_null, ((uintptr_t)weights_dev & 1) == 0, !packed_dev, !keys_dev, ((uintptr_t)packed_dev & 3) == 0, ((uintptr_t)keys_dev & 3) == 0};
}

}  // namespace

extern "C" {

int gsw_tile_agree(const uint8_t* packed_dev, int B, int C, int h, int w, int l, int tile, const uint8_t* keys_dev, const uint8_t* msg_dev,
                   int msg_bits, int32_t* agree_dev, void* stream) {
    const TilePlan p = tile_decide(tile_query(packed_dev, B, C, h, w, l, tile, keys_dev, msg_bits, !msg_dev || !agree_dev, nullptr), false);
    if (p.status != GSW_OK) return p.status;
    const MapArgs a{p.g, packed_dev, keys_dev, msg_dev, agree_dev, (p.g.msg_bytes % 4 == 0) && ((uintptr_t)msg_dev % 4 == 0)};
    return launch(gsw_tile_agree_kernel, a, p.grid, p.lds, stream);
}

int gsw_vote_tiled(const uint8_t* packed_dev, int B, int C, int h, int w, int l, int tile, const uint8_t* keys_dev, const uint16_t* weights_dev,
                   int msg_bits, uint8_t* bits_dev, int32_t* score_dev, int32_t* wsum_dev, void* stream) {
    const TilePlan p = tile_decide(tile_query(packed_dev, B, C, h, w, l, tile, keys_dev, msg_bits, !weights_dev || !bits_dev || !score_dev || !wsum_dev, weights_dev), true);
    if (p.status != GSW_OK) return p.status;
    const VoteArgs a{p.g, packed_dev, keys_dev, weights_dev, VoteOut{bits_dev, score_dev, wsum_dev}};
    return launch(gsw_vote_tiled_kernel, a, p.grid, p.lds, stream);
}

int gsw_decode_robust(const uint8_t* signs_dev, const uint8_t* planes_dev, int P, int B, int C, int h, int w, int l, int tile, const uint8_t* keys_dev,
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
    const RobustArgs r{p.g, signs_dev, keys_dev, planes_dev, VoteOut{bits_dev, score_dev, wsum_dev}, excess_dev, wsq_dev, weights_dev, P, iters, sign_rounds, p.level_rounds,
                       p.planes_off, p.wgt_off, p.wtot_off, p.wsq_off, p.msg_off};
    return launch(gsw_decode_robust_kernel, r, p.grid, p.lds, stream);
}

}  // extern "C"
