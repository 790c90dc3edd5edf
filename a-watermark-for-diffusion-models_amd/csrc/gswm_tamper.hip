// gswm_tamper.hip -- where an image still agrees with a codeword, and a vote that listens to those places, gfx950.
//
//   q        the image's quantised bits, packed MSB first (gsw_sign_pack / gsw_quant_pack): element i = (c, y, x) of the [C, h, w]
//            lattice owns bits [i l, i l + l)
//   ks       the keystream of the image's own (key, nonce16), initial counter and carry as gsw_keystream
//   cw_j     = ks_j ^ m[j mod M]                                  the cipher bits gsw_embed[_l] plants for message m (its codeword)
//   agree[b, ty, tx] = #{ j in tile (ty, tx) : q_j == cw_j }      tile = the elements of ALL channels with y / T == ty, x / T == tx
//   p_j      = q_j ^ ks_j                                         the decrypted bit
//   score[b, t] = sum_{j = t (mod M)} wgt[tile(j / l)] (2 p_j - 1),   wsum[b, t] = sum_{j = t (mod M)} wgt[tile(j / l)]
//   bit_t    = score > 0                                          (a tie or no weight at all -> 0, the reference's tie rule)
//
// One workgroup per image, every image under its own key.  Both kernels start the same way: the quads of the workgroup compute the
// ChaCha20 blocks of the image's keystream with gswm_chacha.h's chacha20_block and, still in registers, XOR them with
// the packed row (and, for the map, the message): what reaches LDS is the row of differences d = q ^ cw (map) or of decrypted bits p
// (vote), in the row's own byte order.  No keystream and no codeword exists in memory.  h and w are multiples of T and T of 8, so a
// row is a whole number of dwords and the T l bits a tile owns of one lattice row are T l / 8 whole bytes, aligned to their own size.
//
// Map.  Eight adjacent lanes own a tile: lane g takes the row segments g, g + 8, .. of its C T segments, counts their set bits and the
// eight partial counts meet in three __shfl_xor steps (distances 1, 2, 4: inside a row of eight lanes, DPP moves).  The lane with
// g == 0 stores n_t minus the differences.  Every tile is written by exactly one lane: no atomics, nothing to zero first.
//
// Vote.  S adjacent lanes (a power of two up to 8, chosen on the host so that small messages still fill the workgroup) own a message
// bit t and walk its copies j = t + k M, k = s, s + S, ..: the bit comes from LDS, the element's tile from two divisions, its weight
// from the caller's [th, tw] table (a few KiB, served by the vector cache).  The S partial sums meet by __shfl_xor, and the eight
// sign bits of a byte of the message are collected from the wave's ballot.  All sums are int32 and exact: the host refuses a vote
// whose copies x 65535 could overflow.
//
// Neither result depends on the launch geometry: each output element is the sum of a fixed set of integers, formed by one owner.
//
// Kernels
//   gsw_tile_agree_kernel : [B] workgroups of 256
//   gsw_vote_tiled_kernel : [B] workgroups of 256
//   gsw_decode_robust_kernel (gswm_tamper_soft.inc) : the vote, the map and the weights of every round in one launch, with reliability levels
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gswm.h"
#include "gswm_host.h"     // GSW_HIP, allow_dynamic_lds
#include "gswm_record.h"   // the record head (a row of `keys`), GSW_ROW_MAX_BITS, repeated_msg_word, the vote tail

namespace {

constexpr int TM_WG = 256;
constexpr int TM_TILE_LANES = 8;                     // lanes per tile of the map

struct TamperArgs {
    const uint8_t* packed;    // [B, rowbytes]
    const uint8_t* keys;      // [B, 48]
    const uint8_t* msg;       // [B, msg_bytes] (map only)
    const uint16_t* weights;  // [B, th * tw] (vote only)
    int32_t* agree;           // [B, th * tw]
    uint8_t* bits;            // [B, msg_bytes]
    int32_t* score;           // [B, msg_bits]
    int32_t* wsum;            // [B, msg_bits]
    int C, h, w;
    int log2l, log2t;
    int tw, tiles;            // tiles per lattice row, per image
    int rowbytes;             // Nb / 8, a multiple of 8
    int nblk;                 // ChaCha blocks per row, the last one possibly partial
    int msg_bits, msg_bytes;
    int msg_aligned;          // message rows are whole, 4-byte aligned dwords
    int copies;               // Nb / msg_bits
    int log2s;                // vote: lanes per message bit
};

// LDS row <- packed row ^ keystream (^ message repeated, when WITH_MSG), dword w of the row at word w.  Words of the last block that
// lie past the row are written as zero and never read.
template <bool WITH_MSG>
__device__ __forceinline__ void stage_row(const TamperArgs& a, int b, uint32_t* row_lds) {
    const int tid = threadIdx.x, col = tid & 3;
    const CipherLane ck = cipher_lane_of_record((const uint32_t*)(a.keys + (int64_t)b * GSW_REC_HEAD), (uint32_t)col);
    const uint8_t* q = a.packed + (int64_t)b * a.rowbytes;
    const uint8_t* msg = WITH_MSG ? a.msg + (int64_t)b * a.msg_bytes : nullptr;
    for (int blk = tid >> 2; blk < a.nblk; blk += TM_WG >> 2) {
        uint32_t ks[4];
        chacha20_block(ck, (uint64_t)blk, (uint32_t)col, ks);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int byte0 = 64 * blk + 16 * r + 4 * col;
            uint32_t v = 0u;
            if (byte0 < a.rowbytes) {
                v = ks[r] ^ *(const uint32_t*)(q + byte0);
                if constexpr (WITH_MSG) v ^= repeated_msg_word(msg, (uint32_t)(byte0 % a.msg_bytes), (uint32_t)a.msg_bytes, a.msg_aligned != 0);
            }
            row_lds[16 * blk + 4 * r + col] = v;
        }
    }
}

__global__ __launch_bounds__(TM_WG) void gsw_tile_agree_kernel(TamperArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    uint32_t* row = (uint32_t*)lds_raw;                // d = q ^ cw
    const int b = blockIdx.x, tid = threadIdx.x;
    stage_row<true>(a, b, row);
    __syncthreads();

    const int T = 1 << a.log2t;
    const int seg_bytes = (T << a.log2l) >> 3;         // 1, 2, 4, 8 or 16: the bits one tile owns of one lattice row
    const int segs = a.C << a.log2t;                   // C T of them per tile
    const int n_t = segs * seg_bytes * 8;
    const int g = tid & (TM_TILE_LANES - 1);
    int32_t* out = a.agree + (int64_t)b * a.tiles;
    // the trip count is the same for every lane of a wave: the shuffles below run with all lanes on
    for (int tile0 = 0; tile0 < a.tiles; tile0 += TM_WG / TM_TILE_LANES) {
        const int tile = tile0 + tid / TM_TILE_LANES;
        int diff = 0;
        if (tile < a.tiles) {
            const int ty = tile / a.tw, tx = tile - ty * a.tw;
            for (int s = g; s < segs; s += TM_TILE_LANES) {
                const int c = s >> a.log2t, y = (ty << a.log2t) + (s & (T - 1));
                const int off = ((((c * a.h + y) * a.w) + (tx << a.log2t)) << a.log2l) >> 3;     // < rowbytes <= 128 Ki
                if (seg_bytes >= 4) {
                    for (int i = 0; i < seg_bytes / 4; ++i) diff += __popc(row[(off >> 2) + i]);
                } else {
                    for (int i = 0; i < seg_bytes; ++i) diff += __popc((uint32_t)lds_raw[off + i]);
                }
            }
        }
        diff += __shfl_xor(diff, 1);
        diff += __shfl_xor(diff, 2);
        diff += __shfl_xor(diff, 4);
        if (g == 0 && tile < a.tiles) out[tile] = n_t - diff;
    }
}

__global__ __launch_bounds__(TM_WG) void gsw_vote_tiled_kernel(TamperArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    stage_row<false>(a, b, (uint32_t*)lds_raw);        // p = q ^ ks
    __syncthreads();

    const int S = 1 << a.log2s, s = tid & (S - 1);
    const uint32_t M = (uint32_t)a.msg_bits, w = (uint32_t)a.w, h = (uint32_t)a.h;
    const uint16_t* wgt = a.weights + (int64_t)b * a.tiles;
    uint8_t* bits = a.bits + (int64_t)b * a.msg_bytes;
    int32_t* score = a.score + (int64_t)b * a.msg_bits;
    int32_t* wsum = a.wsum + (int64_t)b * a.msg_bits;
    const int per_pass = TM_WG >> a.log2s;             // message bits per pass of the workgroup, a multiple of 8 per wave
    for (int t0 = 0; t0 < a.msg_bits; t0 += per_pass) {
        const int t = t0 + (tid >> a.log2s);
        int sc = 0, ws = 0;
        if (t < a.msg_bits) {
            for (int k = s; k < a.copies; k += S) {
                const uint32_t j = (uint32_t)k * M + (uint32_t)t;                   // < Nb <= 2^20
                const int p = (lds_raw[j >> 3] >> (7u - (j & 7u))) & 1;
                const uint32_t e = j >> a.log2l, r = e / w, x = e - r * w, y = r % h;
                const int wv = (int)wgt[(y >> a.log2t) * (uint32_t)a.tw + (x >> a.log2t)];
                sc += p ? wv : -wv;
                ws += wv;
            }
        }
        for (int step = 1; step < S; step <<= 1) {
            sc += __shfl_xor(sc, step);
            ws += __shfl_xor(ws, step);
        }
        const bool one = t < a.msg_bits && sc > 0;
        const uint64_t ball = __ballot(one);           // bit (i S) of the wave's ballot: message bit (t of lane 0) + i
        if (t < a.msg_bits && s == 0) {
            score[t] = sc;
            wsum[t] = ws;
            if ((t & 7) == 0) {                        // msg_bits % 8 == 0: the seven bits after t are this wave's as well
                bits[t >> 3] = (uint8_t)ballot_byte(ball, (uint32_t)lane, (uint32_t)a.log2s);
            }
        }
    }
}

int ilog2(int v) {
    int r = 0;
    while ((1 << r) < v) ++r;
    return r;
}

// the checks both entry points share; fills the geometry of `a`
int prepare(TamperArgs& a, const uint8_t* packed_dev, int B, int C, int h, int w, int l, int tile, const uint8_t* keys_dev, int msg_bits) {
    if (!packed_dev || !keys_dev) return GSW_ERR_BAD_ARG;
    if (B < 1 || C < 1 || h < 1 || w < 1 || msg_bits < 1) return GSW_ERR_BAD_ARG;
    if (l != 1 && l != 2 && l != 4) return GSW_ERR_BAD_ARG;
    if (((uintptr_t)packed_dev & 3) || ((uintptr_t)keys_dev & 3)) return GSW_ERR_BAD_ARG;
    if (tile != 8 && tile != 16 && tile != 32) return GSW_ERR_UNSUPPORTED;
    if (h % tile || w % tile || msg_bits % 8) return GSW_ERR_UNSUPPORTED;
    const int64_t nb = (int64_t)C * h * w * l;
    if (nb > GSW_ROW_MAX_BITS) return GSW_ERR_UNSUPPORTED;
    if (nb % msg_bits) return GSW_ERR_RAGGED;
    a = TamperArgs{};
    a.packed = packed_dev;
    a.keys = keys_dev;
    a.C = C; a.h = h; a.w = w;
    a.log2l = ilog2(l);
    a.log2t = ilog2(tile);
    a.tw = w / tile;
    a.tiles = (h / tile) * a.tw;
    a.rowbytes = (int)(nb / 8);
    a.nblk = (a.rowbytes + 63) / 64;
    a.msg_bits = msg_bits;
    a.msg_bytes = msg_bits / 8;
    a.copies = (int)(nb / msg_bits);
    return GSW_OK;
}

template <typename K>
int launch(K kernel, const TamperArgs& a, int B, hipStream_t st) {
    const uint32_t lds = (uint32_t)a.nblk * 64u;
    GSW_HIP(allow_dynamic_lds((const void*)kernel, lds));
    hipLaunchKernelGGL(kernel, dim3(B), dim3(TM_WG), lds, st, a);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

}  // namespace

extern "C" {

int gsw_tile_agree(const uint8_t* packed_dev, int B, int C, int h, int w, int l, int tile, const uint8_t* keys_dev, const uint8_t* msg_dev,
                   int msg_bits, int32_t* agree_dev, void* stream) {
    if (!msg_dev || !agree_dev) return GSW_ERR_BAD_ARG;
    TamperArgs a;
    const int rc = prepare(a, packed_dev, B, C, h, w, l, tile, keys_dev, msg_bits);
    if (rc != GSW_OK) return rc;
    a.msg = msg_dev;
    a.msg_aligned = (a.msg_bytes % 4 == 0) && ((uintptr_t)msg_dev % 4 == 0);
    a.agree = agree_dev;
    return launch(gsw_tile_agree_kernel, a, B, (hipStream_t)stream);
}

int gsw_vote_tiled(const uint8_t* packed_dev, int B, int C, int h, int w, int l, int tile, const uint8_t* keys_dev, const uint16_t* weights_dev,
                   int msg_bits, uint8_t* bits_dev, int32_t* score_dev, int32_t* wsum_dev, void* stream) {
    if (!weights_dev || !bits_dev || !score_dev || !wsum_dev) return GSW_ERR_BAD_ARG;
    if ((uintptr_t)weights_dev & 1) return GSW_ERR_BAD_ARG;
    TamperArgs a;
    const int rc = prepare(a, packed_dev, B, C, h, w, l, tile, keys_dev, msg_bits);
    if (rc != GSW_OK) return rc;
    if ((int64_t)a.copies * 65535 > (int64_t)INT32_MAX) return GSW_ERR_UNSUPPORTED;      // a message bit's score would not fit int32
    a.weights = weights_dev;
    a.bits = bits_dev;
    a.score = score_dev;
    a.wsum = wsum_dev;
    a.log2s = vote_log2s(msg_bits, a.copies, TM_WG);
    return launch(gsw_vote_tiled_kernel, a, B, (hipStream_t)stream);
}

}  // extern "C"

#include "gswm_tamper_soft.inc"   // gsw_decode_robust: the rounds of the robust decode in one launch, tile weights times reliability levels
