// gswm_record.h -- "an image under its own record", the decisions every kernel family of that kind shares (gswm_codec_keyed.inc,
// gswm_codec_soft.inc, gswm_keyed.hip, gswm_tamper.hip): the record layout and its operand check, the message repeated over a row, the
// record's keystream in LDS, and the tail of a per-image vote.  The block function and the counter rule are gswm_chacha.h's.
// Include after <hip/hip_runtime.h> and include/gswm.h.  A host compiler (gswm_search_plan.h's table program, gswm_tamper_plan.h's sweep) sees the layout, the operand check and vote_log2s only.
#pragma once
#include <stdint.h>

// A record is key[32] | nonce16[16] | message[msg_bytes]: uint8 rows, 16-byte aligned, at a stride that is a multiple of 16.
constexpr int GSW_REC_HEAD = 48;                     // key[32] | nonce16[16]
// The bits of one image's row.  A kernel that stages a row (its keystream, its decrypted bits, its sign bits) keeps it in LDS:
// 1 048 576 bits are 128 KiB of the CU's 160.
constexpr int64_t GSW_ROW_MAX_BITS = 1048576;

// what every entry point asks of its records; the pointer as two facts (gswm_search_plan.h decides without pointers)
static inline int records_layout_check(bool present, bool aligned16, int64_t record_stride, int msg_bytes, int64_t n_records) {
    if (!present || n_records < 1) return GSW_ERR_BAD_ARG;
    if (msg_bytes < 1 || msg_bytes > GSW_MSG_INLINE_MAX) return GSW_ERR_BAD_ARG;
    if (record_stride < (int64_t)GSW_REC_HEAD + msg_bytes || record_stride % 16) return GSW_ERR_BAD_ARG;
    return aligned16 ? GSW_OK : GSW_ERR_BAD_ARG;
}
static inline int records_check(const uint8_t* records_dev, int64_t record_stride, int msg_bytes, int64_t n_records) {
    return records_layout_check(records_dev != nullptr, ((uintptr_t)records_dev & 15u) == 0, record_stride, msg_bytes, n_records);
}
// ... of the entry points that keep the stride in 32 bits
static inline int records_check32(const uint8_t* records_dev, int64_t record_stride, int msg_bytes, int64_t n_records) {
    if (record_stride > (int64_t)0x7FFFFFF0) return GSW_ERR_BAD_ARG;
    return records_check(records_dev, record_stride, msg_bytes, n_records);
}

// Lanes per message bit of a per-image vote (its tail is below): enough to fill the workgroup for short messages, at most 8 (a wave then
// still owns whole bytes) and at most the copies.  Host arithmetic: gswm_tamper_plan.h decides with it.
static inline int vote_log2s(int64_t msg_bits, int64_t copies, int wg) {
    int log2s = 0;
    while (log2s < 3 && (msg_bits << log2s) < wg && ((int64_t)2 << log2s) <= copies) ++log2s;
    return log2s;
}

#ifdef __HIPCC__      // device code from here on
#include "gswm_chacha.h"

// The message repeated over the row: the four bytes at offset o, o + 1, .. (mod msg_bytes, o < msg_bytes) as a little-endian word.
// `dword`: msg_bytes % 4 == 0, o % 4 == 0 and the message is 4-byte aligned -- one load.  Otherwise byte by byte, wrapping by compare;
// only the first `valid` bytes are read, the others are zero.  `valid` has one user, the keyed embed, whose row carries the message up to
// its last whole copy and zeros after it; the search and the tile kernels only walk whole copies and leave it at 4.
__device__ __forceinline__ uint32_t repeated_msg_word(const uint8_t* __restrict__ msg, uint32_t o, uint32_t msg_bytes, bool dword, int valid = 4) {
    if (dword) return *reinterpret_cast<const uint32_t*>(msg + o);
    uint32_t m = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i < valid) m |= (uint32_t)msg[o] << (8 * i);
        o = o + 1u == msg_bytes ? 0u : o + 1u;
    }
    return m;
}

// Keystream blocks [0, nblk) of the record at `rec` into lds[nblk * 16], by every quad of a workgroup of WG threads; the caller's barrier
// follows.
template <int WG>
__device__ __forceinline__ void record_keystream_to_lds(const uint8_t* __restrict__ rec, uint32_t nblk, uint32_t* lds) {
    const uint32_t tid = threadIdx.x, col = tid & 3u;
    const CipherLane ck = cipher_lane_of_record(reinterpret_cast<const uint32_t*>(rec), col);
    for (uint32_t blk = tid >> 2; blk < nblk; blk += WG >> 2) {
        uint32_t ks[4];
        chacha20_block(ck, (uint64_t)blk, col, ks);
#pragma unroll
        for (int r = 0; r < 4; ++r) lds[16u * blk + 4u * r + col] = ks[r];
    }
}

// ---- the tail of a per-image vote: S = 1 << log2s adjacent lanes per message bit, the message byte from the wave's ballot

// Bit (i S) of the wave's ballot above lane `lane` is message bit (t of that lane) + i: the byte that starts at the lane's bit, MSB first.
__device__ __forceinline__ uint32_t ballot_byte(uint64_t ball, uint32_t lane, uint32_t log2s) {
    uint32_t v = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) v |= (uint32_t)((ball >> (lane + ((uint32_t)i << log2s))) & 1ull) << (7 - i);
    return v;
}

// The end of a workgroup of WAVES waves, after its barrier: s_match holds the matching bits per message byte, s_flags[WAVES] the flags
// per wave; the first wave adds them up and lane 0 stores the image's two words.
template <int WAVES>
__device__ __forceinline__ void store_matches_flags(const uint32_t* s_match, const uint32_t* s_flags, uint32_t msg_bytes, uint32_t* matches,
                                                    uint32_t* flags, uint32_t b) {
    const uint32_t tid = threadIdx.x;
    if (tid < 64u) {
        uint32_t m = 0;
        for (uint32_t i = tid; i < msg_bytes; i += 64u) m += s_match[i];
        for (int sh = 32; sh > 0; sh >>= 1) m += __shfl_xor(m, sh, 64);
        if (tid == 0) {
            if (matches) matches[b] = m;
            uint32_t f = s_flags[0];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) f |= s_flags[w];
            flags[b] = f;
        }
    }
}
#endif  // __HIPCC__
