// gswm_chacha.h -- the ChaCha20 block function of the codec family.  chacha20_block computes one block of a cipher whose words a lane
// holds as a CipherLane (cipher_lane_of_record: the per-record codec, the keyed registry search, the tile kernels);
// chacha20_blocks_to_lds is the shared-key kernels' loop (keystream, embed, extract), whose cipher words are kernel arguments and whose
// instruction stream the benchmark times: it keeps its own copy of the rounds.  Device code only; include after <hip/hip_runtime.h>.
#pragma once
#include <stdint.h>

// ------------------------------------------------------------------------------------------------
// ChaCha20, four lanes per 64-byte block.
// Lane q of a quad holds column q of the 4x4 state (a = row0[q], b = row1[q], c = row2[q], d = row3[q]).
// The column round is lane-local; for the diagonal round rows 1..3 are rotated by 1..3 lanes inside the
// quad with DPP quad_perm (no LDS, no extra latency beyond a VALU move), then rotated back.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t rotl32(uint32_t x, int n) { return __builtin_rotateleft32(x, n); }

template <int CTRL>
__device__ __forceinline__ uint32_t quad_perm(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}
// quad_perm selectors: lane i reads lane sel[i]
#define QP_ROT1 0x39  // [1,2,3,0]
#define QP_ROT2 0x4E  // [2,3,0,1]
#define QP_ROT3 0x93  // [3,0,1,2]

#define CHACHA_QR(a, b, c, d) \
    a += b; d = rotl32(d ^ a, 16); \
    c += d; b = rotl32(b ^ c, 12); \
    a += b; d = rotl32(d ^ a, 8);  \
    c += d; b = rotl32(b ^ c, 7);

// A lane's share of a cipher: column `col` of the initial state below the sigma row (which is a function of col alone and so not kept
// here: a loop that walks records would carry it along), the counter as the 64-bit number it is (state words 12 and 13: the 32-bit
// counter carries into the next word, as OpenSSL's) and the lane's word of the nonce tail.
struct CipherLane {
    uint32_t b0, c0;   // key words col, 4 + col
    uint32_t n0, n1;   // initial counter, low and high word
    uint32_t n23;      // state word 12 + col of the lanes col = 2, 3 (nonce16 words 2, 3); the other two lanes do not use it
};

// A lane's share of the cipher of a record head key[32] | nonce16[16] in memory (4-byte aligned), as 32-bit loads by lane `col`.
__device__ __forceinline__ CipherLane cipher_lane_of_record(const uint32_t* __restrict__ rec, uint32_t col) {
    return CipherLane{rec[col], rec[4 + col], rec[8], rec[9], rec[8 + (col | 2u)]};
}

// ChaCha20 block `initial counter + block` of a cipher, four lanes per block: lane col of the quad returns words col, 4 + col, 8 + col,
// 12 + col of the block, i.e. bytes 16 r + 4 col .. + 3 for r = 0 .. 3.  All four lanes of the quad call it together.
// The counter rule and the rounds are written out in two more places, which change together with this one: chacha20_blocks_to_lds below
// and the record loop of gsw_trace_keyed_scan_kernel (gswm_keyed.hip); each says why.
__device__ __forceinline__ void chacha20_block(const CipherLane ck, uint64_t block, uint32_t col, uint32_t (&ks)[4]) {
    const uint32_t a0 = col == 0 ? 0x61707865u : col == 1 ? 0x3320646eu : col == 2 ? 0x79622d32u : 0x6b206574u;
    const uint64_t ctr = (((uint64_t)ck.n1 << 32) | ck.n0) + block;
    const uint32_t d0 = col == 0 ? (uint32_t)ctr : col == 1 ? (uint32_t)(ctr >> 32) : ck.n23;
    uint32_t a = a0, b = ck.b0, c = ck.c0, d = d0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        CHACHA_QR(a, b, c, d)
        b = quad_perm<QP_ROT1>(b); c = quad_perm<QP_ROT2>(c); d = quad_perm<QP_ROT3>(d);
        CHACHA_QR(a, b, c, d)
        b = quad_perm<QP_ROT3>(b); c = quad_perm<QP_ROT2>(c); d = quad_perm<QP_ROT1>(d);
    }
    ks[0] = a + a0; ks[1] = b + ck.b0; ks[2] = c + ck.c0; ks[3] = d + d0;
}

// Computes ChaCha20 blocks [first_block, first_block + nblocks) into ks_words[nblocks*16] (LDS), using every lane
// of the workgroup in quads.  All lanes of a participating quad are active together (4 | blockDim, tid-contiguous).
// The cipher words are taken BY VALUE (SGPRs): handing the by-value kernel-argument struct around by reference
// makes clang materialise it in scratch.
// Written out, not as a loop over chacha20_block: these are the kernels the benchmark times, and gathering the lane's words in a
// CipherLane first gives every one of them a different instruction stream (profiles/record_refactor_resources.txt).
struct CipherRegs {
    uint32_t k0, k1, k2, k3, k4, k5, k6, k7, n0, n1, n2, n3;
};
#define GSW_CIPHER_REGS(ck) CipherRegs{(ck).key[0], (ck).key[1], (ck).key[2], (ck).key[3], (ck).key[4], (ck).key[5], \
                                       (ck).key[6], (ck).key[7], (ck).nonce[0], (ck).nonce[1], (ck).nonce[2], (ck).nonce[3]}

__device__ __forceinline__ void chacha20_blocks_to_lds(const CipherRegs ck, uint64_t first_block, uint32_t nblocks,
                                                       uint32_t* ks_words) {
    const uint32_t tid = threadIdx.x;
    const uint32_t col = tid & 3u;
    const uint32_t a0 = col == 0 ? 0x61707865u : col == 1 ? 0x3320646eu : col == 2 ? 0x79622d32u : 0x6b206574u;
    const uint32_t b0 = col == 0 ? ck.k0 : col == 1 ? ck.k1 : col == 2 ? ck.k2 : ck.k3;
    const uint32_t c0 = col == 0 ? ck.k4 : col == 1 ? ck.k5 : col == 2 ? ck.k6 : ck.k7;
    const uint64_t ctr_base = ((uint64_t)ck.n1 << 32) | ck.n0;
    for (uint32_t blk = tid >> 2; blk < nblocks; blk += blockDim.x >> 2) {
        const uint64_t ctr = ctr_base + first_block + (uint64_t)blk;
        const uint32_t d0 = col == 0 ? (uint32_t)ctr : col == 1 ? (uint32_t)(ctr >> 32) : col == 2 ? ck.n2 : ck.n3;
        uint32_t a = a0, b = b0, c = c0, d = d0;
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            CHACHA_QR(a, b, c, d)
            b = quad_perm<QP_ROT1>(b); c = quad_perm<QP_ROT2>(c); d = quad_perm<QP_ROT3>(d);
            CHACHA_QR(a, b, c, d)
            b = quad_perm<QP_ROT3>(b); c = quad_perm<QP_ROT2>(c); d = quad_perm<QP_ROT1>(d);
        }
        uint32_t* o = ks_words + blk * 16 + col;
        o[0] = a + a0; o[4] = b + b0; o[8] = c + c0; o[12] = d + d0;
    }
}
