// gswm_counts_align_soft.inc -- the level-weighted vote of every candidate alignment of gsw_level_pack's rows under ONE key, in one launch (gfx950): the operand
// of a registry search over (record, alignment) pairs ranked by reliability levels (gsw_trace_topk on the [B A, M] scores).  Included at the end of
// gswm_keyed.hip after gswm_align_soft.inc and gswm_counts_align.inc: align_map is gswm_align.inc's, level_align_gather gswm_align_soft.inc's, GSW_HIP and
// allow_dynamic_lds gswm_host.h's, chacha20_blocks_to_lds gswm_chacha.h's; the policy is level_counts_align_decide (gswm_counts_align_soft_plan.h).
//
//   score[b, a, t] = bias + sum over p = t (mod M) of level_p (2 d_p - 1)
//   wsum [b, a, t] =        sum over p = t (mod M) of level_p                      (optional: a null pointer skips it)
//
// d_p = (bit p of gsw_rows_align's row (b, a) of the sign row) ^ (keystream bit p), level_p = sum_k 2^k (bit p of the aligned plane k): gsw_extract_soft's score
// and wsum of the aligned image under the table the rows were packed with.  It is gsw_counts_align for level rows: the aligned rows are never written, 4 M
// (or 8 M) bytes leave the chip per (image, alignment) instead of (1 + P) n / 8.
//
// Work split as gsw_counts_align_kernel.  Grid (alignment chunks, images), 256 lanes.  A workgroup stages its image's 1 + P rows and generates the keystream into
// LDS, both once, then walks its chunk.  Per alignment, on the word path (M % 32 == 0): a lane computes the source bit of each of a word's 32 elements ONCE
// (level_align_gather<L, 1 + P>), forms d = signs ^ keystream once, and per plane k adds plane_k & d to the vertical counters X_k and plane_k to N_k.  Lane `tid`
// only ever sees message word tid % (M / 32), so its counters are 32 adjacent message positions.  It combines its planes in registers, X' = sum_k 2^k X_k and
// N' = sum_k 2^k N_k (two positions per dword, 11 bits used of 16), leaves 32 + 32 uint16 in the reduction region, and after a barrier lane t sums column t over
// the lanes that share its message word and stores bias + 2 X' - N' and N': coalesced dwords, no atomic.  The byte path (any other M % 8 == 0) is the same
// with bytes and eight int32 accumulators of each kind.
//
// An entry with d outside 0..7, or an odd d on a non-square lattice, has no map: its M scores are written as `bias`, its wsum as zeros, nothing is read
// through it.
//
// Kernel
//   gsw_level_counts_align_kernel<L, P, WORDS> : L bits per element (1 here; 2 and 4 are gswm_counts_align_soft_l.inc's), P level planes (1..4); WORDS: the
//                                                word path

namespace {

struct LevelCountsAlignArgs {
    const uint8_t* signs;     // [B, rowbytes]
    const uint8_t* planes;    // [B, P, rowbytes]
    const int32_t* aligns;    // [A, 3]
    int32_t* score;           // [B, A, M]
    int32_t* wsum;            // [B, A, M] or null
    uint32_t k0, k1, k2, k3, k4, k5, k6, k7, n0, n1, n2, n3;   // the cipher, as chacha20_blocks_to_lds takes it
    int C, H, W, A, chunk, rowbytes, lstride, nblk, M, lanes, groups, cplanes;
    int32_t bias;
    uint32_t off_ks, off_red, off_red_n;
};

// the four counts of nibble `sh` of the first `live` vertical counters as four uint8: byte k = the count of the nibble's bit k (nibble bit 3 is the first position)
__device__ __forceinline__ uint32_t lca_nibble_counts(const uint32_t (&c)[LCA_PLANES], int sh, int live) {
    uint32_t v = 0u;
#pragma unroll
    for (int p = 0; p < LCA_PLANES; ++p)
        if (p < live) v += ((((c[p] >> sh) & 15u) * 0x00204081u) & 0x01010101u) << p;   // the nibble at shifts 0, 7, 14, 21: bit k lands on bit 8 k
    return v;
}

template <int L, int P, bool WORDS>
__global__ __launch_bounds__(LCA_WG) void gsw_level_counts_align_kernel(LevelCountsAlignArgs s) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lca_lds[];
    constexpr int R = 1 + P, EPW = 32 / L, EPB = 8 / L;             // elements per word of the row, per byte
    const int tid = threadIdx.x, b = blockIdx.y;
    uint32_t* ks_words = (uint32_t*)(lca_lds + s.off_ks);
    uint8_t* red_x = lca_lds + s.off_red;
    uint8_t* red_n = lca_lds + s.off_red_n;
    const uint8_t* src[R];

#pragma unroll
    for (int q = 0; q < R; ++q) {                                   // ---- stage the 1 + P rows, generate the keystream
        const uint8_t* row = q == 0 ? s.signs + (int64_t)b * s.rowbytes : s.planes + ((int64_t)b * P + (q - 1)) * s.rowbytes;
        uint8_t* dst = lca_lds + q * s.lstride;
        if (((uintptr_t)row & 3u) == 0) {
            const int nw = s.rowbytes >> 2;
            for (int w = tid; w < nw; w += LCA_WG) ((uint32_t*)dst)[w] = ((const uint32_t*)row)[w];
            for (int j = 4 * nw + tid; j < s.rowbytes; j += LCA_WG) dst[j] = row[j];
        } else {
            for (int j = tid; j < s.rowbytes; j += LCA_WG) dst[j] = row[j];
        }
        src[q] = dst;
    }
    chacha20_blocks_to_lds(CipherRegs{s.k0, s.k1, s.k2, s.k3, s.k4, s.k5, s.k6, s.k7, s.n0, s.n1, s.n2, s.n3}, 0u, (uint32_t)s.nblk, ks_words);
    __syncthreads();

    const bool counting = tid < s.lanes;
    const int a0 = blockIdx.x * s.chunk;
    const int a1 = a0 + s.chunk < s.A ? a0 + s.chunk : s.A;
    for (int a = a0; a < a1; ++a) {
        const AlignMap m = align_map(s.aligns[3 * a], s.aligns[3 * a + 1], s.aligns[3 * a + 2], s.H, s.W);
        if constexpr (WORDS) {
            uint32_t cx[P][LCA_PLANES], cn[P][LCA_PLANES];
#pragma unroll
            for (int k = 0; k < P; ++k)
#pragma unroll
                for (int p = 0; p < LCA_PLANES; ++p) cx[k][p] = 0u, cn[k][p] = 0u;
            if (counting && m.ok) {
                const int nwords = s.rowbytes >> 2;
                for (int w = tid; w < nwords; w += s.lanes) {
                    uint32_t acc[R];
                    level_align_gather<L, R>(src, m, w * EPW, EPW, s.H, s.W, acc);
                    const uint32_t d = acc[0] ^ __builtin_bswap32(ks_words[w]);           // MSB first: bit 31 - q is position 32 w + q
#pragma unroll
                    for (int k = 0; k < P; ++k) {
                        uint32_t carry_x = acc[1 + k] & d, carry_n = acc[1 + k];
#pragma unroll
                        for (int p = 0; p < LCA_PLANES; ++p)
                            if (p < s.cplanes) {
                                const uint32_t tx = cx[k][p] & carry_x, tn = cn[k][p] & carry_n;
                                cx[k][p] ^= carry_x, cn[k][p] ^= carry_n;
                                carry_x = tx, carry_n = tn;
                            }
                    }
                }
            }
            if (counting) {                                         // positions 4 j .. 4 j + 3 of the lane's word -> uint16 4 j .. 4 j + 3 of its 32, in X' and in N'
                uint2* ox = (uint2*)(red_x + 64 * tid);
                uint2* on = (uint2*)(red_n + 64 * tid);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    uint32_t xl = 0u, xh = 0u, nl = 0u, nh = 0u;    // bytes (0, 2) and (1, 3) of the nibble's counts, widened to 16 bits and weighted: at most 15 x 127
#pragma unroll
                    for (int k = 0; k < P; ++k) {
                        const uint32_t vx = lca_nibble_counts(cx[k], 28 - 4 * j, s.cplanes), vn = lca_nibble_counts(cn[k], 28 - 4 * j, s.cplanes);
                        xl += (vx & 0x00FF00FFu) << k, xh += ((vx >> 8) & 0x00FF00FFu) << k;
                        nl += (vn & 0x00FF00FFu) << k, nh += ((vn >> 8) & 0x00FF00FFu) << k;
                    }
                    // byte 3 of the counts is the nibble's first position: (pos 0, pos 1) = (byte 3, byte 2), (pos 2, pos 3) = (byte 1, byte 0)
                    ox[j] = make_uint2((xh >> 16) | (xl & 0xFFFF0000u), (xh & 0xFFFFu) | (xl << 16));
                    on[j] = make_uint2((nh >> 16) | (nl & 0xFFFF0000u), (nh & 0xFFFFu) | (nl << 16));
                }
            }
        } else {
            uint32_t sx[8], sn[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) sx[i] = 0u, sn[i] = 0u;
            if (counting && m.ok) {
                const uint8_t* ks_bytes = (const uint8_t*)ks_words;
                for (int j = tid; j < s.rowbytes; j += s.lanes) {
                    uint32_t acc[R];
                    level_align_gather<L, R>(src, m, j * EPB, EPB, s.H, s.W, acc);
                    const uint32_t d = acc[0] ^ (uint32_t)ks_bytes[j];
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        uint32_t level = 0u;
#pragma unroll
                        for (int k = 0; k < P; ++k) level += ((acc[1 + k] >> (7 - i)) & 1u) << k;
                        sn[i] += level;
                        sx[i] += ((d >> (7 - i)) & 1u) ? level : 0u;
                    }
                }
            }
            if (counting) {
                *(uint4*)(red_x + 16 * tid) = make_uint4(sx[0] | (sx[1] << 16), sx[2] | (sx[3] << 16), sx[4] | (sx[5] << 16), sx[6] | (sx[7] << 16));
                *(uint4*)(red_n + 16 * tid) = make_uint4(sn[0] | (sn[1] << 16), sn[2] | (sn[3] << 16), sn[4] | (sn[5] << 16), sn[6] | (sn[7] << 16));
            }
        }
        __syncthreads();
        const int64_t at = ((int64_t)b * s.A + a) * s.M;
        for (int t = tid; t < s.M; t += LCA_WG) {                   // uint16 g M + t of a region is lane g units + (t's message unit), position t within the unit
            const uint16_t* col_x = (const uint16_t*)red_x + t;
            const uint16_t* col_n = (const uint16_t*)red_n + t;
            int32_t x = 0, n = 0;
            for (int g = 0; g < s.groups; ++g) x += col_x[g * s.M], n += col_n[g * s.M];
            s.score[at + t] = s.bias + 2 * x - n;
            if (s.wsum) s.wsum[at + t] = n;
        }
        __syncthreads();                                            // the next alignment writes the region again
    }
}

template <int L, int P>
int launch_level_counts_align(const LevelCountsAlignArgs& s, const LevelCountsAlignPlan& p, hipStream_t st) {
    void (*kernel)(LevelCountsAlignArgs) = p.words ? gsw_level_counts_align_kernel<L, P, true> : gsw_level_counts_align_kernel<L, P, false>;
    GSW_HIP(allow_dynamic_lds((const void*)kernel, p.lds));
    hipLaunchKernelGGL(kernel, dim3(p.grid_x, p.grid_y), dim3(LCA_WG), p.lds, st, s);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

}  // namespace

extern "C" {

int gsw_level_counts_align(const uint8_t* signs_dev, const uint8_t* planes_dev, int P, int B, int C, int H, int W, const int32_t* aligns_dev, int A,
                           const uint8_t key[32], const uint8_t nonce16[16], int msg_bits, int bias, int32_t* score_dev, int32_t* wsum_dev, void* stream) {
    const bool pointers_ok = signs_dev && planes_dev && aligns_dev && key && nonce16 && score_dev && ((uintptr_t)aligns_dev & 3u) == 0 &&
                             ((uintptr_t)score_dev & 3u) == 0 && ((uintptr_t)wsum_dev & 3u) == 0;
    const LevelCountsAlignPlan p = level_counts_align_decide(pointers_ok, P, B, C, H, W, A, msg_bits, bias);
    if (p.status != GSW_OK) return p.status;
    const auto le = [](const uint8_t* q) { return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24); };
    const LevelCountsAlignArgs s{signs_dev, planes_dev, aligns_dev, score_dev, wsum_dev,
                                 le(key), le(key + 4), le(key + 8), le(key + 12), le(key + 16), le(key + 20), le(key + 24), le(key + 28),
                                 le(nonce16), le(nonce16 + 4), le(nonce16 + 8), le(nonce16 + 12),
                                 C, H, W, A, p.chunk, p.rowbytes, p.lstride, p.nblk, msg_bits, p.lanes, p.groups, p.cplanes, bias,
                                 p.off_ks, p.off_red, p.off_red_n};
    switch (P) {
        case 1: return launch_level_counts_align<1, 1>(s, p, (hipStream_t)stream);
        case 2: return launch_level_counts_align<1, 2>(s, p, (hipStream_t)stream);
        case 3: return launch_level_counts_align<1, 3>(s, p, (hipStream_t)stream);
        default: return launch_level_counts_align<1, 4>(s, p, (hipStream_t)stream);
    }
}

}  // extern "C"
