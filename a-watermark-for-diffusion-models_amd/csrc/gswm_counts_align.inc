// gswm_counts_align.inc -- the vote counts of every candidate alignment of a packed quantised row under ONE key, in one launch (gfx950): the operand of a registry
// search over (record, alignment) pairs (gsw_trace_topk on the [B A, M] counts).  Included at the end of gswm_keyed.hip after gswm_align.inc: align_map and
// align_gather are that file's, GSW_HIP and allow_dynamic_lds gswm_host.h's, chacha20_blocks_to_lds gswm_chacha.h's.
//
//   counts[b, a, t] = #{ p < n_bits : p mod M == t and (bit p of gsw_rows_align's row (b, a)) ^ (keystream bit p) == 1 }
//
// bit p of a row is bit 7 - p % 8 of byte p / 8 (MSB first), the keystream is the first n_bits bits of ChaCha20 under (key, nonce16) as gsw_extract uses them.  The
// aligned rows are never written: 4 M bytes leave the chip per (image, alignment) instead of n_bits / 8, and the vote that would read them back is gone.
//
// Work split.  Grid (alignment chunks, images), 256 lanes.  A workgroup stages its image's row in LDS and generates the keystream into LDS, both once (neither depends
// on the alignment), then walks its chunk.  Per alignment, on the word path (M % 32 == 0): a lane assembles whole 32-bit words of the aligned row (align_gather),
// XORs the keystream word and adds the 32 decrypted bits to seven bit-sliced vertical counters (three operations per plane and word).  Lane `tid` only ever sees
// message word tid % (M / 32) (gswm_counts_align_plan.h), so its 32 counters are 32 adjacent message positions; it leaves them as 32 uint8 in the reduction region and
// after a barrier lane t sums column t over the lanes that share its message word and stores one dword: the M stores are coalesced, there is no atomic.  The byte path
// (any other M % 8 == 0) is the same with bytes, eight int32 counters and uint16 in LDS.
//
// An entry with d outside 0..7, or an odd d on a non-square lattice, has no map: its M counts are written as zeros, nothing is read through it.
//
// Kernel
//   gsw_counts_align_kernel<L, WORDS> : L bits per element (1, 2, 4); WORDS: the word path

namespace {

struct CountsAlignArgs {
    const uint8_t* rows;      // [B, rowbytes]
    const int32_t* aligns;    // [A, 3]
    int32_t* counts;          // [B, A, M]
    uint32_t k0, k1, k2, k3, k4, k5, k6, k7, n0, n1, n2, n3;   // the cipher, as chacha20_blocks_to_lds takes it
    int C, H, W, A, chunk, rowbytes, nblk, M, units, lanes, groups;
    uint32_t off_ks, off_red;
};

// the four counts of nibble `sh` of seven vertical counters as four uint8: byte k = the count of the nibble's bit k (nibble bit 3 is the first position)
__device__ __forceinline__ uint32_t ca_nibble_counts(const uint32_t (&c)[CA_PLANES], int sh) {
    uint32_t v = 0u;
#pragma unroll
    for (int p = 0; p < CA_PLANES; ++p) v += ((((c[p] >> sh) & 15u) * 0x00204081u) & 0x01010101u) << p;   // the nibble at shifts 0, 7, 14, 21: bit k lands on bit 8 k
    return v;
}

template <int L, bool WORDS>
__global__ __launch_bounds__(CA_WG) void gsw_counts_align_kernel(CountsAlignArgs s) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ca_lds[];
    const int tid = threadIdx.x, b = blockIdx.y;
    const uint8_t* row = s.rows + (int64_t)b * s.rowbytes;
    constexpr int EPW = 32 / L, EPB = 8 / L;                        // elements per word, per byte
    uint32_t* ks_words = (uint32_t*)(ca_lds + s.off_ks);
    uint8_t* red = ca_lds + s.off_red;

    if (((uintptr_t)row & 3u) == 0) {                               // ---- stage the row, generate the keystream
        const int nw = s.rowbytes >> 2;
        for (int w = tid; w < nw; w += CA_WG) ((uint32_t*)ca_lds)[w] = ((const uint32_t*)row)[w];
        for (int j = 4 * nw + tid; j < s.rowbytes; j += CA_WG) ca_lds[j] = row[j];
    } else {
        for (int j = tid; j < s.rowbytes; j += CA_WG) ca_lds[j] = row[j];
    }
    chacha20_blocks_to_lds(CipherRegs{s.k0, s.k1, s.k2, s.k3, s.k4, s.k5, s.k6, s.k7, s.n0, s.n1, s.n2, s.n3}, 0u, (uint32_t)s.nblk, ks_words);
    __syncthreads();

    const bool counting = tid < s.lanes;
    const int a0 = blockIdx.x * s.chunk;
    const int a1 = a0 + s.chunk < s.A ? a0 + s.chunk : s.A;
    for (int a = a0; a < a1; ++a) {
        const AlignMap m = align_map(s.aligns[3 * a], s.aligns[3 * a + 1], s.aligns[3 * a + 2], s.H, s.W);
        if constexpr (WORDS) {
            uint32_t c[CA_PLANES];
#pragma unroll
            for (int p = 0; p < CA_PLANES; ++p) c[p] = 0u;
            if (counting && m.ok) {
                const int nwords = s.rowbytes >> 2;
                for (int w = tid; w < nwords; w += s.lanes) {
                    uint32_t carry = align_gather<L>((const uint8_t*)ca_lds, m, w * EPW, EPW, s.H, s.W) ^ __builtin_bswap32(ks_words[w]);   // MSB first: bit 31 - q is position 32 w + q
#pragma unroll
                    for (int p = 0; p < CA_PLANES; ++p) {
                        const uint32_t t = c[p] & carry;
                        c[p] ^= carry;
                        carry = t;
                    }
                }
            }
            if (counting) {                                         // position q of the lane's word -> byte q ^ 3 of its 32
                uint4* o = (uint4*)(red + 32 * tid);
                o[0] = make_uint4(ca_nibble_counts(c, 28), ca_nibble_counts(c, 24), ca_nibble_counts(c, 20), ca_nibble_counts(c, 16));
                o[1] = make_uint4(ca_nibble_counts(c, 12), ca_nibble_counts(c, 8), ca_nibble_counts(c, 4), ca_nibble_counts(c, 0));
            }
        } else {
            uint32_t c[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) c[i] = 0u;
            if (counting && m.ok) {
                const uint8_t* ks_bytes = (const uint8_t*)ks_words;
                for (int j = tid; j < s.rowbytes; j += s.lanes) {
                    const uint32_t x = align_gather<L>((const uint8_t*)ca_lds, m, j * EPB, EPB, s.H, s.W) ^ (uint32_t)ks_bytes[j];
#pragma unroll
                    for (int i = 0; i < 8; ++i) c[i] += (x >> (7 - i)) & 1u;
                }
            }
            if (counting)
                *(uint4*)(red + 16 * tid) = make_uint4(c[0] | (c[1] << 16), c[2] | (c[3] << 16), c[4] | (c[5] << 16), c[6] | (c[7] << 16));
        }
        __syncthreads();
        int32_t* out = s.counts + ((int64_t)b * s.A + a) * s.M;
        for (int t = tid; t < s.M; t += CA_WG) {
            uint32_t sum = 0u;
            if constexpr (WORDS) {
                const uint8_t* col = red + (t ^ 3);
                for (int g = 0; g < s.groups; ++g) sum += col[g * s.M];
            } else {
                const uint16_t* col = (const uint16_t*)red + t;
                for (int g = 0; g < s.groups; ++g) sum += col[g * s.M];
            }
            out[t] = (int32_t)sum;
        }
        __syncthreads();                                            // the next alignment writes the region again
    }
}

template <int L>
int launch_counts_align(const CountsAlignArgs& s, const CountsAlignPlan& p, hipStream_t st) {
    void (*kernel)(CountsAlignArgs) = p.words ? gsw_counts_align_kernel<L, true> : gsw_counts_align_kernel<L, false>;
    GSW_HIP(allow_dynamic_lds((const void*)kernel, p.lds));
    hipLaunchKernelGGL(kernel, dim3(p.grid_x, p.grid_y), dim3(CA_WG), p.lds, st, s);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

}  // namespace

extern "C" {

int gsw_counts_align(const uint8_t* rows_dev, int B, int C, int H, int W, int l, const int32_t* aligns_dev, int A, const uint8_t key[32],
                     const uint8_t nonce16[16], int msg_bits, int32_t* counts_dev, void* stream) {
    const bool pointers_ok = rows_dev && aligns_dev && key && nonce16 && counts_dev && ((uintptr_t)aligns_dev & 3u) == 0 && ((uintptr_t)counts_dev & 3u) == 0;
    const CountsAlignPlan p = counts_align_decide(pointers_ok, B, C, H, W, l, A, msg_bits);
    if (p.status != GSW_OK) return p.status;
    const auto le = [](const uint8_t* q) { return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24); };
    const CountsAlignArgs s{rows_dev, aligns_dev, counts_dev,
                            le(key), le(key + 4), le(key + 8), le(key + 12), le(key + 16), le(key + 20), le(key + 24), le(key + 28),
                            le(nonce16), le(nonce16 + 4), le(nonce16 + 8), le(nonce16 + 12),
                            C, H, W, A, p.chunk, p.rowbytes, p.nblk, msg_bits, p.units, p.lanes, p.groups, p.off_ks, p.off_red};
    switch (l) {
        case 1: return launch_counts_align<1>(s, p, (hipStream_t)stream);
        case 2: return launch_counts_align<2>(s, p, (hipStream_t)stream);
        default: return launch_counts_align<4>(s, p, (hipStream_t)stream);
    }
}

}  // extern "C"
