// gswm_codec_keyed.inc -- the codec with one record per image: embed and extract B images, each under its own key, nonce and
// message, in one launch each (gfx950).  Included at the end of gswm_kernels.hip, after gswm_codec_l.inc: the per-element arithmetic is
// the shared-key kernels' own (embed_quad / codec_l::embed_quad_l, SrcPlain::byte8 / codec_l::quant_group8), so row b of either result
// is bit for bit what gsw_embed[_l] / gsw_extract[_l] give for that one image under record b.
//
// Records (gsw_trace_keyed_topk's rows): uint8 [B, stride], 16-byte aligned, stride % 16 == 0, a row is key[32] | nonce16[16] |
// msg[msg_bytes] (gswm_record.h: layout, operand check, the repeated message, the vote tail).  Key, nonce and message words are read
// from the row with ordinary vector loads by the lanes that need them; the block function is gswm_chacha.h's chacha20_block.
//
// Cipher bits of image b: the keystream of record b (initial counter nonce16[0:8] as a 64-bit little-endian number, so the 32-bit
// counter carries into the next word, as gsw_keystream) XOR the message repeated floor(Nb / (8 msg_bytes)) times, then zeros.  Cipher
// byte g of the image therefore takes msg[g % msg_bytes] iff 8 g < lim, lim = floor(Nb / msg_bits) msg_bits (a multiple of 8).
//
// Embed.  grid = (chunks, image groups).  A workgroup owns one 2048-element chunk of a GROUP of G consecutive images, G <= 16 / l: its
// 64 quads compute the G x 4 l ChaCha blocks of the group in one pass (quad q: image q / (4 l) of the group, block q % (4 l) of the
// chunk), XOR the message into their own four words while these are still in registers, and leave G x 256 l cipher bytes in LDS
// (4 KiB at G = 16 / l).  After one barrier every lane walks the G images with the shared-key kernels' per-element loop (thread t owns
// elements chunk * 2048 + r * 1024 + 4 t .. + 3, r = 0, 1: one 16-byte fp32 store each).  G only decides which workgroup computes an
// image, never what is computed.
//
// Extract.  One workgroup per image.  The quads write the image's keystream to LDS; a thread quantises eight elements into l bytes
// and XORs them into the row in place; S adjacent lanes (gsw_vote_tiled's choice) count the ones of a message bit over its copies and
// meet by __shfl_xor; the bytes of the message come from the wave's ballot.  Flags and matches are reduced through LDS slots, one
// writer each: no atomics, no workspace, nothing to zero first.
//
// Kernels
//   gsw_embed_keyed_kernel<OutT, L, HAS_U, FAST>   : (chunks, min(groups, 65535)) workgroups of 256
//   gsw_extract_keyed_kernel<T, L>                 : [B] workgroups of 256, ceil(Nb / 512) x 64 bytes of dynamic LDS
//
// A NaN element (its image is flagged GSW_FLAG_NAN, the reference raises for it) votes as gsw_extract[_l] counts it for the same geometry:
// as 0, except at l = 1 where gsw_extract takes its wave vote, which goes by the sign bit (nan_ones8).

namespace codec_keyed {

struct EmbedKeyedArgs {
    const uint8_t* records; // [B][stride]
    const double* u;        // [B][N] or nullptr
    void* out;              // [B][N]
    uint64_t seed, image_index0;
    uint32_t stride;
    uint32_t n_elems;       // N
    uint32_t msg_bytes;
    uint32_t lim_bits;      // floor(Nb / msg_bits) * msg_bits
    int32_t B;
    int32_t G;              // images per group, 1 .. 16 / l
    int32_t ngroups;        // ceil(B / G)
};

template <typename OutT, int L, bool HAS_U, bool FAST>
__global__ __launch_bounds__(GSW_WG) void gsw_embed_keyed_kernel(EmbedKeyedArgs p) {
    constexpr uint32_t BLKS = 4u * L;              // ChaCha blocks of a chunk
    constexpr uint32_t CW = 16u * BLKS;            // cipher words of a chunk, one image
    constexpr bool TABLE = (L == 1) && FAST && !HAS_U;
    __shared__ uint32_t cw_words[1024];            // [G][CW], G <= 16 / l
    __shared__ float4 icdf[TABLE ? GSW_ICDF_ENTRIES : 1];
    __shared__ typename codec_l::BinOf<OutT>::V bins[1u << L];
    const uint32_t tid = threadIdx.x, col = tid & 3u;
    if constexpr (TABLE)
        for (uint32_t i = tid; i < GSW_ICDF_ENTRIES; i += GSW_WG) icdf[i] = GSW_ICDF_TABLE[i];
    if constexpr (L > 1)
        if (tid < (1u << L)) bins[tid] = codec_l::bin_entry<L, OutT>(tid);
    const uint32_t chunk = (blockIdx.x + blockIdx.y) % gridDim.x;   // the shared-key kernels' XCD rotation
    const uint32_t N = p.n_elems;
    const uint32_t e_chunk = chunk * GSW_CHUNK;
    const uint32_t cbytes = (min(GSW_CHUNK, N - e_chunk) * L + 7u) >> 3;
    const uint32_t nblk = (cbytes + 63u) >> 6;
    const uint32_t q_img = (tid >> 2) / BLKS, q_blk = (tid >> 2) % BLKS;
    const uint32_t k0 = (uint32_t)p.seed, k1 = (uint32_t)(p.seed >> 32);

    for (int grp = blockIdx.y; grp < p.ngroups; grp += gridDim.y) {
        const int b0 = grp * p.G;
        const uint32_t gcount = (uint32_t)min(p.G, p.B - b0);
        if (q_img < gcount && q_blk < nblk) {      // the same for the four lanes of a quad
            const uint8_t* rec = p.records + (int64_t)(b0 + (int)q_img) * p.stride;
            uint32_t ks[4];
            chacha20_block(cipher_lane_of_record(reinterpret_cast<const uint32_t*>(rec), col), (uint64_t)chunk * BLKS + q_blk, col, ks);
            const uint8_t* msg = rec + GSW_REC_HEAD;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t g0 = chunk * (64u * BLKS) + 64u * q_blk + 16u * r + 4u * col;   // cipher byte of the image, < 2^28
                // the message ends with its last whole copy: byte g takes it iff 8 g < lim_bits, and lim_bits (whole copies of whole
                // bytes) is a multiple of 8, so the bytes g0 + i < lim_bits / 8 are the first lim_bits / 8 - g0 of the word
                const uint32_t m = repeated_msg_word(msg, g0 % p.msg_bytes, p.msg_bytes, false, (int)(p.lim_bits >> 3) - (int)g0);
                cw_words[q_img * CW + q_blk * 16u + 4u * r + col] = ks[r] ^ m;
            }
        }
        __syncthreads();
        for (uint32_t gi = 0; gi < gcount; ++gi) {
            const int b = b0 + (int)gi;
            const uint64_t img = p.image_index0 + (uint64_t)b;
            const uint8_t* cb = reinterpret_cast<const uint8_t*>(cw_words + gi * CW);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const uint32_t el = r * 1024u + 4u * tid;
                const uint32_t e = e_chunk + el;
                if (e >= N) continue;
                const size_t off = (size_t)b * N + e;
                OutT* dst = reinterpret_cast<OutT*>(p.out) + off;
                if constexpr (L == 1) {
                    const uint32_t byte = cb[el >> 3];
                    const uint32_t ynib = (tid & 1u) ? (byte & 0xFu) : (byte >> 4);
                    embed_quad<OutT, HAS_U, FAST>(dst, p.u + off, e, img, k0, k1, ynib, icdf);
                } else {
                    uint32_t yw = 0;
#pragma unroll
                    for (int i = 0; i < L / 2; ++i) yw = (yw << 8) | cb[((el * L) >> 3) + i];
                    codec_l::embed_quad_l<OutT, L, HAS_U, FAST>(dst, p.u + off, e, img, k0, k1, yw, bins);
                }
            }
        }
        __syncthreads();                           // the next group overwrites the cipher bytes
    }
}

struct ExtractKeyedArgs {
    const void* z;          // [B][N]
    const uint8_t* records; // [B][stride]
    uint8_t* bits;          // [B][msg_bytes]
    uint32_t* counts;       // [B][msg_bits] or nullptr
    uint32_t* flags;        // [B]
    uint32_t* matches;      // [B] or nullptr
    uint32_t stride;
    uint32_t n_elems;       // N
    uint32_t msg_bytes;
    uint32_t nblk;          // ChaCha blocks that cover the staged row
    uint32_t copies;        // Nb / msg_bits
    uint32_t log2s;         // lanes per message bit
    uint32_t nan_by_sign;   // l = 1: gsw_extract takes the wave vote for this geometry, which counts a NaN by its sign bit
    Thr thr;                // l = 1 quantiser
};

// l = 1, the elements of a group that gsw_extract's wave vote counts as 1 although they are NaN (byte8 packs every NaN as 0): the NaNs whose
// sign bit is clear, for fp64 every NaN (its fp32 surrogate is a positive NaN).  Only reached in a group that raised GSW_FLAG_NAN.
template <typename T>
__device__ __forceinline__ uint32_t nan_ones8(const T* __restrict__ p) {
    uint32_t m = 0;
#pragma unroll 1
    for (int k = 0; k < 8; ++k) {
        if constexpr (std::is_same<T, double>::value) {
            const double v = p[k];
            if (v != v) m |= 0x80u >> k;
        } else {
            const float v = Load8<T>::ld1(p + k);
            if (v != v && !(__float_as_uint(v) >> 31)) m |= 0x80u >> k;
        }
    }
    return m;
}

template <typename T, int L>
__global__ __launch_bounds__(GSW_WG) void gsw_extract_keyed_kernel(ExtractKeyedArgs p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];   // the row: keystream, then decrypted bits, p.nblk * 16 words
    __shared__ uint32_t s_flags[GSW_WG / 64];
    __shared__ uint32_t s_match[GSW_MSG_INLINE_MAX];                 // matching bits per message byte
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t b = blockIdx.x;
    const uint32_t N = p.n_elems, M = p.msg_bytes * 8u;
    const uint8_t* rec = p.records + (int64_t)b * p.stride;
    uint8_t* row = reinterpret_cast<uint8_t*>(lds);

    record_keystream_to_lds<GSW_WG>(rec, p.nblk, lds);
    __syncthreads();

    const size_t base = (size_t)b * N;
    uint32_t flags = 0;
    if constexpr (L == 1) {
        const SrcPlain<T> src{reinterpret_cast<const T*>(p.z)};
        for (uint32_t j = tid; j < (N >> 3); j += GSW_WG) {         // N % 8 == 0: whole, 16-byte aligned groups
            const size_t off = base + ((size_t)j << 3);
            uint32_t f = 0;
            uint32_t c = src.byte8(off, p.thr, f);
            if ((f & GSW_FLAG_NAN) && p.nan_by_sign) c |= nan_ones8<T>(src.z + off);
            flags |= f;
            row[j] ^= (uint8_t)c;
        }
    } else {
        const T* z = reinterpret_cast<const T*>(p.z);
        const uint32_t ngroups = (N + 7u) >> 3;
        for (uint32_t g = tid; g < ngroups; g += GSW_WG) {
            const uint32_t bits = codec_l::quant_group8<T, L>(z, base, g << 3, N, flags);
            if constexpr (L == 2) reinterpret_cast<uint16_t*>(lds)[g] ^= (uint16_t)(((bits >> 8) & 0xFFu) | ((bits & 0xFFu) << 8));   // first byte at the lower address
            else lds[g] ^= __builtin_bswap32(bits);
        }
    }
    for (int s = 32; s > 0; s >>= 1) flags |= __shfl_xor(flags, s, 64);
    if (lane == 0) s_flags[tid >> 6] = flags;
    __syncthreads();

    const uint32_t S = 1u << p.log2s, s = tid & (S - 1u);
    const uint32_t per_pass = GSW_WG >> p.log2s;                     // message bits per pass of the workgroup, a multiple of 8 per wave
    for (uint32_t t0 = 0; t0 < M; t0 += per_pass) {                  // the same trip count for every lane: the shuffles run with all lanes on
        const uint32_t t = t0 + (tid >> p.log2s);
        uint32_t c1 = 0;
        if (t < M) {
            for (uint32_t k = s; k < p.copies; k += S) {
                const uint32_t j = k * M + t;                        // < Nb <= 2^20
                c1 += (row[j >> 3] >> (7u - (j & 7u))) & 1u;
            }
        }
        for (uint32_t step = 1; step < S; step <<= 1) c1 += __shfl_xor(c1, (int)step, 64);
        const bool one = t < M && 2u * c1 > p.copies;                // strict majority, ties -> 0
        const uint64_t ball = __ballot(one);                         // bit (i S) of the wave's ballot: message bit (t of lane 0) + i
        if (t < M && s == 0) {
            if (p.counts) p.counts[(size_t)b * M + t] = c1;
            if ((t & 7u) == 0) {                                     // the seven bits after t are this wave's as well
                const uint32_t v = ballot_byte(ball, lane, p.log2s);
                p.bits[(size_t)b * p.msg_bytes + (t >> 3)] = (uint8_t)v;
                s_match[t >> 3] = 8u - __popc(v ^ (uint32_t)rec[GSW_REC_HEAD + (t >> 3)]);
            }
        }
    }
    __syncthreads();
    store_matches_flags<GSW_WG / 64>(s_match, s_flags, p.msg_bytes, p.matches, p.flags, b);
}

template <typename OutT, int L>
static void launch_embed(const EmbedKeyedArgs& a, bool has_u, bool fast, dim3 grid, hipStream_t st) {
    if (has_u) {
        if (fast) hipLaunchKernelGGL((gsw_embed_keyed_kernel<OutT, L, true, true>), grid, dim3(GSW_WG), 0, st, a);
        else hipLaunchKernelGGL((gsw_embed_keyed_kernel<OutT, L, true, false>), grid, dim3(GSW_WG), 0, st, a);
    } else {
        if (fast) hipLaunchKernelGGL((gsw_embed_keyed_kernel<OutT, L, false, true>), grid, dim3(GSW_WG), 0, st, a);
        else hipLaunchKernelGGL((gsw_embed_keyed_kernel<OutT, L, false, false>), grid, dim3(GSW_WG), 0, st, a);
    }
}

template <int L>
static void launch_embed_dtype(const EmbedKeyedArgs& a, int out_dtype, bool has_u, bool fast, dim3 grid, hipStream_t st) {
    switch (out_dtype) {
        case GSW_F32: launch_embed<float, L>(a, has_u, fast, grid, st); break;
        case GSW_F16: launch_embed<__half, L>(a, has_u, fast, grid, st); break;
        case GSW_BF16: launch_embed<__hip_bfloat16, L>(a, has_u, fast, grid, st); break;
        default: launch_embed<double, L>(a, has_u, fast, grid, st); break;
    }
}

template <typename T, int L>
static int launch_extract(const ExtractKeyedArgs& a, int B, hipStream_t st) {
    const uint32_t lds = a.nblk * 64u;
    GSW_HIP(allow_dynamic_lds((const void*)gsw_extract_keyed_kernel<T, L>, lds));
    hipLaunchKernelGGL((gsw_extract_keyed_kernel<T, L>), dim3((uint32_t)B), dim3(GSW_WG), lds, st, a);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

template <int L>
static int launch_extract_dtype(const ExtractKeyedArgs& a, int dtype, int B, hipStream_t st) {
    switch (dtype) {
        case GSW_F32: return launch_extract<float, L>(a, B, st);
        case GSW_F16: return launch_extract<__half, L>(a, B, st);
        case GSW_BF16: return launch_extract<__hip_bfloat16, L>(a, B, st);
        default: return launch_extract<double, L>(a, B, st);
    }
}

}  // namespace codec_keyed

int gsw_embed_keyed(const uint8_t* records_dev, int64_t record_stride, int msg_bytes, const double* u_dev, uint64_t seed,
                    uint64_t image_index0, void* out_dev, int out_dtype, int B, int64_t n_elems, uint32_t flags, int l, void* stream) {
    const int rc = records_check32(records_dev, record_stride, msg_bytes, B);
    if (rc != GSW_OK) return rc;
    if (!out_dev || n_elems <= 0 || (n_elems & 3)) return GSW_ERR_BAD_ARG;
    if (out_dtype < GSW_F32 || out_dtype > GSW_F64) return GSW_ERR_BAD_ARG;
    if (((uintptr_t)out_dev & 15u) || ((uintptr_t)u_dev & 15u)) return GSW_ERR_BAD_ARG;      // 16-byte stores and loads
    const int wc = codec_l::window_check(l, n_elems);
    if (wc != GSW_OK) return wc;
    if (n_elems > (int64_t)0x7FFFFFF0) return GSW_ERR_UNSUPPORTED;
    codec_keyed::EmbedKeyedArgs a;
    memset(&a, 0, sizeof(a));
    const int64_t nbits = n_elems * l, msg_bits = (int64_t)msg_bytes * 8;
    a.records = records_dev;
    a.u = u_dev;
    a.out = out_dev;
    a.seed = seed;
    a.image_index0 = image_index0;
    a.stride = (uint32_t)record_stride;
    a.n_elems = (uint32_t)n_elems;
    a.msg_bytes = (uint32_t)msg_bytes;
    a.lim_bits = (uint32_t)((nbits / msg_bits) * msg_bits);
    a.B = B;
    // images per workgroup: as many as one ChaCha pass of the 64 quads covers (16 / l), halved while the grid would leave the chip short
    // of four workgroups per CU -- a small batch spreads over the chip instead of amortising a pass it cannot fill
    const int64_t nchunks = (n_elems + GSW_CHUNK - 1) / GSW_CHUNK;
    int G = 16 / l;
    while (G > 1 && nchunks * (((int64_t)B + G - 1) / G) < (int64_t)device_cus() * 4) G >>= 1;
    a.G = G;
    a.ngroups = (B + G - 1) / G;
    const dim3 grid((uint32_t)nchunks, (uint32_t)std::min(a.ngroups, 65535));
    hipStream_t st = (hipStream_t)stream;
    const bool fast = (flags & GSW_EMBED_FAST_F32) != 0;
    if (l == 1) codec_keyed::launch_embed_dtype<1>(a, out_dtype, u_dev != nullptr, fast, grid, st);
    else if (l == 2) codec_keyed::launch_embed_dtype<2>(a, out_dtype, u_dev != nullptr, fast, grid, st);
    else codec_keyed::launch_embed_dtype<4>(a, out_dtype, u_dev != nullptr, fast, grid, st);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

int gsw_extract_keyed(const void* z_dev, int z_dtype, const uint8_t* records_dev, int64_t record_stride, int msg_bytes, uint8_t* bits_dev,
                      uint32_t* counts_dev, uint32_t* flags_dev, uint32_t* matches_dev, int B, int64_t n_elems, int l, void* stream) {
    const int rc = records_check32(records_dev, record_stride, msg_bytes, B);
    if (rc != GSW_OK) return rc;
    if (!z_dev || !bits_dev || !flags_dev || n_elems <= 0) return GSW_ERR_BAD_ARG;
    if (z_dtype < GSW_F32 || z_dtype > GSW_F64) return GSW_ERR_BAD_ARG;
    if ((uintptr_t)z_dev & 15u) return GSW_ERR_BAD_ARG;                                      // 16-byte loads
    if (l != 1 && l != 2 && l != 4) return GSW_ERR_UNSUPPORTED;
    if (n_elems > GSW_ROW_MAX_BITS) return GSW_ERR_UNSUPPORTED;
    const int64_t nbits = n_elems * l, msg_bits = (int64_t)msg_bytes * 8;
    if (nbits % 8 || nbits > GSW_ROW_MAX_BITS) return GSW_ERR_UNSUPPORTED;
    if (nbits % msg_bits) return GSW_ERR_RAGGED;
    codec_keyed::ExtractKeyedArgs a;
    memset(&a, 0, sizeof(a));
    a.z = z_dev;
    a.records = records_dev;
    a.bits = bits_dev;
    a.counts = counts_dev;
    a.flags = flags_dev;
    a.matches = matches_dev;
    a.stride = (uint32_t)record_stride;
    a.n_elems = (uint32_t)n_elems;
    a.msg_bytes = (uint32_t)msg_bytes;
    a.nblk = (uint32_t)((((n_elems + 7) / 8) * l + 63) / 64);      // whole groups of eight elements are staged
    a.copies = (uint32_t)(nbits / msg_bits);
    a.log2s = (uint32_t)vote_log2s(msg_bits, a.copies, GSW_WG);
    a.thr = make_thr(z_dtype);
    a.nan_by_sign = l == 1 && extract_votes_by_wave((uint32_t)n_elems, (uint32_t)msg_bits);
    hipStream_t st = (hipStream_t)stream;
    if (l == 1) return codec_keyed::launch_extract_dtype<1>(a, z_dtype, B, st);
    if (l == 2) return codec_keyed::launch_extract_dtype<2>(a, z_dtype, B, st);
    return codec_keyed::launch_extract_dtype<4>(a, z_dtype, B, st);
}
