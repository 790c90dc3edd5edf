// gswm_codec_l.inc -- the codec with multi-bit windows (l = 2, 4): embed, extract and quantise-and-pack, gfx950.
// Included at the end of gswm_kernels.hip (same translation unit: ChaCha20, Philox, both ndtri cores, the vector loads and stores and
// the host helpers are the l = 1 kernels' own); nothing above this line changes, l = 1 keeps its entry points and kernels.
//
// Semantics (DESIGN.md, "Multi-bit windows"; the reference's own l > 1 path does not run, extract.py:84-86 / gs_insert.py:23,58-66):
//   Nb = n_elems * l cipher bits per image = keystream XOR the message repeated over Nb bits, MSB-first within each byte
//   element i takes bits [i l, i l + l), first bit = MSB of y_i;  z_i = ndtri((u_i + y_i) / 2^l)
//   stored value = the representable value of the output dtype nearest to z_i that still quantises to y_i (bin-safe rounding)
//   quantise: y = int(ndtr(float64(z)) * 2^l) = #{j : z >= T_j}, T from quant_thresholds.inc; z >= GSW_QT_SAT: all ones + SATURATED;
//   NaN: zeros + NAN
//   extract: the y of an image as Nb bits, XOR keystream, strict-majority vote over Nb / msg_bits copies (ties -> 0)
//
// Index algebra: element e owns cipher byte (e l) >> 3, bits 8 - l - ((e l) & 7) .. +l-1; l in {2, 4} never straddles a byte.  Four
// consecutive elements are l / 2 whole bytes, eight are l bytes.

#include "quant_thresholds.inc"

namespace codec_l {

// ---- thresholds as compile-time constants: a binary search whose next threshold is a select tree over the bits already decided
template <int L, typename F>
__device__ __forceinline__ constexpr F qthr(int j) {
    if constexpr (L == 2) {
        if constexpr (std::is_same<F, double>::value) return GSW_QT_D_L2[j]; else return GSW_QT_F_L2[j];
    } else {
        if constexpr (std::is_same<F, double>::value) return GSW_QT_D_L4[j]; else return GSW_QT_F_L4[j];
    }
}

// threshold of candidate BASE' + S, where BASE' are the bits of y above S (examined from BIT downwards)
template <int L, int S, int BIT, int BASE, typename F>
__device__ __forceinline__ F pick_thr(uint32_t y) {
    if constexpr (BIT == S) return qthr<L, F>(BASE + S - 1);
    else return (y & BIT) ? pick_thr<L, S, BIT / 2, BASE + BIT, F>(y) : pick_thr<L, S, BIT / 2, BASE, F>(y);
}

template <int L, int S, typename F>
__device__ __forceinline__ void quant_levels(F z, uint32_t& y) {
    if constexpr (S >= 1) {
        if (z >= pick_thr<L, S, (1 << (L - 1)), 0, F>(y)) y |= S;     // false for NaN at every level: y == 0
        quant_levels<L, S / 2, F>(z, y);
    }
}

template <int L, typename F>
__device__ __forceinline__ uint32_t quant1(F z, uint32_t& flags) {
    uint32_t y = 0;
    quant_levels<L, (1 << (L - 1)), F>(z, y);
    if constexpr (std::is_same<F, double>::value) { if (z >= GSW_QT_SAT_D) flags |= GSW_FLAG_SATURATED; }
    else { if (z >= GSW_QT_SAT_F) flags |= GSW_FLAG_SATURATED; }
    if (z != z) flags |= GSW_FLAG_NAN;
    return y;
}

// ---- eight consecutive elements in the compare type (fp32 for fp16 / bf16 / fp32 inputs, fp64 for fp64)
template <typename T> struct QLoad {
    typedef float F;
    static __device__ __forceinline__ void ld8(const T* p, float (&v)[8]) { Load8<T>::ld(p, v); }
    static __device__ __forceinline__ float ld1(const T* p) { return Load8<T>::ld1(p); }
};
template <> struct QLoad<double> {
    typedef double F;
    static __device__ __forceinline__ void ld8(const double* p, double (&v)[8]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { const double2 a = reinterpret_cast<const double2*>(p)[i]; v[2 * i] = a.x; v[2 * i + 1] = a.y; }
    }
    static __device__ __forceinline__ double ld1(const double* p) { return *p; }
};

// The 8 l window bits of elements e .. e+7 of the image at `base`, first element in the top bits.  Elements at or past n read as
// -100 (y = 0, no flag): they belong to bytes past the lattice, which nobody uses.
template <typename T, int L>
__device__ __forceinline__ uint32_t quant_group8(const T* __restrict__ z, size_t base, uint32_t e, uint32_t n, uint32_t& flags) {
    typedef typename QLoad<T>::F F;
    F v[8];
    const uint32_t cnt = min(8u, n - e);
    if (cnt == 8u && ((base + e) & 7u) == 0) {
        QLoad<T>::ld8(z + base + e, v);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = (uint32_t)k < cnt ? QLoad<T>::ld1(z + base + e + k) : (F)-100.0f;
    }
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) bits |= quant1<L, F>(v[k], flags) << (L * (7 - k));
    return bits;
}

__device__ __forceinline__ void or_image_flags(uint32_t flags, uint32_t* dst) {
    if (__any(flags != 0)) {
        uint32_t f = flags;
        for (int s = 32; s > 0; s >>= 1) f |= __shfl_xor(f, s, 64);
        if ((threadIdx.x & 63u) == 0) atomicOr(dst, f);
    }
}

// ------------------------------------------------------------------------------------------------
// Embed.  The l = 1 kernel's geometry: one workgroup = one 2048-element chunk (2048 l cipher bits = 4 l ChaCha blocks in LDS) looped
// over a strided set of images; thread t owns elements chunk*2048 + r*1024 + 4t .. +3 (r = 0, 1), whose window bits (l / 2 whole
// bytes) are computed once and reused for every image.  p.lim_elems counts BITS here: the message repeats over the first lim bits.
// ------------------------------------------------------------------------------------------------
template <typename OutT> struct BinOf { typedef float F; typedef float2 V; };
template <> struct BinOf<double> { typedef double F; typedef double2 V; };

template <int L, typename OutT>
__device__ __forceinline__ typename BinOf<OutT>::V bin_entry(uint32_t y) {
    typedef typename BinOf<OutT>::V V;
    if constexpr (L == 2) {
        if constexpr (std::is_same<OutT, double>::value) return V{GSW_QT_BIN_F64_L2[y][0], GSW_QT_BIN_F64_L2[y][1]};
        else if constexpr (std::is_same<OutT, __half>::value) return V{GSW_QT_BIN_F16_L2[y][0], GSW_QT_BIN_F16_L2[y][1]};
        else if constexpr (std::is_same<OutT, __hip_bfloat16>::value) return V{GSW_QT_BIN_BF16_L2[y][0], GSW_QT_BIN_BF16_L2[y][1]};
        else return V{GSW_QT_BIN_F32_L2[y][0], GSW_QT_BIN_F32_L2[y][1]};
    } else {
        if constexpr (std::is_same<OutT, double>::value) return V{GSW_QT_BIN_F64_L4[y][0], GSW_QT_BIN_F64_L4[y][1]};
        else if constexpr (std::is_same<OutT, __half>::value) return V{GSW_QT_BIN_F16_L4[y][0], GSW_QT_BIN_F16_L4[y][1]};
        else if constexpr (std::is_same<OutT, __hip_bfloat16>::value) return V{GSW_QT_BIN_BF16_L4[y][0], GSW_QT_BIN_BF16_L4[y][1]};
        else return V{GSW_QT_BIN_F32_L4[y][0], GSW_QT_BIN_F32_L4[y][1]};
    }
}

// Bin-safe rounding: round as the l = 1 store does (fp64 -> fp32 -> dtype), then clamp into [smallest value >= T_y, largest value
// < T_(y+1)] of the output dtype.  z itself lies in that interval up to the last ulps of ndtri, so the clamp returns the nearest
// representable value that quantises to y.
template <typename OutT, typename ZT>
__device__ __forceinline__ void store_binsafe(OutT* dst, const ZT (&z)[4], const uint32_t (&y)[4], const typename BinOf<OutT>::V* bins /* LDS */) {
    if constexpr (std::is_same<OutT, double>::value) {
        double o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { const double2 b = bins[y[k]]; o[k] = fmin(fmax((double)z[k], b.x), b.y); }
        Vec4Store<double>::st(dst, o);
    } else {
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { const float2 b = bins[y[k]]; o[k] = fminf(fmaxf(round_to<OutT>((float)z[k]), b.x), b.y); }
        Vec4Store<OutT>::stf(dst, o);
    }
}

// The four elements e .. e+3 of image `img`, one thread: uniforms (usrc, or the Philox group of e) -> z -> bin-safe 16-byte store at dst.
// Element e + k owns bits [l (3 - k), l (4 - k)) of yw.  The body of gsw_embed_l_kernel's image loop, shared with the per-record kernel
// (gswm_codec_keyed.inc).
template <typename OutT, int L, bool HAS_U, bool FAST>
__device__ __forceinline__ void embed_quad_l(OutT* dst, const double* usrc, uint32_t e, uint64_t img, uint32_t k0, uint32_t k1, uint32_t yw,
                                             const typename BinOf<OutT>::V* bins /* LDS */) {
    constexpr uint32_t FULL = 1u << L, HALF = FULL / 2u, MASK = FULL - 1u;
    constexpr double INV = 1.0 / (double)FULL, INVH = 1.0 / (double)HALF;
    double u[4];
    if (HAS_U) {
        const double2 ua = reinterpret_cast<const double2*>(usrc)[0];
        const double2 ub = reinterpret_cast<const double2*>(usrc)[1];
        u[0] = ua.x; u[1] = ua.y; u[2] = ub.x; u[3] = ub.y;
    } else {
        uint32_t w[4];
        philox4x32<GSW_PHILOX_ROUNDS>(e >> 2, 0u, (uint32_t)img, (uint32_t)(img >> 32), k0, k1, w);
#pragma unroll
        for (int k = 0; k < 4; ++k) u[k] = u_from_word(w[k]);
    }
    uint32_t y[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = (yw >> (L * (3 - k))) & MASK;
    if (FAST) {
        // the tail-side mass, exact in fp64 up to one rounding: p = (u + y) / 2^l below the median, 1 - p = ((2^l - 1 - y) + (1 - u)) / 2^l
        // above it; v = 2 min(p, 1 - p), x = 1 - v as the l = 1 fast path takes them
        float v[4], x[4], a[4], zf[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double m = y[k] < HALF ? u[k] + (double)y[k] : (double)(MASK - y[k]) + (1.0 - u[k]);
            const double vd = m * INVH;
            v[k] = (float)vd;
            x[k] = (float)(1.0 - vd);
        }
        ndtri_fast_abs4(v, x, a);
#pragma unroll
        for (int k = 0; k < 4; ++k) zf[k] = y[k] < HALF ? -a[k] : a[k];
        // The fp32 tail polynomial was fitted for l = 1, whose argument stops at v = 2^-53; here it reaches 2^-53 / 2^(l-1).
        // Below 2^-50 (one element in 10^15) the element takes the exact core instead.  Only a supplied u gets there: a Philox
        // uniform is (w + .5) 2^-32, so v >= 2^-33 / 2^(l-1), and that instantiation carries no fp64 core (and not its registers).
        if constexpr (HAS_U) {
            const float vmin = fminf(fminf(v[0], v[1]), fminf(v[2], v[3]));
            if (!(vmin >= 0x1p-50f)) {
#pragma unroll 1
                for (int k = 0; k < 4; ++k)
                    if (!(v[k] >= 0x1p-50f)) zf[k] = (float)ndtri_cephes((u[k] + (double)y[k]) * INV);
            }
        }
        store_binsafe<OutT, float>(dst, zf, y, bins);
    } else {
        double z[4];
#pragma unroll 1
        for (int k = 0; k < 4; ++k) z[k] = ndtri_cephes((u[k] + (double)y[k]) * INV);
        store_binsafe<OutT, double>(dst, z, y, bins);
    }
}

template <typename OutT, int L, bool HAS_U, bool FAST>
__global__ __launch_bounds__(GSW_WG) void gsw_embed_l_kernel(EmbedArgs p) {
    constexpr uint32_t FULL = 1u << L;
    __shared__ uint32_t ks_words[64 * L];  // 4 l blocks x 16 words
    __shared__ typename BinOf<OutT>::V bins[FULL];
    const uint32_t tid = threadIdx.x;
    if (tid < FULL) bins[tid] = bin_entry<L, OutT>(tid);
    const uint32_t chunk = (blockIdx.x + blockIdx.y) % gridDim.x;   // the l = 1 kernel's XCD rotation
    const uint32_t N = p.n_elems;
    const uint32_t e_chunk = chunk * GSW_CHUNK;
    const uint32_t cbytes = (min(GSW_CHUNK, N - e_chunk) * L + 7u) >> 3;
    chacha20_blocks_to_lds(GSW_CIPHER_REGS(p.ck), (uint64_t)chunk * (4u * L), (cbytes + 63u) >> 6, ks_words);
    __syncthreads();
    const uint8_t* ksb = reinterpret_cast<const uint8_t*>(ks_words);

    // window bits per round: element e_r + k owns bits [l (3 - k), l (4 - k)) of yw[r]
    uint32_t yw[2], e_r[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const uint32_t el = r * 1024u + 4u * tid;
        const uint32_t e = e_chunk + el;
        e_r[r] = e;
        uint32_t w = 0;
        if (e < N) {
#pragma unroll
            for (int i = 0; i < L / 2; ++i) {
                uint32_t c = ksb[((el * L) >> 3) + i];
                const uint32_t g = ((e * L) >> 3) + i;                // cipher byte of the image
                if (g * 8u < p.lim_elems) {                           // lim is a multiple of 8: whole bytes in or out
                    const uint32_t mi = g % p.msg_bytes;
                    c ^= p.msg_dev ? p.msg_dev[mi] : inline_msg_byte(mi);
                }
                w = (w << 8) | c;
            }
        }
        yw[r] = w;
    }

    const uint32_t k0 = (uint32_t)p.seed, k1 = (uint32_t)(p.seed >> 32);
    for (int b = blockIdx.y; b < p.B; b += gridDim.y) {
        const uint64_t img = p.image_index0 + (uint64_t)b;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const uint32_t e = e_r[r];
            if (e >= N) continue;
            const size_t off = (size_t)b * N + e;
            OutT* dst = reinterpret_cast<OutT*>(p.out) + off;
            embed_quad_l<OutT, L, HAS_U, FAST>(dst, p.u + off, e, img, k0, k1, yw[r], bins);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Extract: one workgroup per image (grid-stride).  LDS: [keystream of the image's Nb bits][decrypted bytes][vote bits]; the keystream
// is generated once per workgroup.  A thread quantises eight elements (one 16-byte load of a 16-bit dtype) into l bytes, decrypts
// them as one 16- or 32-bit word and leaves them in LDS; after a barrier thread m counts bit m over the Nb / M copies.
// ------------------------------------------------------------------------------------------------
struct ExtractLArgs {
    GswCipher ck;
    const void* z;     // [B][N]
    uint8_t* bits;     // [B][ceil(M/8)]
    uint32_t* counts;  // [B][M] or nullptr
    uint32_t* flags;   // [B]
    uint32_t n_elems;  // N
    uint32_t msg_bits; // M
    int32_t B;
};

template <typename T, int L>
__global__ __launch_bounds__(GSW_WG) void gsw_extract_l_kernel(ExtractLArgs p) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t tid = threadIdx.x;
    const uint32_t N = p.n_elems, M = p.msg_bits;
    const uint32_t ngroups = (N + 7u) >> 3;
    const uint32_t gbytes = ngroups * L;          // staged bytes (whole groups); the first N l / 8 are the lattice's
    const uint32_t nblk = (gbytes + 63u) >> 6;
    const uint32_t out_bytes = (M + 7u) >> 3;
    const uint32_t out_words = (M + 31u) >> 5;
    uint32_t* ks_words = lds;
    uint32_t* ptw = lds + nblk * 16u;
    const uint8_t* pt = reinterpret_cast<const uint8_t*>(ptw);
    uint32_t* vote = ptw + ((gbytes + 3u) >> 2);
    __shared__ uint32_t s_flags;
    const T* z = reinterpret_cast<const T*>(p.z);

    chacha20_blocks_to_lds(GSW_CIPHER_REGS(p.ck), 0u, nblk, ks_words);
    const uint32_t nseg = (N * L) / M;

    for (int b = blockIdx.x; b < p.B; b += gridDim.x) {
        for (uint32_t i = tid; i < out_words; i += GSW_WG) vote[i] = 0;
        if (tid == 0) s_flags = 0;
        __syncthreads();
        const size_t base = (size_t)b * N;
        uint32_t flags = 0;
        for (uint32_t g = tid; g < ngroups; g += GSW_WG) {
            const uint32_t bits = quant_group8<T, L>(z, base, g << 3, N, flags);
            if constexpr (L == 2) {
                const uint32_t le = ((bits >> 8) & 0xFFu) | ((bits & 0xFFu) << 8);    // first byte at the lower address
                reinterpret_cast<uint16_t*>(ptw)[g] = (uint16_t)(le ^ reinterpret_cast<const uint16_t*>(ks_words)[g]);
            } else {
                ptw[g] = __builtin_bswap32(bits) ^ ks_words[g];
            }
        }
        or_image_flags(flags, &s_flags);
        __syncthreads();
        if ((M & 7u) == 0) {
            const uint32_t Mb = M >> 3;
            for (uint32_t m = tid; m < M; m += GSW_WG) {
                const uint32_t sh = 7u - (m & 7u);
                uint32_t c1 = 0, o = m >> 3;
                for (uint32_t c = 0; c < nseg; ++c, o += Mb) c1 += (pt[o] >> sh) & 1u;
                if (2u * c1 > nseg) atomicOr(&vote[m >> 5], 1u << (m & 31u));
                if (p.counts) p.counts[(size_t)b * M + m] = c1;
            }
        } else {
            for (uint32_t m = tid; m < M; m += GSW_WG) {
                uint32_t c1 = 0, idx = m;
                for (uint32_t c = 0; c < nseg; ++c, idx += M) c1 += (pt[idx >> 3] >> (7u - (idx & 7u))) & 1u;
                if (2u * c1 > nseg) atomicOr(&vote[m >> 5], 1u << (m & 31u));
                if (p.counts) p.counts[(size_t)b * M + m] = c1;
            }
        }
        __syncthreads();
        for (uint32_t t = tid; t < out_bytes; t += GSW_WG) {
            const uint32_t w = (vote[t >> 2] >> (8u * (t & 3u))) & 0xFFu;  // bits 8t..8t+7, LSB-first
            p.bits[(size_t)b * out_bytes + t] = (uint8_t)(__brev(w) >> 24);  // -> MSB-first byte
        }
        if (tid == 0) p.flags[b] = s_flags;
        __syncthreads();
    }
}

// The l-bit form of gsw_sign_pack: the window bits alone, one thread per eight elements (l bytes); flags_out is zeroed by the caller.
template <typename T, int L>
__global__ __launch_bounds__(GSW_WG) void gsw_quant_pack_kernel(const T* __restrict__ z, uint8_t* __restrict__ out, uint32_t* __restrict__ flags_out,
                                                                uint32_t N, int B) {
    const uint32_t g = blockIdx.x * GSW_WG + threadIdx.x;
    const uint32_t ngroups = (N + 7u) >> 3;
    const uint32_t rowbytes = (N * L) >> 3;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        uint32_t flags = 0;
        if (g < ngroups) {
            const uint32_t bits = quant_group8<T, L>(z, (size_t)b * N, g << 3, N, flags);
            uint8_t* row = out + (size_t)b * rowbytes;
            if ((N & 7u) == 0 && (reinterpret_cast<uintptr_t>(out) & (uintptr_t)(L - 1)) == 0) {
                // whole groups only, and every row starts on an l-byte boundary: one store, first byte at the lower address
                if constexpr (L == 2) reinterpret_cast<uint16_t*>(row)[g] = (uint16_t)(((bits >> 8) & 0xFFu) | ((bits & 0xFFu) << 8));
                else reinterpret_cast<uint32_t*>(row)[g] = __builtin_bswap32(bits);
            } else {
#pragma unroll
                for (int i = 0; i < L; ++i)
                    if (g * L + i < rowbytes) row[g * L + i] = (uint8_t)(bits >> (8 * (L - 1 - i)));
            }
        }
        or_image_flags(flags, &flags_out[b]);
    }
}

template <typename OutT, int L>
static void launch_embed_l(const EmbedArgs& a, bool has_u, bool fast, dim3 grid, hipStream_t st) {
    if (has_u) {
        if (fast) hipLaunchKernelGGL((gsw_embed_l_kernel<OutT, L, true, true>), grid, dim3(GSW_WG), 0, st, a);
        else hipLaunchKernelGGL((gsw_embed_l_kernel<OutT, L, true, false>), grid, dim3(GSW_WG), 0, st, a);
    } else {
        if (fast) hipLaunchKernelGGL((gsw_embed_l_kernel<OutT, L, false, true>), grid, dim3(GSW_WG), 0, st, a);
        else hipLaunchKernelGGL((gsw_embed_l_kernel<OutT, L, false, false>), grid, dim3(GSW_WG), 0, st, a);
    }
}

template <int L>
static void launch_embed_l_dtype(const EmbedArgs& a, int out_dtype, bool has_u, bool fast, dim3 grid, hipStream_t st) {
    switch (out_dtype) {
        case GSW_F32: launch_embed_l<float, L>(a, has_u, fast, grid, st); break;
        case GSW_F16: launch_embed_l<__half, L>(a, has_u, fast, grid, st); break;
        case GSW_BF16: launch_embed_l<__hip_bfloat16, L>(a, has_u, fast, grid, st); break;
        default: launch_embed_l<double, L>(a, has_u, fast, grid, st); break;
    }
}

template <typename T, int L>
static int launch_extract_l(const ExtractLArgs& a, hipStream_t st) {
    const uint32_t gbytes = ((a.n_elems + 7u) / 8u) * L;
    const size_t lds = (size_t)((gbytes + 63u) / 64u) * 64u + (size_t)((gbytes + 3u) / 4u) * 4u + (size_t)((a.msg_bits + 31u) / 32u) * 4u;
    if (lds > GSW_MAX_DYN_LDS) return GSW_ERR_UNSUPPORTED;
    const uint32_t grid = (uint32_t)std::min<int64_t>(a.B, (int64_t)device_cus() * 8);
    GSW_HIP(allow_dynamic_lds((const void*)gsw_extract_l_kernel<T, L>, lds));
    hipLaunchKernelGGL((gsw_extract_l_kernel<T, L>), dim3(grid), dim3(GSW_WG), lds, st, a);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

template <int L>
static int launch_extract_l_dtype(const ExtractLArgs& a, int dtype, hipStream_t st) {
    switch (dtype) {
        case GSW_F32: return launch_extract_l<float, L>(a, st);
        case GSW_F16: return launch_extract_l<__half, L>(a, st);
        case GSW_BF16: return launch_extract_l<__hip_bfloat16, L>(a, st);
        default: return launch_extract_l<double, L>(a, st);
    }
}

template <typename T, int L>
static int launch_quant_pack(const void* z, uint8_t* out, uint32_t* flags, int B, uint32_t n, hipStream_t st) {
    const uint32_t ngroups = (n + 7u) / 8u;
    const dim3 grid((ngroups + GSW_WG - 1) / GSW_WG, (uint32_t)std::min(B, 65535));
    hipLaunchKernelGGL((gsw_quant_pack_kernel<T, L>), grid, dim3(GSW_WG), 0, st, (const T*)z, out, flags, n, B);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

template <int L>
static int launch_quant_pack_dtype(const void* z, int dtype, uint8_t* out, uint32_t* flags, int B, uint32_t n, hipStream_t st) {
    switch (dtype) {
        case GSW_F32: return launch_quant_pack<float, L>(z, out, flags, B, n, st);
        case GSW_F16: return launch_quant_pack<__half, L>(z, out, flags, B, n, st);
        case GSW_BF16: return launch_quant_pack<__hip_bfloat16, L>(z, out, flags, B, n, st);
        default: return launch_quant_pack<double, L>(z, out, flags, B, n, st);
    }
}

// GSW_OK for a supported window whose bits fill whole bytes and whose bit count fits the 32-bit index algebra
static int window_check(int l, int64_t n_elems) {
    if (l != 1 && l != 2 && l != 4) return GSW_ERR_UNSUPPORTED;
    if (l > 1 && n_elems > 0 && ((n_elems * l) % 8 != 0 || n_elems * l > (int64_t)0x7FFFFFF0)) return GSW_ERR_UNSUPPORTED;
    return GSW_OK;
}

}  // namespace codec_l

int gsw_embed_l(const uint8_t key[32], const uint8_t nonce16[16], const uint8_t* msg, int msg_bytes, const double* u_dev, uint64_t seed,
                uint64_t image_index0, void* out_dev, int out_dtype, int B, int64_t n_elems, uint32_t flags, int l, void* stream) {
    const int wc = codec_l::window_check(l, n_elems);
    if (wc != GSW_OK) return wc;
    if (l == 1) return gsw_embed(key, nonce16, msg, msg_bytes, u_dev, seed, image_index0, out_dev, out_dtype, B, n_elems, flags, stream);
    if (!key || !nonce16 || !msg || msg_bytes <= 0 || msg_bytes > (1 << 27) || !out_dev || B < 0 || n_elems <= 0 || (n_elems & 3)) return GSW_ERR_BAD_ARG;
    if (out_dtype < GSW_F32 || out_dtype > GSW_F64) return GSW_ERR_BAD_ARG;
    if (B == 0) return GSW_OK;
    hipStream_t st = (hipStream_t)stream;
    EmbedArgs a;
    memset(&a, 0, sizeof(a));
    a.ck = make_cipher(key, nonce16);
    uint8_t* staged = nullptr;
    if (msg_bytes <= GSW_MSG_INLINE_MAX) {
        memcpy(a.msg.b, msg, (size_t)msg_bytes);
    } else {   // as gsw_embed: the one allocation the header documents
        GSW_HIP(hipMallocAsync((void**)&staged, (size_t)msg_bytes, st));
        GSW_HIP(hipMemcpyAsync(staged, msg, (size_t)msg_bytes, hipMemcpyHostToDevice, st));
        a.msg_dev = staged;
    }
    const int64_t nbits = n_elems * l, msg_bits = (int64_t)msg_bytes * 8;
    a.u = u_dev;
    a.out = out_dev;
    a.seed = seed;
    a.image_index0 = image_index0;
    a.n_elems = (uint32_t)n_elems;
    a.msg_bytes = (uint32_t)msg_bytes;
    a.msg_bits = (uint32_t)msg_bits;
    a.lim_elems = (uint32_t)((nbits / msg_bits) * msg_bits);   // in bits
    a.B = B;
    const uint32_t nchunks = (uint32_t)((n_elems + GSW_CHUNK - 1) / GSW_CHUNK);
    uint32_t G = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(B, ((int64_t)device_cus() * 8 + nchunks - 1) / nchunks));
    G = std::min<uint32_t>(G, 65535u);
    const dim3 grid(nchunks, G);
    const bool fast = (flags & GSW_EMBED_FAST_F32) != 0;
    if (l == 2) codec_l::launch_embed_l_dtype<2>(a, out_dtype, u_dev != nullptr, fast, grid, st);
    else codec_l::launch_embed_l_dtype<4>(a, out_dtype, u_dev != nullptr, fast, grid, st);
    hipError_t le = hipGetLastError();
    if (staged) (void)hipFreeAsync(staged, st);
    if (le != hipSuccess) return hip_fail(le);
    return GSW_OK;
}

int gsw_extract_l(const void* z_dev, int z_dtype, const uint8_t key[32], const uint8_t nonce16[16], int msg_bits, uint8_t* bits_dev,
                  uint32_t* counts_dev, uint32_t* flags_dev, int B, int64_t n_elems, int l, void* stream) {
    const int wc = codec_l::window_check(l, n_elems);
    if (wc != GSW_OK) return wc;
    if (l == 1) return gsw_extract(z_dev, z_dtype, key, nonce16, msg_bits, bits_dev, counts_dev, flags_dev, B, n_elems, stream);
    if (!z_dev || !key || !nonce16 || msg_bits <= 0 || !bits_dev || !flags_dev || B < 0 || n_elems <= 0) return GSW_ERR_BAD_ARG;
    if (z_dtype < GSW_F32 || z_dtype > GSW_F64) return GSW_ERR_BAD_ARG;
    if ((n_elems * l) % msg_bits) return GSW_ERR_RAGGED;
    if (B == 0) return GSW_OK;
    codec_l::ExtractLArgs a;
    memset(&a, 0, sizeof(a));
    a.ck = make_cipher(key, nonce16);
    a.z = z_dev;
    a.bits = bits_dev;
    a.counts = counts_dev;
    a.flags = flags_dev;
    a.n_elems = (uint32_t)n_elems;
    a.msg_bits = (uint32_t)msg_bits;
    a.B = B;
    hipStream_t st = (hipStream_t)stream;
    return l == 2 ? codec_l::launch_extract_l_dtype<2>(a, z_dtype, st) : codec_l::launch_extract_l_dtype<4>(a, z_dtype, st);
}

int gsw_quant_pack(const void* z_dev, int z_dtype, uint8_t* packed_dev, uint32_t* flags_dev, int B, int64_t n_elems, int l, void* stream) {
    const int wc = codec_l::window_check(l, n_elems);
    if (wc != GSW_OK) return wc;
    if (l == 1) return gsw_sign_pack(z_dev, z_dtype, packed_dev, flags_dev, B, n_elems, stream);
    if (!z_dev || !packed_dev || !flags_dev || B < 0 || n_elems < 1) return GSW_ERR_BAD_ARG;
    if (z_dtype < GSW_F32 || z_dtype > GSW_F64) return GSW_ERR_BAD_ARG;
    if (B == 0) return GSW_OK;
    hipStream_t st = (hipStream_t)stream;
    GSW_HIP(hipMemsetAsync(flags_dev, 0, (size_t)B * sizeof(uint32_t), st));
    return l == 2 ? codec_l::launch_quant_pack_dtype<2>(z_dev, z_dtype, packed_dev, flags_dev, B, (uint32_t)n_elems, st)
                  : codec_l::launch_quant_pack_dtype<4>(z_dev, z_dtype, packed_dev, flags_dev, B, (uint32_t)n_elems, st);
}
