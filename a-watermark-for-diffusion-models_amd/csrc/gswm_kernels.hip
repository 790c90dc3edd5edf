// gswm_kernels.hip -- hand-written CDNA4 (gfx950) kernels + C ABI of the Gaussian-Shading watermark hot path.
//
// Built only for gfx950 (wave64, 256 CUs / 8 XCDs, 160 KiB LDS per CU):
//     hipcc --offload-arch=gfx950 -O3 -std=c++17 -shared -fPIC gswm_kernels.hip -o libgswm.so
//
// Reference semantics (file:line relative to lthero-big/A-watermark-for-Diffusion-Models @ 2024_08_07):
//   embed   : gs_insert.py:8-66, ComfyUI_GSWaterMark/nodes.py:51-123
//   extract : extract.py:72-101
//   ddim    : __pycache__/inverse_stable_diffusion_gs.cpython-38.pyc (backward_ddim) / diffusers DDIM(Inverse)Scheduler
// The algorithms are restated from SURVEY.md Appendix A; nothing here is translated code (the reference is
// pure Python on top of OpenSSL / scipy / numpy).
//
// Data layout in HBM
//   latents  [B][N]   N = 4*(H/8)*(W/8), C-order flat lattice index i; fp32 / fp16 / bf16 / fp64
//   u        [B][N]   fp64 (bit-parity mode only)
//   bits     [B][ceil(M/8)] recovered message bytes, MSB-first
//   counts   [B][M]   uint32 '1'-votes per message bit (optional)
//   flags    [B]      uint32
// Index algebra: cipher byte j = i>>3, bit 7-(i&7); keystream byte j = byte j&63 of ChaCha20 block j>>6.

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <stddef.h>
#include <algorithm>
#include <type_traits>

#include "../../include/gswm.h"

#define GSW_WG 256  // 4 waves of 64

// ------------------------------------------------------------------------------------------------
// kernel-argument blocks (passed by value: they live in the kernarg segment, read through SGPRs)
// ------------------------------------------------------------------------------------------------
struct GswCipher {
    uint32_t key[8];
    uint32_t nonce[4];  // [0],[1] = 64-bit block counter (OpenSSL carries word 12 into word 13); [2],[3] = nonce tail
};

struct GswMsgInline {
    uint8_t b[GSW_MSG_INLINE_MAX];
};

#include "gswm_chacha.h"   // ChaCha20, four lanes per 64-byte block: CipherRegs, chacha20_block, chacha20_blocks_to_lds
#include "gswm_record.h"   // one record per image: layout, operand check, repeated message, vote tail
#include "gswm_host.h"     // GSW_HIP, hip_fail, device_cus, allow_dynamic_lds

// ------------------------------------------------------------------------------------------------
// Philox4x32-R (in-kernel uniform source; NOT reference behaviour -- the reference draws from numpy's
// MT19937).  counter = (pair_lo, pair_hi, img_lo, img_hi), key = seed.  Restated in oracle/gs_oracle.py.
// The throughput stream runs R = 7 rounds: Random123's philox4x32_R(7), the shortest variant its authors report as passing BigCrush
// (Salmon et al., SC'11, table 2; 10 is their default safety margin).  The embed kernel is VALU-bound on exactly these rounds (two
// quarter-rate v_mad_u64_u32 each): 7 instead of 10 is ~25 % fewer instruction slots per store.
// ------------------------------------------------------------------------------------------------
constexpr int GSW_PHILOX_ROUNDS = 7;
template <int R>
__device__ __forceinline__ void philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                           uint32_t (&o)[4]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// In-kernel uniform: ONE 32-bit word per element, u = (w + 0.5) * 2^-32 in (0, 1) -- exactly representable in fp64.
// Group g = e >> 2 of image `img` draws Philox4x32-7(counter = (g, 0, img_lo, img_hi), key = seed); element e takes
// word e & 3.  One Philox call per 16-byte fp32 store.
__device__ __forceinline__ double u_from_word(uint32_t w) { return fma((double)w, 0x1p-32, 0x1p-33); }

// ------------------------------------------------------------------------------------------------
// Inverse normal CDF.
// Exact path: Cephes ndtri (the routine scipy.stats.norm.ppf -> scipy.special.ndtri runs), evaluated in
// fp64 in the same operation order; coefficients are the published Cephes tables.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double polevl5(double x, const double (&c)[5]) {
    double a = c[0];
#pragma unroll
    for (int i = 1; i < 5; ++i) a = a * x + c[i];
    return a;
}
__device__ __forceinline__ double polevl9(double x, const double (&c)[9]) {
    double a = c[0];
#pragma unroll
    for (int i = 1; i < 9; ++i) a = a * x + c[i];
    return a;
}
__device__ __forceinline__ double p1evl8(double x, const double (&c)[8]) {
    double a = x + c[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) a = a * x + c[i];
    return a;
}

__device__ __forceinline__ double ndtri_cephes(double y0) {
    constexpr double P0[5] = {-5.99633501014107895267E1, 9.80010754185999661536E1, -5.66762857469070293439E1,
                              1.39312609387279679503E1, -1.23916583867381258016E0};
    constexpr double Q0[8] = {1.95448858338141759834E0, 4.67627912898881538453E0, 8.63602421390890590575E1,
                              -2.25462687854119370527E2, 2.00260212380060660359E2, -8.20372256168333339912E1,
                              1.59056225126211695515E1, -1.18331621121330003142E0};
    constexpr double P1[9] = {4.05544892305962419923E0, 3.15251094599893866154E1, 5.71628192246421288162E1,
                              4.40805073893200834700E1, 1.46849561928858024014E1, 2.18663306850790267539E0,
                              -1.40256079171354495875E-1, -3.50424626827848203418E-2, -8.57456785154685413611E-4};
    constexpr double Q1[8] = {1.57799883256466749731E1, 4.53907635128879210584E1, 4.13172038254672030440E1,
                              1.50425385692907503408E1, 2.50464946208309415979E0, -1.42182922854787788574E-1,
                              -3.80806407691578277194E-2, -9.33259480895457427372E-4};
    constexpr double P2[9] = {3.23774891776946035970E0, 6.91522889068984211695E0, 3.93881025292474443415E0,
                              1.33303460815807542389E0, 2.01485389549179081538E-1, 1.23716634817820021358E-2,
                              3.01581553508235416007E-4, 2.65806974686737550832E-6, 6.23974539184983293730E-9};
    constexpr double Q2[8] = {6.02427039364742014255E0, 3.67983563856160859403E0, 1.37702099489081330271E0,
                              2.16236993594496635890E-1, 1.34204006088543189037E-2, 3.28014464682127739104E-4,
                              2.89247864745380683936E-6, 6.79019408009981274425E-9};
    constexpr double EXPM2 = 0.13533528323661269189;
    constexpr double S2PI = 2.50662827463100050242E0;
    if (y0 <= 0.0) return -INFINITY;  // norm.ppf(0) == -inf (u == 0 with a zero cipher bit)
    if (y0 >= 1.0) return INFINITY;
    bool negate = true;
    double y = y0;
    if (y > 1.0 - EXPM2) { y = 1.0 - y; negate = false; }
    if (y > EXPM2) {
        y = y - 0.5;
        const double y2 = y * y;
        double x = y + y * (y2 * polevl5(y2, P0) / p1evl8(y2, Q0));
        return x * S2PI;
    }
    double x = sqrt(-2.0 * log(y));
    const double x0 = x - log(x) / x;
    const double z = 1.0 / x;
    double x1;
    if (x < 8.0) x1 = z * polevl9(z, P1) / p1evl8(z, Q1);
    else         x1 = z * polevl9(z, P2) / p1evl8(z, Q2);
    x = x0 - x1;
    return negate ? -x : x;
}

// Fast path: z = sign * sqrt(2) * erfinv(1 - v) with v = min(p, 1-p)*2 taken from the side that is exact in fp64
// (v = u for a 0 bit, 1 - u for a 1 bit; both exact for 53-bit u), w = -log(v (2 - v)) and two minimax
// polynomials in fp32 (coefficients fitted offline against mpmath, see tools/fit_ndtri_fast.py).
// |z_fast - ndtri_fp64| <= 4e-6 over the whole 53-bit u range (tests pin <= 1e-5).
#include "ndtri_fast_coeffs.inc"

__device__ __forceinline__ float ndtri_fast_tail(float w) {
    const float t = __fsqrt_rn(w) - GSW_NF_C1;
    float r = GSW_NF_B[0];
#pragma unroll
    for (int i = 1; i < GSW_NF_NB; ++i) r = fmaf(r, t, GSW_NF_B[i]);
    return r;
}

// |ndtri(v/2)| for 4 elements; v in (0,1], x = 1 - v (each rounded from an exact value); v == 0 -> +inf.
// The central polynomial covers w < 10 (v > 2.3e-5): a wave takes the tail branch for ~0.6 % of its 4-element groups.
__device__ __forceinline__ void ndtri_fast_abs4(const float (&v)[4], const float (&x)[4], float (&a)[4]) {
    float w[4], r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        w[k] = -0.69314718056f * __log2f(v[k] * (2.0f - v[k]));
        const float t = w[k] - GSW_NF_C0;
        float q = GSW_NF_A[0];
#pragma unroll
        for (int i = 1; i < GSW_NF_NA; ++i) q = fmaf(q, t, GSW_NF_A[i]);
        r[k] = q;
    }
    const float wmax = fmaxf(fmaxf(w[0], w[1]), fmaxf(w[2], w[3]));
    if (!(wmax < GSW_NF_SPLIT)) {   // also catches w = +inf (v == 0) and NaN
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (!(w[k] < GSW_NF_SPLIT)) r[k] = ndtri_fast_tail(w[k]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) a[k] = r[k] * x[k];
}

// RNG fast path: |z| straight from the tail-side 32-bit uniform word through a piecewise-cubic table indexed by the
// position of the leading one (logarithmic segmentation = relative resolution in the tail); no log, no branch.
// Generated + verified by tools/fit_icdf_table.py (max |dz| 5.2e-7 vs fp64 ndtri over the whole 32-bit range).
#include "icdf_table.inc"

__device__ __forceinline__ float icdf_table_abs(uint32_t wv, const float4* __restrict__ tab /* LDS */) {
    const uint32_t lz = wv ? (uint32_t)__builtin_clz(wv) : 32u;
    const uint32_t norm = wv << (lz & 31u);                                     // leading one at bit 31 (0 stays 0)
    const uint32_t sub = (norm >> (31 - GSW_ICDF_M)) & ((1u << GSW_ICDF_M) - 1u);
    const float t = (float)(norm << (GSW_ICDF_M + 1)) * 0x1p-32f;               // position inside the sub-interval, [0,1)
    const float4 c = tab[(lz << GSW_ICDF_M) + sub];
    const float r = fmaf(fmaf(fmaf(c.w, t, c.z), t, c.y), t, c.x);
    return fmaxf(r, 1.0e-10f);   // true minimum is 1.46e-10: rounding noise near v -> 1 can never zero or flip the magnitude
}

// ------------------------------------------------------------------------------------------------
// output conversion (fp64 -> fp32 -> fp16/bf16 mirrors the caller's `.float()` then `.half()`, README.md:112)
// ------------------------------------------------------------------------------------------------
template <typename T> struct Vec4Store;
template <> struct Vec4Store<float> {
    static __device__ __forceinline__ void st(float* p, const double (&z)[4]) {
        float4 v = make_float4((float)z[0], (float)z[1], (float)z[2], (float)z[3]);
        *reinterpret_cast<float4*>(p) = v;
    }
    static __device__ __forceinline__ void stf(float* p, const float (&z)[4]) {
        // Non-temporal: a batch of fp32 Z_s_T (1 GiB at 16 384 images) is written once and read by nobody on this device soon.  Plain stores leave the
        // last ~256 MB dirty in the memory-side cache, and their write-back competes with the NEXT kernel's reads: the extract of the same codec step read
        // at 3.6 TB/s behind plain stores and reads at 5.2 TB/s behind these (the embed itself: 5.17 -> 4.8-5.0 TB/s; the step: +10 %).
        typedef float f4v __attribute__((ext_vector_type(4)));
        __builtin_nontemporal_store(f4v{z[0], z[1], z[2], z[3]}, reinterpret_cast<f4v*>(p));
    }
};
template <> struct Vec4Store<double> {
    static __device__ __forceinline__ void st(double* p, const double (&z)[4]) {
        reinterpret_cast<double2*>(p)[0] = make_double2(z[0], z[1]);
        reinterpret_cast<double2*>(p)[1] = make_double2(z[2], z[3]);
    }
    static __device__ __forceinline__ void stf(double* p, const float (&z)[4]) {
        reinterpret_cast<double2*>(p)[0] = make_double2((double)z[0], (double)z[1]);
        reinterpret_cast<double2*>(p)[1] = make_double2((double)z[2], (double)z[3]);
    }
};
template <> struct Vec4Store<__half> {
    static __device__ __forceinline__ void stf(__half* p, const float (&z)[4]) {
        union { __half2 h[2]; uint2 u; } v;
        v.h[0] = __floats2half2_rn(z[0], z[1]);
        v.h[1] = __floats2half2_rn(z[2], z[3]);
        *reinterpret_cast<uint2*>(p) = v.u;
    }
    static __device__ __forceinline__ void st(__half* p, const double (&z)[4]) {
        const float f[4] = {(float)z[0], (float)z[1], (float)z[2], (float)z[3]};
        stf(p, f);
    }
};
template <> struct Vec4Store<__hip_bfloat16> {
    static __device__ __forceinline__ void stf(__hip_bfloat16* p, const float (&z)[4]) {
        union { __hip_bfloat16 h[4]; uint2 u; } v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v.h[i] = __float2bfloat16(z[i]);
        *reinterpret_cast<uint2*>(p) = v.u;
    }
    static __device__ __forceinline__ void st(__hip_bfloat16* p, const double (&z)[4]) {
        const float f[4] = {(float)z[0], (float)z[1], (float)z[2], (float)z[3]};
        stf(p, f);
    }
};

// ------------------------------------------------------------------------------------------------
// E2: keystream to HBM (known-answer tests; the hot kernels keep their keystream window in LDS instead)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GSW_WG) void gsw_keystream_kernel(GswCipher ck, uint8_t* __restrict__ out, uint64_t nbytes) {
    __shared__ uint32_t ks[(GSW_WG / 4) * 16];  // 64 blocks = 4 KiB per workgroup
    const uint64_t nblocks_total = (nbytes + 63) / 64;
    for (uint64_t first = (uint64_t)blockIdx.x * (GSW_WG / 4); first < nblocks_total; first += (uint64_t)gridDim.x * (GSW_WG / 4)) {
        const uint32_t nb = (uint32_t)min((uint64_t)(GSW_WG / 4), nblocks_total - first);
        chacha20_blocks_to_lds(GSW_CIPHER_REGS(ck), first, nb, ks);
        __syncthreads();
        const uint8_t* kb = reinterpret_cast<const uint8_t*>(ks);
        for (uint32_t i = threadIdx.x; i < nb * 64u; i += GSW_WG) {
            const uint64_t g = first * 64 + i;
            if (g < nbytes) out[g] = kb[i];
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------
// Embed.  One workgroup = one 2048-element chunk (4 ChaCha blocks, 256 B of keystream in LDS) of the lattice,
// looped over a strided set of images: key, nonce and message are shared by the whole batch, so the cipher
// bits a thread owns are computed once and reused for every image.  Thread t owns elements
// chunk*2048 + r*1024 + 4t .. +3 (r = 0,1): one 16-byte fp32 store per round, fully coalesced.
// grid = (n_chunks, G): blockIdx.y strides the batch.
// ------------------------------------------------------------------------------------------------
#define GSW_CHUNK 2048u

struct EmbedArgs {
    GswCipher ck;
    GswMsgInline msg;       // inline message bytes (msg_dev == nullptr)
    const uint8_t* msg_dev; // staged message for msg_bytes > GSW_MSG_INLINE_MAX
    const double* u;        // [B][N] or nullptr
    void* out;              // [B][N]
    uint64_t seed, image_index0;
    uint32_t n_elems;       // N
    uint32_t msg_bytes;     // |k|
    uint32_t msg_bits;      // message bits (8*|k| for whole-byte messages)
    uint32_t lim_elems;     // repeats * msg_bits: elements past it carry plaintext 0 (nodes.py:85-87)
    int32_t B;
};

// Message byte `i` of the inline copy.  EmbedArgs is the first kernel argument, so it sits at offset 0 of the kernarg
// segment; reading it through the segment pointer keeps a lane-dependent index from forcing a scratch copy of the
// whole by-value struct.
typedef const uint8_t __attribute__((address_space(4))) * gsw_kernarg_bytes;
__device__ __forceinline__ uint32_t inline_msg_byte(uint32_t i) {
    gsw_kernarg_bytes ka = (gsw_kernarg_bytes)__builtin_amdgcn_kernarg_segment_ptr();
    return ka[offsetof(EmbedArgs, msg) + i];
}

// The four elements e .. e+3 of image `img`, one thread: uniforms (usrc, or the Philox group of e) -> z -> one 16-byte store at dst.
// Bit (3-k) of ynib is the cipher bit of element e + k.  The body of gsw_embed_kernel's image loop, shared with the per-record kernel
// (gswm_codec_keyed.inc).
template <typename OutT, bool HAS_U, bool FAST>
__device__ __forceinline__ void embed_quad(OutT* dst, const double* usrc, uint32_t e, uint64_t img, uint32_t k0, uint32_t k1, uint32_t ynib,
                                           const float4* icdf /* LDS, FAST && !HAS_U only */) {
    uint32_t w[4];
    double u[4];
    if (HAS_U) {
        const double2 ua = reinterpret_cast<const double2*>(usrc)[0];
        const double2 ub = reinterpret_cast<const double2*>(usrc)[1];
        u[0] = ua.x; u[1] = ua.y; u[2] = ub.x; u[3] = ub.y;
    } else {
        philox4x32<GSW_PHILOX_ROUNDS>(e >> 2, 0u, (uint32_t)img, (uint32_t)(img >> 32), k0, k1, w);
    }
    if (FAST) {
        float a[4];
        if (HAS_U) {
            float v[4], x[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool one = (ynib >> (3 - k)) & 1u;
                v[k] = (float)(one ? 1.0 - u[k] : u[k]);   // exact in fp64 for a 53-bit u, then one rounding
                x[k] = (float)(one ? u[k] : 1.0 - u[k]);
            }
            ndtri_fast_abs4(v, x, a);
        } else {
            // u = (w + .5) 2^-32  =>  1 - u = (~w + .5) 2^-32: the tail-side uniform is an integer select of the
            // Philox word, and |z| comes from the table without ever forming u
            const uint32_t ones = (ynib & 8u ? 1u : 0u) | (ynib & 4u ? 2u : 0u) | (ynib & 2u ? 4u : 0u) | (ynib & 1u ? 8u : 0u);
#pragma unroll
            for (int k = 0; k < 4; ++k) a[k] = icdf_table_abs(((ones >> k) & 1u) ? ~w[k] : w[k], icdf);
        }
        float zf[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t neg = ((~ynib >> (3 - k)) & 1u) << 31;   // cipher bit 0 -> negative half
            zf[k] = __uint_as_float(__float_as_uint(a[k]) | neg);
        }
        Vec4Store<OutT>::stf(dst, zf);
    } else {
        double z[4];
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {
            const double uk = HAS_U ? u[k] : u_from_word(w[k]);
            const double y = (double)((ynib >> (3 - k)) & 1u);
            z[k] = ndtri_cephes((uk + y) * 0.5);       // gs_insert.py:64, same operation order
        }
        Vec4Store<OutT>::st(dst, z);
    }
}

// BITMSG: message length is not a multiple of 8 bits -> plaintext bit looked up per element (generic geometry)
template <typename OutT, bool HAS_U, bool FAST, bool BITMSG>
__global__ __launch_bounds__(GSW_WG) void gsw_embed_kernel(EmbedArgs p) {
    __shared__ uint32_t ks_words[64];  // 4 blocks x 16 words
    __shared__ float4 icdf[(FAST && !HAS_U) ? GSW_ICDF_ENTRIES : 1];
    const uint32_t tid = threadIdx.x;
    if (FAST && !HAS_U)
        for (uint32_t i = tid; i < GSW_ICDF_ENTRIES; i += GSW_WG) icdf[i] = GSW_ICDF_TABLE[i];
    // Workgroup (x, y) is dispatched to XCD (x + gridDim.x * y) % 8.  With chunk == x every XCD would only ever write
    // addresses congruent to x * 8 KiB (mod 64 KiB), i.e. a fraction of its L2 channels; rotating by y spreads them.
    const uint32_t chunk = (blockIdx.x + blockIdx.y) % gridDim.x;
    const uint32_t N = p.n_elems;
    const uint32_t e_chunk = chunk * GSW_CHUNK;
    const uint32_t nblk = min(4u, (N - e_chunk + 511u) / 512u);
    chacha20_blocks_to_lds(GSW_CIPHER_REGS(p.ck), chunk * 4u, nblk, ks_words);
    __syncthreads();
    const uint8_t* ksb = reinterpret_cast<const uint8_t*>(ks_words);

    // cipher nibble per round: bit (3-k) of ynib[r] is the cipher bit of element e_r + k
    uint32_t ynib[2];
    uint32_t e_r[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const uint32_t e = e_chunk + r * 1024u + 4u * tid;
        e_r[r] = e;
        uint32_t nib = 0;
        if (e < N) {
            const uint32_t kbyte = ksb[(r * 128u) + (tid >> 1)];
            const uint32_t knib = (tid & 1u) ? (kbyte & 0xFu) : (kbyte >> 4);
            uint32_t pnib = 0;
            if (BITMSG) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t i = e + k;
                    uint32_t bit = 0;
                    if (i < p.lim_elems) {
                        const uint32_t m = i % p.msg_bits;
                        const uint32_t by = p.msg_dev ? p.msg_dev[m >> 3] : inline_msg_byte(m >> 3);
                        bit = (by >> (7u - (m & 7u))) & 1u;
                    }
                    pnib |= bit << (3 - k);
                }
            } else if (e < p.lim_elems) {                       // lim is a multiple of 8: whole bytes in or out
                const uint32_t mi = (e >> 3) % p.msg_bytes;     // global cipher byte -> message byte
                const uint32_t pbyte = p.msg_dev ? p.msg_dev[mi] : inline_msg_byte(mi);
                pnib = (tid & 1u) ? (pbyte & 0xFu) : (pbyte >> 4);
            }
            nib = knib ^ pnib;
        }
        ynib[r] = nib;
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
            embed_quad<OutT, HAS_U, FAST>(dst, p.u + off, e, img, k0, k1, ynib[r], icdf);
        }
    }
}

__global__ __launch_bounds__(GSW_WG) void gsw_philox_uniform_kernel(double* __restrict__ u, uint64_t seed, uint64_t image_index0,
                                                                    int B, uint32_t N) {
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const uint32_t ngroups = (N + 3) / 4;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const uint64_t img = image_index0 + (uint64_t)b;
        for (uint32_t g = blockIdx.x * GSW_WG + threadIdx.x; g < ngroups; g += gridDim.x * GSW_WG) {
            uint32_t w[4];
            philox4x32<GSW_PHILOX_ROUNDS>(g, 0u, (uint32_t)img, (uint32_t)(img >> 32), k0, k1, w);
            const size_t off = (size_t)b * N + 4u * g;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4u * g + k < N) u[off + k] = u_from_word(w[k]);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Extract: quantise -> decrypt -> majority vote.
//
// Element loaders: 8 consecutive lattice elements (one cipher byte) as fp32.
// ------------------------------------------------------------------------------------------------
template <typename T> struct Load8;
template <> struct Load8<float> {
    static __device__ __forceinline__ void ld(const float* p, float (&v)[8]) {
        const float4 a = reinterpret_cast<const float4*>(p)[0];
        const float4 b = reinterpret_cast<const float4*>(p)[1];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
    static __device__ __forceinline__ float ld1(const float* p) { return *p; }
};
template <> struct Load8<__half> {
    static __device__ __forceinline__ void ld(const __half* p, float (&v)[8]) {
        union { uint4 u; __half2 h[4]; } x;
        x.u = *reinterpret_cast<const uint4*>(p);
#pragma unroll
        for (int i = 0; i < 4; ++i) { const float2 f = __half22float2(x.h[i]); v[2 * i] = f.x; v[2 * i + 1] = f.y; }
    }
    static __device__ __forceinline__ float ld1(const __half* p) { return __half2float(*p); }
};
template <> struct Load8<__hip_bfloat16> {
    static __device__ __forceinline__ void ld(const __hip_bfloat16* p, float (&v)[8]) {
        const uint4 x = *reinterpret_cast<const uint4*>(p);
        const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[2 * i] = __uint_as_float(w[i] << 16); v[2 * i + 1] = __uint_as_float(w[i] & 0xFFFF0000u); }
    }
    static __device__ __forceinline__ float ld1(const __hip_bfloat16* p) { return __bfloat162float(*p); }
};

// Decision thresholds of y = int(norm.cdf(float64(z)) * 2) (extract.py:83-84), found by bisection against the
// reference's scipy (tests/golden/extract_recover.json `_thresholds`):
//   y >= 1  <=>  z >= -6.957291061679417e-17      y == 2  <=>  z >= 8.292361075813597
// For fp32/fp16/bf16 inputs the comparison is done in fp32 against the smallest float >= the double threshold,
// which is equivalent for every representable input.
#define GSW_Y1_THR (-6.957291061679417e-17)
#define GSW_Y2_THR (8.292361075813597)

struct Thr {
    float y1f, y2f;     // float-compare form (generic vote)
    uint32_t nz_add;    // packed-integer form (wave vote): t + nz_add sets the top bit of the field iff |z| > T1, where T1 is the
                        // largest magnitude with int(cdf(-|z|)*2) == 1  (0 for fp16: every non-zero half is far beyond it)
    uint32_t sat_bits;  // smallest magnitude bit pattern with z >= Y2 (also below inf/NaN patterns)
};

// cipher byte of 8 consecutive elements, MSB-first (extract.py:86), plus error flags
__device__ __forceinline__ uint32_t quantise8(const float (&v)[8], const Thr& t, uint32_t& flags) {
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        c |= (v[k] >= t.y1f ? 1u : 0u) << (7 - k);
        if (v[k] >= t.y2f) flags |= GSW_FLAG_SATURATED;
        if (v[k] != v[k]) flags |= GSW_FLAG_NAN;
    }
    return c;
}
__device__ __forceinline__ uint32_t quantise8d(const double (&v)[8], uint32_t& flags) {
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        c |= (v[k] >= GSW_Y1_THR ? 1u : 0u) << (7 - k);
        if (v[k] >= GSW_Y2_THR) flags |= GSW_FLAG_SATURATED;
        if (v[k] != v[k]) flags |= GSW_FLAG_NAN;
    }
    return c;
}

// Sources of the latent being voted on.
// Packed-integer view used by the wave-per-image vote: one cipher byte = 8 consecutive elements =
//   16-bit types: 4 words (2 elements per word, element 2i in the low half of word i)
//   fp32        : 8 words
// fp64 inputs are mapped to an fp32 surrogate that makes the same three decisions (>= Y1, >= Y2, NaN).
template <typename T> struct WordsOf { static constexpr int NW = 8; static constexpr bool PK16 = false; };
template <> struct WordsOf<__half> { static constexpr int NW = 4; static constexpr bool PK16 = true; };
template <> struct WordsOf<__hip_bfloat16> { static constexpr int NW = 4; static constexpr bool PK16 = true; };

template <typename InT>
struct SrcPlain {  // z read from HBM
    typedef InT elem_t;
    const InT* z;
    __device__ __forceinline__ void words(size_t off, uint32_t (&w)[WordsOf<InT>::NW]) const {
        const uint4* p = reinterpret_cast<const uint4*>(z + off);
        const uint4 a = p[0];
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
        if constexpr (WordsOf<InT>::NW == 8) { const uint4 b = p[1]; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w; }
    }
    __device__ __forceinline__ uint32_t byte8(size_t off, const Thr& t, uint32_t& flags) const {
        float v[8];
        Load8<InT>::ld(z + off, v);
        return quantise8(v, t, flags);
    }
    __device__ __forceinline__ uint32_t bit1(size_t off, const Thr& t, uint32_t& flags) const {
        const float v = Load8<InT>::ld1(z + off);
        if (v >= t.y2f) flags |= GSW_FLAG_SATURATED;
        if (v != v) flags |= GSW_FLAG_NAN;
        return v >= t.y1f ? 1u : 0u;
    }
};
template <>
struct SrcPlain<double> {
    typedef double elem_t;
    const double* z;
    __device__ __forceinline__ void words(size_t off, uint32_t (&w)[8]) const {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double2 d = reinterpret_cast<const double2*>(z + off)[i];
            const double v[2] = {d.x, d.y};
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                float sgt = v[j] >= GSW_Y1_THR ? (v[j] >= GSW_Y2_THR ? 16.0f : 1.0f) : -1.0f;
                if (v[j] != v[j]) sgt = __uint_as_float(0x7FC00000u);
                w[2 * i + j] = __float_as_uint(sgt);
            }
        }
    }
    __device__ __forceinline__ uint32_t byte8(size_t off, const Thr&, uint32_t& flags) const {
        double v[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) { const double2 d = reinterpret_cast<const double2*>(z + off)[i]; v[2 * i] = d.x; v[2 * i + 1] = d.y; }
        return quantise8d(v, flags);
    }
    __device__ __forceinline__ uint32_t bit1(size_t off, const Thr&, uint32_t& flags) const {
        const double v = z[off];
        if (v >= GSW_Y2_THR) flags |= GSW_FLAG_SATURATED;
        if (v != v) flags |= GSW_FLAG_NAN;
        return v >= GSW_Y1_THR ? 1u : 0u;
    }
};

template <typename T> __device__ __forceinline__ float round_to(float x);
template <> __device__ __forceinline__ float round_to<float>(float x) { return x; }
template <> __device__ __forceinline__ float round_to<__half>(float x) { return __half2float(__float2half_rn(x)); }
template <> __device__ __forceinline__ float round_to<__hip_bfloat16>(float x) { return __bfloat162float(__float2bfloat16(x)); }

template <typename T> struct Store8;
template <> struct Store8<float> {
    static __device__ __forceinline__ void st(float* p, const float (&v)[8]) {
        reinterpret_cast<float4*>(p)[0] = make_float4(v[0], v[1], v[2], v[3]);
        reinterpret_cast<float4*>(p)[1] = make_float4(v[4], v[5], v[6], v[7]);
    }
};
template <> struct Store8<__half> {
    static __device__ __forceinline__ void st(__half* p, const float (&v)[8]) {
        union { uint4 u; __half2 h[4]; } x;
#pragma unroll
        for (int i = 0; i < 4; ++i) x.h[i] = __floats2half2_rn(v[2 * i], v[2 * i + 1]);
        *reinterpret_cast<uint4*>(p) = x.u;
    }
};
template <> struct Store8<__hip_bfloat16> {
    static __device__ __forceinline__ void st(__hip_bfloat16* p, const float (&v)[8]) {
        union { uint4 u; __hip_bfloat16 h[8]; } x;
#pragma unroll
        for (int i = 0; i < 8; ++i) x.h[i] = __float2bfloat16(v[i]);
        *reinterpret_cast<uint4*>(p) = x.u;
    }
};

// z = a x + b e of a DDIM update, in fp32 and as ONE value for every kernel that forms it.  The empty asm keeps hipcc from folding the conversion to fp16 into the
// multiply-add (v_fma_mixlo_f16 rounds the exact sum once; the fp32 sum rounded again differs from that next to a tie), which it did in some inlined copies and
// not in others: the fused last step (SrcDdim) and gsw_ddim_step then stored different bits for the same operands.
static __device__ __forceinline__ float ddim_z(float a, float x, float b, float e) {
    float z = fmaf(b, e, a * x);
    asm volatile("" : "+v"(z));
    return z;
}

template <typename T>
struct SrcDdim {  // z = round_T(a*x + b*e): the last inversion step fused into the vote
    typedef T elem_t;
    const T* x;
    const T* e;
    T* zout;  // nullable
    float a, b;
    __device__ __forceinline__ void words(size_t off, uint32_t (&w)[WordsOf<T>::NW]) const {
        float xv[8], ev[8], zv[8];
        Load8<T>::ld(x + off, xv);
        Load8<T>::ld(e + off, ev);
#pragma unroll
        for (int k = 0; k < 8; ++k) zv[k] = ddim_z(a, xv[k], b, ev[k]);
        if constexpr (std::is_same<T, float>::value) {
#pragma unroll
            for (int k = 0; k < 8; ++k) w[k] = __float_as_uint(zv[k]);
        } else if constexpr (std::is_same<T, __half>::value) {
#pragma unroll
            for (int i = 0; i < 4; ++i) { union { __half2 h; uint32_t u; } c; c.h = __floats2half2_rn(zv[2 * i], zv[2 * i + 1]); w[i] = c.u; }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) { union { __hip_bfloat16 h[2]; uint32_t u; } c; c.h[0] = __float2bfloat16(zv[2 * i]); c.h[1] = __float2bfloat16(zv[2 * i + 1]); w[i] = c.u; }
        }
        if (zout) {
            uint4* q = reinterpret_cast<uint4*>(zout + off);
            q[0] = make_uint4(w[0], w[1], w[2], w[3]);
            if constexpr (WordsOf<T>::NW == 8) q[1] = make_uint4(w[4], w[5], w[6], w[7]);
        }
    }
    __device__ __forceinline__ uint32_t byte8(size_t off, const Thr& t, uint32_t& flags) const {
        float xv[8], ev[8], zv[8];
        Load8<T>::ld(x + off, xv);
        Load8<T>::ld(e + off, ev);
#pragma unroll
        for (int k = 0; k < 8; ++k) zv[k] = round_to<T>(ddim_z(a, xv[k], b, ev[k]));
        if (zout) Store8<T>::st(zout + off, zv);
        return quantise8(zv, t, flags);
    }
    __device__ __forceinline__ uint32_t bit1(size_t off, const Thr& t, uint32_t& flags) const {
        const float v = round_to<T>(ddim_z(a, Load8<T>::ld1(x + off), b, Load8<T>::ld1(e + off)));
        if (zout) {
            float tmp = v;
            if constexpr (sizeof(T) == 4) reinterpret_cast<float*>(zout)[off] = tmp;
            else if constexpr (std::is_same<T, __half>::value) zout[off] = __float2half_rn(tmp);
            else zout[off] = __float2bfloat16(tmp);
        }
        if (v >= t.y2f) flags |= GSW_FLAG_SATURATED;
        if (v != v) flags |= GSW_FLAG_NAN;
        return v >= t.y1f ? 1u : 0u;
    }
};
// input streams a source reads per element (the register budget of the extract kernels' load batches)
template <typename S> struct SrcStreams { static constexpr int n = 1; };
template <typename T> struct SrcStreams<SrcDdim<T>> { static constexpr int n = 2; };

struct ExtractArgs {
    GswCipher ck;
    uint8_t* bits;     // [B][ceil(M/8)]
    uint32_t* counts;  // [B][M] or nullptr
    uint32_t* flags;   // [B]
    uint32_t n_elems;  // N
    uint32_t msg_bits; // M
    int32_t B;
    Thr thr;
};

// Spread the 8 bits of a byte (MSB-first: bit 7 belongs to the first element of the group) into 8 byte-wide
// counters held as two u32: lo lane k (k = 0..3) <- bit (7-k), hi lane k <- bit (3-k).
__device__ __forceinline__ void spread_bits(uint32_t byte, uint32_t& lo, uint32_t& hi) {
    const uint32_t x = byte * 0x01010101u;                                  // byte replicated in all 4 lanes
    lo = (((x & 0x10204080u) + 0x70604000u) >> 7) & 0x01010101u;            // lane k keeps bit (7-k); +pad carries a set bit into bit 7
    hi = (((x & 0x01020408u) + 0x7F7E7C78u) >> 7) & 0x01010101u;            // lane k keeps bit (3-k)
}

typedef unsigned short gsw_us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b) {
    const gsw_us2 r = __builtin_elementwise_max(__builtin_bit_cast(gsw_us2, a), __builtin_bit_cast(gsw_us2, b));
    return __builtin_bit_cast(uint32_t, r);
}

// "cipher bit is 0" indicators of one 8-element group as byte lanes (lane k of n_lo = element k, of n_hi = element 4+k),
// from the raw bit patterns: element is a 0-bit  <=>  sign set and |z| > T1  (y = int(cdf(z)*2) == 0, extract.py:83-84).
// Pure VALU integer work: no compare -> SGPR -> select round trips.  tmax tracks the largest magnitude pattern seen.
template <bool PK16, int NW>
__device__ __forceinline__ void negbits8(const uint32_t (&w)[NW], uint32_t nz_add, uint32_t& n_lo, uint32_t& n_hi, uint32_t& tmax) {
    uint32_t n[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const uint32_t t = w[i] & (PK16 ? 0x7FFF7FFFu : 0x7FFFFFFFu);
        n[i] = w[i] & (t + nz_add);                       // top bit of each field: negative AND beyond T1
        tmax = PK16 ? pk_max_u16(tmax, t) : max(tmax, t);
    }
    if (PK16) {   // high bytes of the 8 halves -> [e0 e1 e2 e3], [e4 e5 e6 e7]
        n_lo = __builtin_amdgcn_perm(n[1], n[0], 0x07050301u);
        n_hi = __builtin_amdgcn_perm(n[3], n[2], 0x07050301u);
    } else {      // top bytes of the 8 words
        const uint32_t a = __builtin_amdgcn_perm(n[1], n[0], 0x0C0C0703u);   // [n0.b3, n1.b3, 0, 0]
        const uint32_t b = __builtin_amdgcn_perm(n[3], n[2], 0x0C0C0703u);
        const uint32_t c = __builtin_amdgcn_perm(n[5], n[4], 0x0C0C0703u);
        const uint32_t d = __builtin_amdgcn_perm(n[7], n[6], 0x0C0C0703u);
        n_lo = __builtin_amdgcn_perm(b, a, 0x05040100u);
        n_hi = __builtin_amdgcn_perm(d, c, 0x05040100u);
    }
    n_lo = (n_lo >> 7) & 0x01010101u;
    n_hi = (n_hi >> 7) & 0x01010101u;
}

// exact flags of one image (rare path: only when a magnitude >= the saturation pattern was seen)
template <typename Src>
__device__ __forceinline__ uint32_t wave_exact_flags(const Src& src, size_t base, uint32_t nbytes, const Thr& thr, uint32_t lane) {
    uint32_t f = 0;
    for (uint32_t j = lane; j < nbytes; j += 64) (void)src.byte8(base + ((size_t)j << 3), thr, f);
    for (int s = 32; s > 0; s >>= 1) f |= __shfl_xor(f, s, 64);
    return f;
}

// Wave-per-image vote.  Requires N % 8 == 0, M % 8 == 0, N % M == 0, Mb = M/8 a power of two <= 64*NSETS, N/M <= 65535.
//   * LDS (per workgroup, filled once): ChaCha20 keystream of the whole lattice, then its bitwise complement in "spread"
//     form (8 bytes per cipher byte), so that plaintext-bit byte lanes = negbits ^ spread(~keystream) is two XORs.
//   * every wave owns whole images: lane L reads cipher bytes j = L + 64 r (16 B of fp16 per load, 1 KiB per wave
//     instruction), which all vote for message byte (L + 64 (r % NSETS)) % Mb  ->  per-lane counters, no atomics and no
//     barriers in the image loop; lanes sharing a message byte are combined with __shfl_xor at the end.
template <typename Src, int NSETS>
__global__ __launch_bounds__(1024) void gsw_extract_wave_kernel(ExtractArgs p, Src src) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    typedef typename Src::elem_t T;
    constexpr int NW = WordsOf<T>::NW;
    constexpr bool PK16 = WordsOf<T>::PK16;
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    const uint32_t N = p.n_elems, M = p.msg_bits;
    const uint32_t nbytes = N >> 3;
    const uint32_t nblk = (nbytes + 63u) >> 6;
    const uint32_t Mb = M >> 3;
    uint32_t* ks_words = lds;
    uint2* nks = reinterpret_cast<uint2*>(lds + nblk * 16u);   // spread(~keystream byte j)

    chacha20_blocks_to_lds(GSW_CIPHER_REGS(p.ck), 0u, nblk, ks_words);
    __syncthreads();
    {
        const uint8_t* ksb = reinterpret_cast<const uint8_t*>(ks_words);
        for (uint32_t j = tid; j < nbytes; j += blockDim.x) {
            uint32_t lo, hi;
            spread_bits((~(uint32_t)ksb[j]) & 0xFFu, lo, hi);
            nks[j] = make_uint2(lo, hi);
        }
    }
    __syncthreads();

    const uint32_t nseg = N / M;
    const uint32_t waves_per_wg = blockDim.x >> 6;
    const uint32_t wave_global = blockIdx.x * waves_per_wg + (tid >> 6);
    const uint32_t wave_stride = gridDim.x * waves_per_wg;
    const uint32_t rounds = (nbytes + 63u) >> 6;

    for (uint32_t b = wave_global; b < (uint32_t)p.B; b += wave_stride) {
        const size_t base = (size_t)b * N;
        uint32_t acc[NSETS][2];      // 8-bit lanes, flushed every 255 rounds
        uint32_t wide[NSETS][4];     // 16-bit fields: [0] = elements 0,2  [1] = 1,3  [2] = 4,6  [3] = 5,7
#pragma unroll
        for (int s = 0; s < NSETS; ++s) { acc[s][0] = acc[s][1] = 0; wide[s][0] = wide[s][1] = wide[s][2] = wide[s][3] = 0; }
        uint32_t tmax = 0, in_acc = 0;
        // cipher bytes per lane per batch: 32 data VGPRs in flight -- 16 for the fused last step on fp32 latents with four counter sets (two input streams of 8 words
        // per byte + 24 counters: at the 128 registers of a 1024-thread workgroup that instantiation spilled 13)
        constexpr int QB = (NSETS >= 4 && NW == 8 && SrcStreams<Src>::n == 2) ? 2 : 32 / NW;
        constexpr int PER_SET = QB / NSETS;
        for (uint32_t r0 = 0; r0 < rounds; r0 += QB) {
            uint32_t w[QB][NW];
            // issue all loads of this batch first (QB independent 16/32-byte loads per lane in flight)
#pragma unroll
            for (int q = 0; q < QB; ++q) {
                const uint32_t j = lane + 64u * (r0 + q);
                if (j < nbytes) src.words(base + ((size_t)j << 3), w[q]);
                else {
#pragma unroll
                    for (int i = 0; i < NW; ++i) w[q][i] = 0;
                }
            }
#pragma unroll
            for (int q = 0; q < QB; ++q) {
                const uint32_t j = lane + 64u * (r0 + q);
                uint32_t n_lo, n_hi;
                negbits8<PK16, NW>(w[q], p.thr.nz_add, n_lo, n_hi, tmax);
                if (j < nbytes) {
                    const uint2 k = nks[j];
                    acc[q % NSETS][0] += n_lo ^ k.x;
                    acc[q % NSETS][1] += n_hi ^ k.y;
                }
            }
            in_acc += PER_SET;
            if (in_acc > 255u - PER_SET) {
#pragma unroll
                for (int s = 0; s < NSETS; ++s) {
                    wide[s][0] += acc[s][0] & 0x00FF00FFu; wide[s][1] += (acc[s][0] >> 8) & 0x00FF00FFu;
                    wide[s][2] += acc[s][1] & 0x00FF00FFu; wide[s][3] += (acc[s][1] >> 8) & 0x00FF00FFu;
                    acc[s][0] = acc[s][1] = 0;
                }
                in_acc = 0;
            }
        }
        // saturation / NaN: decided exactly on the rare path only
        const uint32_t tm = PK16 ? max(tmax & 0xFFFFu, tmax >> 16) : tmax;
        uint32_t flags = 0;
        if (__any(tm >= p.thr.sat_bits)) flags = wave_exact_flags(src, base, nbytes, p.thr, lane);
        if (lane == 0) p.flags[b] = flags;
#pragma unroll
        for (int s = 0; s < NSETS; ++s) {
            wide[s][0] += acc[s][0] & 0x00FF00FFu; wide[s][1] += (acc[s][0] >> 8) & 0x00FF00FFu;
            wide[s][2] += acc[s][1] & 0x00FF00FFu; wide[s][3] += (acc[s][1] >> 8) & 0x00FF00FFu;
            // lanes L, L+Mb, L+2Mb, ... (< 64) vote for the same message byte
            for (uint32_t sh = Mb; sh < 64u; sh <<= 1) {
#pragma unroll
                for (int i = 0; i < 4; ++i) wide[s][i] += __shfl_xor(wide[s][i], (int)sh, 64);
            }
            const uint32_t mbyte = lane + 64u * s;
            if (mbyte < Mb) {
                // element k of the group = message bit 8*mbyte + k
                const uint32_t c[8] = {wide[s][0] & 0xFFFFu, wide[s][1] & 0xFFFFu, wide[s][0] >> 16, wide[s][1] >> 16,
                                       wide[s][2] & 0xFFFFu, wide[s][3] & 0xFFFFu, wide[s][2] >> 16, wide[s][3] >> 16};
                uint32_t byte = 0;
#pragma unroll
                for (int k = 0; k < 8; ++k) byte |= (2u * c[k] > nseg ? 1u : 0u) << (7 - k);   // strict majority, ties -> 0
                p.bits[(size_t)b * Mb + mbyte] = (uint8_t)byte;
                if (p.counts) {
                    uint4* cp = reinterpret_cast<uint4*>(p.counts + (size_t)b * M + 8u * mbyte);
                    cp[0] = make_uint4(c[0], c[1], c[2], c[3]);
                    cp[1] = make_uint4(c[4], c[5], c[6], c[7]);
                }
            }
        }
    }
}

// Generic vote: any N (incl. N % 8 != 0, where the reference right-aligns the trailing partial byte, extract.py:86)
// and any M with 8*ceil(N/8) % M == 0.  LDS: [keystream][decrypted plaintext bytes][vote bits M/32 words]
template <typename Src>
__global__ __launch_bounds__(GSW_WG) void gsw_extract_generic_kernel(ExtractArgs p, Src src) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t tid = threadIdx.x;
    const uint32_t N = p.n_elems, M = p.msg_bits;
    const uint32_t nbytes = (N + 7u) >> 3;
    const uint32_t nblk = (nbytes + 63u) >> 6;
    const uint32_t out_bytes = (M + 7u) >> 3;
    const uint32_t out_words = (M + 31u) >> 5;
    uint32_t* ks_words = lds;
    uint8_t* pt = reinterpret_cast<uint8_t*>(lds + nblk * 16u);
    uint32_t* vote = lds + nblk * 16u + ((nbytes + 3u) >> 2);
    __shared__ uint32_t s_flags;

    chacha20_blocks_to_lds(GSW_CIPHER_REGS(p.ck), 0u, nblk, ks_words);
    const uint8_t* ksb = reinterpret_cast<const uint8_t*>(ks_words);
    const uint32_t nseg = (nbytes * 8u) / M;

    for (int b = blockIdx.x; b < p.B; b += gridDim.x) {
        for (uint32_t i = tid; i < out_words; i += GSW_WG) vote[i] = 0;
        if (tid == 0) s_flags = 0;
        __syncthreads();
        const size_t base = (size_t)b * N;
        uint32_t flags = 0;
        for (uint32_t j = tid; j < nbytes; j += GSW_WG) {
            const uint32_t e = j << 3;
            uint32_t cb = 0;
            if (e + 8u <= N && ((base + e) & 7u) == 0) {
                cb = src.byte8(base + e, p.thr, flags);
            } else {
                const uint32_t r = min(8u, N - e);  // trailing partial group: int('b0..b(r-1)', 2) => right-aligned
                for (uint32_t k = 0; k < r; ++k) cb |= src.bit1(base + e + k, p.thr, flags) << (r - 1u - k);
            }
            pt[j] = (uint8_t)(cb ^ ksb[j]);
        }
        if (__any(flags != 0)) {
            uint32_t f = flags;
            for (int s = 32; s > 0; s >>= 1) f |= __shfl_xor(f, s, 64);
            if ((tid & 63u) == 0) atomicOr(&s_flags, f);
        }
        __syncthreads();
        for (uint32_t m = tid; m < M; m += GSW_WG) {
            uint32_t c1 = 0;
            uint32_t idx = m;
            for (uint32_t c = 0; c < nseg; ++c, idx += M) c1 += (pt[idx >> 3] >> (7u - (idx & 7u))) & 1u;
            if (2u * c1 > nseg) atomicOr(&vote[m >> 5], 1u << (m & 31u));
            if (p.counts) p.counts[(size_t)b * M + m] = c1;
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

// X3 alone: the cipher bytes of the quantised signs (no decryption, no vote), the operand of the keyed registry search (gswm_keyed.hip).
// One thread per byte; the flags of an image are OR-ed into flags_out[b], which the caller zeroes.
template <typename Src>
__global__ __launch_bounds__(GSW_WG) void gsw_sign_pack_kernel(Src src, Thr thr, uint8_t* __restrict__ signs, uint32_t* __restrict__ flags_out,
                                                               uint32_t nbytes, int B) {
    const uint32_t j = blockIdx.x * GSW_WG + threadIdx.x;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        uint32_t flags = 0;
        if (j < nbytes) {
            const size_t byte = (size_t)b * nbytes + j;
            signs[byte] = (uint8_t)src.byte8(byte << 3, thr, flags);
        }
        if (__any(flags != 0)) {
            uint32_t f = flags;
            for (int s = 32; s > 0; s >>= 1) f |= __shfl_xor(f, s, 64);
            if ((threadIdx.x & 63u) == 0) atomicOr(&flags_out[b], f);
        }
    }
}

// X6: matches between recovered bits and the reference message over the first nb bits
__global__ __launch_bounds__(64) void gsw_bit_matches_kernel(const uint8_t* __restrict__ bits, uint32_t row_bytes,
                                                            const uint8_t* __restrict__ ref, uint32_t nb, uint32_t* __restrict__ matches, int B) {
    const int b = blockIdx.x;
    if (b >= B) return;
    uint32_t m = 0;
    const uint32_t full = nb >> 3;
    for (uint32_t i = threadIdx.x; i < full; i += 64) m += 8u - __popc((uint32_t)(bits[(size_t)b * row_bytes + i] ^ ref[i]));
    if (threadIdx.x == 0 && (nb & 7u)) {
        const uint32_t mask = (0xFF00u >> (nb & 7u)) & 0xFFu;
        m += (nb & 7u) - __popc((uint32_t)((bits[(size_t)b * row_bytes + full] ^ ref[full]) & mask));
    }
    for (int s = 32; s > 0; s >>= 1) m += __shfl_xor(m, s, 64);
    if (threadIdx.x == 0) matches[b] = m;
}

// ------------------------------------------------------------------------------------------------
// DDIM elementwise update: out = a*x + b*e   (fp32 math, one rounding); HBM-bound: 3 * sizeof(T) bytes / element
// ------------------------------------------------------------------------------------------------
template <typename T, bool CFG>
__global__ __launch_bounds__(GSW_WG) void gsw_ddim_step_kernel(const T* __restrict__ x, const T* __restrict__ e0, const T* __restrict__ e1,
                                                              T* __restrict__ out, float a, float b, float g, uint64_t n) {
    const uint64_t nvec = n >> 3;
    const uint64_t stride = (uint64_t)gridDim.x * GSW_WG;
    for (uint64_t i = (uint64_t)blockIdx.x * GSW_WG + threadIdx.x; i < nvec; i += stride) {
        float xv[8], ev[8], zv[8];
        Load8<T>::ld(x + (i << 3), xv);
        Load8<T>::ld(e0 + (i << 3), ev);
        if (CFG) {
            float tv[8];
            Load8<T>::ld(e1 + (i << 3), tv);
#pragma unroll
            for (int k = 0; k < 8; ++k) ev[k] = fmaf(g, tv[k] - ev[k], ev[k]);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) zv[k] = ddim_z(a, xv[k], b, ev[k]);
        Store8<T>::st(out + (i << 3), zv);
    }
    // tail (< 8 elements)
    if (blockIdx.x == 0) {
        for (uint64_t i = (nvec << 3) + threadIdx.x; i < n; i += GSW_WG) {
            float ev = Load8<T>::ld1(e0 + i);
            if (CFG) { const float tv = Load8<T>::ld1(e1 + i); ev = fmaf(g, tv - ev, ev); }
            const float z = ddim_z(a, Load8<T>::ld1(x + i), b, ev);
            if constexpr (sizeof(T) == 4) reinterpret_cast<float*>(out)[i] = z;
            else if constexpr (std::is_same<T, __half>::value) out[i] = __float2half_rn(z);
            else out[i] = __float2bfloat16(z);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// DPM-Solver++ multistep update, the whole scheduler step in one pass:
//   e = CFG ? e0 + g (e1 - e0) : e0;  m0 = round_T(P x + Q e);  x' = round_T(A x + B m0 + (ORDER2 ? C m_prev : 0))
// fp32 math; m0 is formed by ddim_z like every other x0 prediction / DDIM update and enters the update AS STORED, so the next step's m_prev is the value
// this step used.  HBM-bound: (2 + CFG + ORDER2) streams in, 2 out.  x_out may alias x and m_out may alias m_prev (no __restrict__ on those four: m0 does
// not depend on m_prev, so a restrict-qualified m_out store could legally move above the m_prev load); a thread reads all it needs before it writes.
// ------------------------------------------------------------------------------------------------
static __device__ __forceinline__ float dpm_x(float A, float x, float B, float m0, float C, float mp, bool order2) {
    float z = fmaf(B, m0, A * x);
    if (order2) z = fmaf(C, mp, z);
    asm volatile("" : "+v"(z));      // as ddim_z: the conversion to T stays a second rounding in every copy
    return z;
}

template <typename T> static __device__ __forceinline__ void store1(T* p, float v) {
    if constexpr (sizeof(T) == 4) *reinterpret_cast<float*>(p) = v;
    else if constexpr (std::is_same<T, __half>::value) *p = __float2half_rn(v);
    else *p = __float2bfloat16(v);
}

template <typename T, bool CFG, bool ORDER2>
__global__ __launch_bounds__(GSW_WG) void gsw_dpm_step_kernel(const T* x, const T* __restrict__ e0, const T* __restrict__ e1, const T* m_prev,
                                                             T* x_out, T* m_out, float P, float Q, float A, float B, float C, float g, uint64_t n) {
    const uint64_t nvec = n >> 3;
    const uint64_t stride = (uint64_t)gridDim.x * GSW_WG;
    for (uint64_t i = (uint64_t)blockIdx.x * GSW_WG + threadIdx.x; i < nvec; i += stride) {
        float xv[8], ev[8], pv[8], mv[8], zv[8];
        Load8<T>::ld(x + (i << 3), xv);
        Load8<T>::ld(e0 + (i << 3), ev);
        if (CFG) {
            float tv[8];
            Load8<T>::ld(e1 + (i << 3), tv);
#pragma unroll
            for (int k = 0; k < 8; ++k) ev[k] = fmaf(g, tv[k] - ev[k], ev[k]);
        }
        if (ORDER2) Load8<T>::ld(m_prev + (i << 3), pv);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            mv[k] = round_to<T>(ddim_z(P, xv[k], Q, ev[k]));
            zv[k] = dpm_x(A, xv[k], B, mv[k], C, ORDER2 ? pv[k] : 0.f, ORDER2);
        }
        Store8<T>::st(x_out + (i << 3), zv);
        Store8<T>::st(m_out + (i << 3), mv);
    }
    // tail (< 8 elements)
    if (blockIdx.x == 0) {
        for (uint64_t i = (nvec << 3) + threadIdx.x; i < n; i += GSW_WG) {
            float ev = Load8<T>::ld1(e0 + i);
            if (CFG) { const float tv = Load8<T>::ld1(e1 + i); ev = fmaf(g, tv - ev, ev); }
            const float xs = Load8<T>::ld1(x + i);
            const float mp = ORDER2 ? Load8<T>::ld1(m_prev + i) : 0.f;
            const float m0 = round_to<T>(ddim_z(P, xs, Q, ev));
            store1<T>(x_out + i, dpm_x(A, xs, B, m0, C, mp, ORDER2));
            store1<T>(m_out + i, m0);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// UNet elementwise fusions (rows X2 / G1: the eps model's non-GEMM traffic).  rocprofv3 of the SD2.1-shaped UNet on
// PyTorch-ROCm shows ~30 % of the forward in elementwise / normalisation kernels; these two remove the largest pieces.
//
// gsw_groupnorm_silu: y = act( GroupNorm(x + pre_bias[b,c]) * gamma[c] + beta[c] ), NCHW, one workgroup per (image, group).
//   A group's channels are adjacent in NCHW, so its data is ONE contiguous chunk of (C/G)*HW elements: the chunk is read
//   once from HBM into registers (<= 40960 elements per workgroup), mean and centred variance are computed exactly in fp32,
//   and the normalised + activated values are written straight back -- 2 passes over HBM instead of the 5-6 of
//   moments / apply / SiLU (/ broadcast add) as separate kernels.  Larger chunks re-read from L2 for the second pass.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float block_sum(float v, float* red /* >= 16 floats of LDS */) {
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    const uint32_t wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63u) == 0) red[wid] = v;
    __syncthreads();
    float t = 0.f;
    for (uint32_t i = 0; i < nw; ++i) t += red[i];
    return t;
}

__device__ __forceinline__ float silu_f(float x) { return x / (1.0f + __expf(-x)); }

template <typename T, int MAXV>   // MAXV = max 8-element vectors held per thread (0: always re-read)
__global__ __launch_bounds__(256) void gsw_groupnorm_silu_kernel(const T* __restrict__ x, const T* __restrict__ pre_bias, const T* __restrict__ gamma,
                                                                 const T* __restrict__ beta, T* __restrict__ y, uint32_t C, uint32_t HW, uint32_t G,
                                                                 float eps, int act) {
    __shared__ float red[16];
    const uint32_t bg = blockIdx.x;                 // image * G + group
    const uint32_t b = bg / G, g = bg - b * G;
    const uint32_t cpg = C / G;
    const size_t base = ((size_t)b * C + (size_t)g * cpg) * HW;
    const uint32_t n = cpg * HW;                    // elements of the chunk; HW % 8 == 0 is required by the host wrapper
    const uint32_t nvec = n >> 3;
    const uint32_t tid = threadIdx.x;
    float vals[MAXV > 0 ? MAXV : 1][8];
    float sum = 0.f;
    // pass 1: load (+ per-channel pre-bias), accumulate the sum
#pragma unroll
    for (int i = 0; i < (MAXV > 0 ? MAXV : 1); ++i) {
        const uint32_t v = tid + i * 256u;
        if (MAXV > 0 && v < nvec) {
            Load8<T>::ld(x + base + ((size_t)v << 3), vals[i]);
            if (pre_bias) {
                const float pb = Load8<T>::ld1(pre_bias + (size_t)b * C + g * cpg + (v << 3) / HW);
#pragma unroll
                for (int k = 0; k < 8; ++k) vals[i][k] += pb;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) sum += vals[i][k];
        }
    }
    if (MAXV == 0) {
        for (uint32_t v = tid; v < nvec; v += 256u) {
            float t[8];
            Load8<T>::ld(x + base + ((size_t)v << 3), t);
            const float pb = pre_bias ? Load8<T>::ld1(pre_bias + (size_t)b * C + g * cpg + (v << 3) / HW) : 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) sum += t[k] + pb;
        }
    }
    const float mean = block_sum(sum, red) / (float)n;
    float sq = 0.f;
    if (MAXV > 0) {
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const uint32_t v = tid + i * 256u;
            if (v < nvec) {
#pragma unroll
                for (int k = 0; k < 8; ++k) { const float d = vals[i][k] - mean; sq += d * d; }
            }
        }
    } else {
        for (uint32_t v = tid; v < nvec; v += 256u) {
            float t[8];
            Load8<T>::ld(x + base + ((size_t)v << 3), t);
            const float pb = pre_bias ? Load8<T>::ld1(pre_bias + (size_t)b * C + g * cpg + (v << 3) / HW) : 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) { const float d = t[k] + pb - mean; sq += d * d; }
        }
    }
    const float rstd = rsqrtf(block_sum(sq, red) / (float)n + eps);
    // pass 2: normalise, affine, activation, store
    auto emit = [&](uint32_t v, const float (&in)[8]) {
        const uint32_t c = g * cpg + (v << 3) / HW;
        const float ga = Load8<T>::ld1(gamma + c) * rstd;
        const float be = Load8<T>::ld1(beta + c) - mean * ga;
        float o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { const float t = fmaf(in[k], ga, be); o[k] = act ? silu_f(t) : t; }
        Store8<T>::st(y + base + ((size_t)v << 3), o);
    };
    if (MAXV > 0) {
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const uint32_t v = tid + i * 256u;
            if (v < nvec) emit(v, vals[i]);
        }
    } else {
        for (uint32_t v = tid; v < nvec; v += 256u) {
            float t[8];
            Load8<T>::ld(x + base + ((size_t)v << 3), t);
            if (pre_bias) {
                const float pb = Load8<T>::ld1(pre_bias + (size_t)b * C + g * cpg + (v << 3) / HW);
#pragma unroll
                for (int k = 0; k < 8; ++k) t[k] += pb;
            }
            emit(v, t);
        }
    }
}

// gsw_geglu: out[t, i] = in[t, i] * gelu(in[t, I + i])   (exact erf GELU, fp32 math): one pass instead of gelu + mul
template <typename T>
__global__ __launch_bounds__(256) void gsw_geglu_kernel(const T* __restrict__ in, T* __restrict__ out, uint64_t rows, uint32_t I) {
    const uint32_t vpr = I >> 3;                          // vectors per output row
    const uint64_t nvec = rows * vpr;
    for (uint64_t v = (uint64_t)blockIdx.x * 256u + threadIdx.x; v < nvec; v += (uint64_t)gridDim.x * 256u) {
        const uint64_t r = v / vpr;
        const uint32_t c = (uint32_t)(v - r * vpr) << 3;
        float h[8], gt[8], o[8];
        Load8<T>::ld(in + r * 2u * I + c, h);
        Load8<T>::ld(in + r * 2u * I + I + c, gt);
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = h[k] * (0.5f * gt[k] * (1.0f + erff(gt[k] * 0.70710678118654752f)));
        Store8<T>::st(out + r * I + c, o);
    }
}

// ================================================================================================
// host side of the C ABI
// ================================================================================================
// ---------------------------------------------------------------------------------------------------------------------------
// E4 in bit-parity mode -- gs_insert.py:62 `np.random.uniform(0, 1)` (nodes.py:114-117 `rng.uniform(0, 1)`): NumPy's legacy MT19937
// `random_sample`, continued on the device from a host-supplied generator state so that the uniforms never cross PCIe.
// MT19937 is one serial stream (the reference draws image after image from ONE generator), so this is a single workgroup: the
// 624-word twist runs as three data-parallel phases (k < 227 | k < 454 | k < 624: each phase only reads words the previous
// phases finished), tempering and the 53-bit double (a >> 5, b >> 6) are element-parallel.  Throughput mode uses Philox instead.
// ---------------------------------------------------------------------------------------------------------------------------
struct Mt19937State { uint32_t key[624]; };

__device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

__global__ __launch_bounds__(256) void gsw_mt19937_kernel(Mt19937State st, int32_t pos, double* __restrict__ out, int64_t n, uint32_t* __restrict__ state_out) {
    __shared__ uint32_t mt[624];
    const int tid = threadIdx.x;
    {
        typedef const uint32_t __attribute__((address_space(4))) * kernarg_words;       // the state is kernel argument 0
        kernarg_words ka = (kernarg_words)__builtin_amdgcn_kernarg_segment_ptr();
        for (int i = tid; i < 624; i += 256) mt[i] = ka[i];
    }
    __syncthreads();
    int64_t o = 0;              // doubles written so far
    int wpos = pos;             // next unconsumed word of the current block (624 = block exhausted)
    bool has_carry = false;     // an unpaired high word is waiting for the first word of the next block
    uint32_t carry = 0;
    while (o < n) {
        if (wpos >= 624) {
            // genrand twist, in place: new[k] = old_or_new[(k + 397) % 624] ^ f(old[k], old[(k + 1) % 624])
            for (int ph = 0; ph < 3; ++ph) {
                const int lo = ph * 227, hi = ph == 2 ? 624 : lo + 227;
                const int k = lo + tid;
                uint32_t v = 0;
                if (k < hi) {
                    const int kn = k == 623 ? 0 : k + 1, km = k + 397 >= 624 ? k + 397 - 624 : k + 397;
                    const uint32_t y = (mt[k] & 0x80000000u) | (mt[kn] & 0x7fffffffu);
                    v = mt[km] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
                }
                __syncthreads();
                if (k < hi) mt[k] = v;
                __syncthreads();
            }
            wpos = 0;
        }
        int first = wpos;       // first word of the first (a, b) pair taken wholly from this block
        if (has_carry) {
            if (tid == 0) out[o] = ((double)(carry >> 5) * 67108864.0 + (double)(mt_temper(mt[0]) >> 6)) / 9007199254740992.0;
            o += 1;
            first = 1;
            has_carry = false;
        }
        const int64_t want = n - o;
        const int pairs_avail = (624 - first) >> 1;
        const int pairs = (int)(want < (int64_t)pairs_avail ? want : (int64_t)pairs_avail);
        for (int i = tid; i < pairs; i += 256) {
            const uint32_t a = mt_temper(mt[first + 2 * i]) >> 5, b = mt_temper(mt[first + 2 * i + 1]) >> 6;
            out[o + i] = ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
        }
        o += pairs;
        wpos = first + 2 * pairs;
        if (o < n && wpos == 623) {          // odd leftover and more to draw: its partner is word 0 of the next block
            carry = mt_temper(mt[623]);
            has_carry = true;
            wpos = 624;
        }
        __syncthreads();
    }
    if (state_out) {
        for (int i = tid; i < 624; i += 256) state_out[i] = mt[i];
        if (tid == 0) state_out[624] = (uint32_t)wpos;
    }
}

__attribute__((visibility("hidden"))) thread_local int g_last_hip_error = 0;   // declared in gswm_host.h; shared with gswm_conv.hip / gswm_image.hip

static inline uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

static GswCipher make_cipher(const uint8_t key[32], const uint8_t nonce16[16]) {
    GswCipher c;
    for (int i = 0; i < 8; ++i) c.key[i] = le32(key + 4 * i);
    for (int i = 0; i < 4; ++i) c.nonce[i] = le32(nonce16 + 4 * i);
    return c;
}

static Thr make_thr(int dtype) {
    Thr t;
    float f = (float)GSW_Y1_THR;
    if ((double)f < GSW_Y1_THR) f = nextafterf(f, INFINITY);   // smallest float >= Y1
    t.y1f = f;
    float g = (float)GSW_Y2_THR;
    if ((double)g < GSW_Y2_THR) g = nextafterf(g, INFINITY);   // smallest float >= Y2
    t.y2f = g;
    // integer form: T1 = bit pattern of the largest magnitude m with -m >= Y1; SAT = pattern of the smallest value >= Y2
    float m = (float)(-GSW_Y1_THR);
    if ((double)m > -GSW_Y1_THR) m = nextafterf(m, 0.0f);
    uint32_t t1_32, sat_32;
    memcpy(&t1_32, &m, 4);
    memcpy(&sat_32, &g, 4);
    switch (dtype) {
        case GSW_F16:   // every non-zero half (>= 2^-24) is beyond T1; 8.296875 = 0x4826 is the smallest half >= Y2
            t.nz_add = 0x7FFFu * 0x00010001u; t.sat_bits = 0x4826u; break;
        case GSW_BF16: {  // bf16 = top 16 bits of the float pattern: truncation gives the largest bf16 <= m; round SAT up
            const uint32_t t1 = t1_32 >> 16;
            const uint32_t sat = (sat_32 >> 16) + ((sat_32 & 0xFFFFu) ? 1u : 0u);
            t.nz_add = (0x7FFFu - t1) * 0x00010001u; t.sat_bits = sat; break;
        }
        default:        // fp32, and the fp32 surrogate of fp64 inputs (-1 / +1 / +16 / NaN)
            t.nz_add = 0x7FFFFFFFu - t1_32; t.sat_bits = sat_32; break;
    }
    return t;
}

// The public functions below get C linkage from their declarations in include/gswm.h.

int gsw_version(void) { return GSW_VERSION; }

const char* gsw_strerror(int s) {
    switch (s) {
        case GSW_OK: return "ok";
        case GSW_ERR_BAD_ARG: return "bad argument";
        case GSW_ERR_UNSUPPORTED: return "unsupported lattice / message geometry";
        case GSW_ERR_RAGGED: return "padded lattice bit count is not a multiple of message_length (reference raises IndexError)";
        case GSW_ERR_HIP: return "HIP runtime error";
        case GSW_WARN_NO_RECORDS: return "the launch wrote no statistics records for the armed request (split-K / whole-tensor / off-engine launch)";
        default: return "unknown status";
    }
}

int gsw_last_hip_error(void) { return g_last_hip_error; }

int gsw_keystream(const uint8_t key[32], const uint8_t nonce16[16], uint8_t* out_dev, size_t nbytes, void* stream) {
    if (!key || !nonce16 || (!out_dev && nbytes)) return GSW_ERR_BAD_ARG;
    if (nbytes == 0) return GSW_OK;
    const GswCipher ck = make_cipher(key, nonce16);
    const uint64_t nblocks = (nbytes + 63) / 64;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((nblocks + 63) / 64, (uint64_t)device_cus() * 8);
    hipLaunchKernelGGL(gsw_keystream_kernel, dim3(grid), dim3(GSW_WG), 0, (hipStream_t)stream, ck, out_dev, (uint64_t)nbytes);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

template <typename OutT>
static void launch_embed(const EmbedArgs& a, bool has_u, bool fast, bool bitmsg, dim3 grid, hipStream_t st) {
#define GSW_LAUNCH_E(HU, F) \
    do { if (bitmsg) hipLaunchKernelGGL((gsw_embed_kernel<OutT, HU, F, true>), grid, dim3(GSW_WG), 0, st, a); \
         else hipLaunchKernelGGL((gsw_embed_kernel<OutT, HU, F, false>), grid, dim3(GSW_WG), 0, st, a); } while (0)
    if (has_u) { if (fast) GSW_LAUNCH_E(true, true); else GSW_LAUNCH_E(true, false); }
    else       { if (fast) GSW_LAUNCH_E(false, true); else GSW_LAUNCH_E(false, false); }
#undef GSW_LAUNCH_E
}

// message bits need not be a multiple of 8 on this internal entry; the public one takes whole bytes
static int embed_impl(const uint8_t key[32], const uint8_t nonce16[16], const uint8_t* msg, int msg_bits, const double* u_dev,
                      uint64_t seed, uint64_t image_index0, void* out_dev, int out_dtype, int B, int64_t n_elems, uint32_t flags,
                      void* stream) {
    if (!key || !nonce16 || !msg || msg_bits <= 0 || !out_dev || B < 0 || n_elems <= 0 || (n_elems & 3)) return GSW_ERR_BAD_ARG;
    if (n_elems > (int64_t)0x7FFFFFF0) return GSW_ERR_UNSUPPORTED;
    if (out_dtype < GSW_F32 || out_dtype > GSW_F64) return GSW_ERR_BAD_ARG;
    if (B == 0) return GSW_OK;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t msg_bytes = (uint32_t)(msg_bits + 7) / 8;
    EmbedArgs a;
    memset(&a, 0, sizeof(a));
    a.ck = make_cipher(key, nonce16);
    uint8_t* staged = nullptr;
    if (msg_bytes <= GSW_MSG_INLINE_MAX) {
        memcpy(a.msg.b, msg, msg_bytes);
    } else {
        GSW_HIP(hipMallocAsync((void**)&staged, msg_bytes, st));
        GSW_HIP(hipMemcpyAsync(staged, msg, msg_bytes, hipMemcpyHostToDevice, st));
        // the host buffer may be pageable: the copy above is then synchronous w.r.t. the host, which is what lets the
        // caller reuse `msg` immediately
        a.msg_dev = staged;
    }
    a.u = u_dev;
    a.out = out_dev;
    a.seed = seed;
    a.image_index0 = image_index0;
    a.n_elems = (uint32_t)n_elems;
    a.msg_bytes = msg_bytes;
    a.msg_bits = (uint32_t)msg_bits;
    a.lim_elems = (uint32_t)((n_elems / msg_bits) * msg_bits);
    a.B = B;
    const uint32_t nchunks = (uint32_t)((n_elems + GSW_CHUNK - 1) / GSW_CHUNK);
    // enough workgroups to fill 256 CUs x 8, but never more image-groups than images
    uint32_t G = (uint32_t)std::max<int64_t>(1, std::min<int64_t>(B, ((int64_t)device_cus() * 8 + nchunks - 1) / nchunks));
    G = std::min<uint32_t>(G, 65535u);
    const dim3 grid(nchunks, G);
    const bool fast = (flags & GSW_EMBED_FAST_F32) != 0;
    const bool bitmsg = (msg_bits & 7) != 0;
    switch (out_dtype) {
        case GSW_F32: launch_embed<float>(a, u_dev != nullptr, fast, bitmsg, grid, st); break;
        case GSW_F16: launch_embed<__half>(a, u_dev != nullptr, fast, bitmsg, grid, st); break;
        case GSW_BF16: launch_embed<__hip_bfloat16>(a, u_dev != nullptr, fast, bitmsg, grid, st); break;
        default: launch_embed<double>(a, u_dev != nullptr, fast, bitmsg, grid, st); break;
    }
    hipError_t le = hipGetLastError();
    if (staged) (void)hipFreeAsync(staged, st);
    if (le != hipSuccess) return hip_fail(le);
    return GSW_OK;
}

int gsw_embed(const uint8_t key[32], const uint8_t nonce16[16], const uint8_t* msg, int msg_bytes, const double* u_dev,
              uint64_t seed, uint64_t image_index0, void* out_dev, int out_dtype, int B, int64_t n_elems, uint32_t flags,
              void* stream) {
    if (msg_bytes <= 0 || msg_bytes > (1 << 27)) return GSW_ERR_BAD_ARG;
    return embed_impl(key, nonce16, msg, msg_bytes * 8, u_dev, seed, image_index0, out_dev, out_dtype, B, n_elems, flags, stream);
}

int gsw_philox_uniform(uint64_t seed, uint64_t image_index0, double* u_dev, int B, int64_t n_elems, void* stream) {
    if (!u_dev || B < 0 || n_elems <= 0 || n_elems > (int64_t)0x7FFFFFF0) return GSW_ERR_BAD_ARG;
    if (B == 0) return GSW_OK;
    const uint32_t ngroups = (uint32_t)((n_elems + 3) / 4);
    const dim3 grid(std::min<uint32_t>((ngroups + GSW_WG - 1) / GSW_WG, 1024u), (uint32_t)std::min<int>(B, 65535));
    hipLaunchKernelGGL(gsw_philox_uniform_kernel, grid, dim3(GSW_WG), 0, (hipStream_t)stream, u_dev, seed, image_index0, B, (uint32_t)n_elems);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

void gsw_mt19937_seed(uint32_t seed, uint32_t key[624]) {
    // numpy/random/src/mt19937/mt19937.c mt19937_seed: what RandomState(seed=int) / np.random.seed(int) run; pos starts at 624
    for (int pos = 0; pos < 624; ++pos) {
        key[pos] = seed;
        seed = 1812433253u * (seed ^ (seed >> 30)) + (uint32_t)pos + 1u;
    }
}

int gsw_mt19937_uniform(const uint32_t key[624], int pos, double* u_dev, int64_t n, uint32_t* state_out_dev, void* stream) {
    if (!key || !u_dev || n < 0 || pos < 0 || pos > 624) return GSW_ERR_BAD_ARG;
    if (n == 0 && !state_out_dev) return GSW_OK;
    Mt19937State st;
    memcpy(st.key, key, sizeof(st.key));
    hipLaunchKernelGGL(gsw_mt19937_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, st, (int32_t)pos, u_dev, n, state_out_dev);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

#define GSW_MAX_DYN_LDS (160u * 1024u - 64u)

template <typename Src, int NSETS>
static int launch_extract_wave(const ExtractArgs& a, const Src& src, size_t lds, hipStream_t st) {
    // big batches: 1024-thread workgroups (16 waves share one keystream fill, 2 workgroups per CU);
    // small batches: 256-thread workgroups so that the images spread over more CUs
    const uint32_t block = a.B >= 2048 ? 1024u : 256u;
    const uint32_t waves = block / 64u;
    const uint32_t max_grid = (uint32_t)device_cus() * (2048u / block);
    const uint32_t grid = std::max<uint32_t>(1u, std::min<uint32_t>(((uint32_t)a.B + waves - 1u) / waves, max_grid));
    GSW_HIP(allow_dynamic_lds((const void*)gsw_extract_wave_kernel<Src, NSETS>, lds));
    hipLaunchKernelGGL((gsw_extract_wave_kernel<Src, NSETS>), dim3(grid), dim3(block), lds, st, a, src);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

// gsw_extract votes wave-per-image (gsw_extract_wave_kernel) for these geometries and through the generic kernel otherwise.  The two agree on
// every element but a NaN, which the wave vote counts by its sign bit (fp64: as 1) and the generic vote as 0; gsw_extract_keyed asks here
// to count a flagged image's NaNs as gsw_extract does.
static bool extract_votes_by_wave(uint32_t N, uint32_t M) {
    const uint32_t nbytes = (N + 7u) / 8u;
    const uint32_t nblk = (nbytes + 63u) / 64u;
    const uint32_t Mb = M / 8u;
    const size_t lds_wave = (size_t)nblk * 64u + (size_t)nbytes * 8u;
    return (N % 8u == 0) && (M % 8u == 0) && Mb >= 1 && Mb <= 256u && (256u % Mb == 0) && (N % M == 0) &&
           (N / M <= 65535u) && lds_wave <= GSW_MAX_DYN_LDS;
}

template <typename Src>
static int launch_extract(const ExtractArgs& a, const Src& src, hipStream_t st) {
    const uint32_t N = a.n_elems, M = a.msg_bits;
    const uint32_t nbytes = (N + 7u) / 8u;
    const uint32_t nblk = (nbytes + 63u) / 64u;
    const uint32_t Mb = M / 8u;
    const size_t lds_wave = (size_t)nblk * 64u + (size_t)nbytes * 8u;
    const bool fast = extract_votes_by_wave(N, M);
    if (fast) {
        if (Mb <= 64u) return launch_extract_wave<Src, 1>(a, src, lds_wave, st);
        if (Mb == 128u) return launch_extract_wave<Src, 2>(a, src, lds_wave, st);
        return launch_extract_wave<Src, 4>(a, src, lds_wave, st);
    }
    const uint32_t grid = (uint32_t)std::min<int64_t>(a.B, (int64_t)device_cus() * 8);
    const size_t lds = (size_t)nblk * 64u + (size_t)((nbytes + 3u) / 4u) * 4u + (size_t)((M + 31u) / 32u) * 4u;
    if (lds > GSW_MAX_DYN_LDS) return GSW_ERR_UNSUPPORTED;
    GSW_HIP(allow_dynamic_lds((const void*)gsw_extract_generic_kernel<Src>, lds));
    hipLaunchKernelGGL((gsw_extract_generic_kernel<Src>), dim3(grid), dim3(GSW_WG), lds, st, a, src);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

static int extract_check(const uint8_t* key, const uint8_t* nonce16, int msg_bits, uint8_t* bits_dev, uint32_t* flags_dev, int B,
                         int64_t n_elems, int dtype, ExtractArgs& a) {
    if (!key || !nonce16 || msg_bits <= 0 || !bits_dev || !flags_dev || B < 0 || n_elems <= 0) return GSW_ERR_BAD_ARG;
    if (n_elems > (int64_t)0x7FFFFFF0) return GSW_ERR_UNSUPPORTED;
    const int64_t padded_bits = ((n_elems + 7) / 8) * 8;
    if (padded_bits % msg_bits) return GSW_ERR_RAGGED;
    memset(&a, 0, sizeof(a));
    a.ck = make_cipher(key, nonce16);
    a.bits = bits_dev;
    a.flags = flags_dev;
    a.n_elems = (uint32_t)n_elems;
    a.msg_bits = (uint32_t)msg_bits;
    a.B = B;
    a.thr = make_thr(dtype);
    return GSW_OK;
}

int gsw_extract(const void* z_dev, int z_dtype, const uint8_t key[32], const uint8_t nonce16[16], int msg_bits,
                uint8_t* bits_dev, uint32_t* counts_dev, uint32_t* flags_dev, int B, int64_t n_elems, void* stream) {
    if (!z_dev) return GSW_ERR_BAD_ARG;
    ExtractArgs a;
    const int rc = extract_check(key, nonce16, msg_bits, bits_dev, flags_dev, B, n_elems, z_dtype, a);
    if (rc != GSW_OK) return rc;
    if (B == 0) return GSW_OK;
    a.counts = counts_dev;
    hipStream_t st = (hipStream_t)stream;
    switch (z_dtype) {
        case GSW_F32: return launch_extract(a, SrcPlain<float>{(const float*)z_dev}, st);
        case GSW_F16: return launch_extract(a, SrcPlain<__half>{(const __half*)z_dev}, st);
        case GSW_BF16: return launch_extract(a, SrcPlain<__hip_bfloat16>{(const __hip_bfloat16*)z_dev}, st);
        case GSW_F64: return launch_extract(a, SrcPlain<double>{(const double*)z_dev}, st);
        default: return GSW_ERR_BAD_ARG;
    }
}

template <typename Src>
static int launch_sign_pack(const Src& src, int dtype, uint8_t* signs_dev, uint32_t* flags_dev, int B, uint32_t nbytes, hipStream_t st) {
    GSW_HIP(hipMemsetAsync(flags_dev, 0, (size_t)B * sizeof(uint32_t), st));
    const dim3 grid((nbytes + GSW_WG - 1) / GSW_WG, (uint32_t)std::min(B, 65535));
    hipLaunchKernelGGL((gsw_sign_pack_kernel<Src>), grid, dim3(GSW_WG), 0, st, src, make_thr(dtype), signs_dev, flags_dev, nbytes, B);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

int gsw_sign_pack(const void* z_dev, int z_dtype, uint8_t* signs_dev, uint32_t* flags_dev, int B, int64_t n_elems, void* stream) {
    if (!z_dev || !signs_dev || !flags_dev || B < 0 || n_elems < 1) return GSW_ERR_BAD_ARG;
    if (z_dtype != GSW_F32 && z_dtype != GSW_F16 && z_dtype != GSW_BF16 && z_dtype != GSW_F64) return GSW_ERR_BAD_ARG;
    if ((n_elems & 7) || n_elems > (int64_t)0x7FFFFFF0) return GSW_ERR_UNSUPPORTED;
    if (B == 0) return GSW_OK;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t nbytes = (uint32_t)(n_elems / 8);
    switch (z_dtype) {
        case GSW_F32: return launch_sign_pack(SrcPlain<float>{(const float*)z_dev}, z_dtype, signs_dev, flags_dev, B, nbytes, st);
        case GSW_F16: return launch_sign_pack(SrcPlain<__half>{(const __half*)z_dev}, z_dtype, signs_dev, flags_dev, B, nbytes, st);
        case GSW_BF16: return launch_sign_pack(SrcPlain<__hip_bfloat16>{(const __hip_bfloat16*)z_dev}, z_dtype, signs_dev, flags_dev, B, nbytes, st);
        default: return launch_sign_pack(SrcPlain<double>{(const double*)z_dev}, z_dtype, signs_dev, flags_dev, B, nbytes, st);
    }
}

int gsw_ddim_step_extract(const void* x_dev, const void* model_out_dev, void* z_out_dev, float ca, float cb, int dtype,
                          const uint8_t key[32], const uint8_t nonce16[16], int msg_bits, uint8_t* bits_dev,
                          uint32_t* counts_dev, uint32_t* flags_dev, int B, int64_t n_elems, void* stream) {
    if (!x_dev || !model_out_dev) return GSW_ERR_BAD_ARG;
    ExtractArgs a;
    const int rc = extract_check(key, nonce16, msg_bits, bits_dev, flags_dev, B, n_elems, dtype, a);
    if (rc != GSW_OK) return rc;
    if (B == 0) return GSW_OK;
    a.counts = counts_dev;
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
        case GSW_F32: return launch_extract(a, SrcDdim<float>{(const float*)x_dev, (const float*)model_out_dev, (float*)z_out_dev, ca, cb}, st);
        case GSW_F16: return launch_extract(a, SrcDdim<__half>{(const __half*)x_dev, (const __half*)model_out_dev, (__half*)z_out_dev, ca, cb}, st);
        case GSW_BF16: return launch_extract(a, SrcDdim<__hip_bfloat16>{(const __hip_bfloat16*)x_dev, (const __hip_bfloat16*)model_out_dev, (__hip_bfloat16*)z_out_dev, ca, cb}, st);
        default: return GSW_ERR_BAD_ARG;
    }
}

int gsw_bit_matches(const uint8_t* bits_dev, int msg_bits, const uint8_t* ref_msg, int ref_bits, uint32_t* matches_dev, int B, void* stream) {
    if (!bits_dev || !ref_msg || !matches_dev || msg_bits <= 0 || ref_bits <= 0 || B < 0) return GSW_ERR_BAD_ARG;
    if (B == 0) return GSW_OK;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t nb = (uint32_t)std::min(msg_bits, ref_bits);
    const uint32_t ref_bytes = (nb + 7u) / 8u;
    uint8_t* ref_dev = nullptr;
    GSW_HIP(hipMallocAsync((void**)&ref_dev, ref_bytes, st));
    GSW_HIP(hipMemcpyAsync(ref_dev, ref_msg, ref_bytes, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(gsw_bit_matches_kernel, dim3(B), dim3(64), 0, st, bits_dev, (uint32_t)((msg_bits + 7) / 8), (const uint8_t*)ref_dev, nb, matches_dev, B);
    hipError_t le = hipGetLastError();
    (void)hipFreeAsync(ref_dev, st);
    if (le != hipSuccess) return hip_fail(le);
    return GSW_OK;
}

template <typename T>
static int launch_ddim(const void* x, const void* e0, const void* e1, void* out, float a, float b, float g, int64_t n, hipStream_t st) {
    const uint64_t nvec = (uint64_t)n >> 3;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((nvec + GSW_WG - 1) / GSW_WG, (uint64_t)device_cus() * 8));
    if (e1) hipLaunchKernelGGL((gsw_ddim_step_kernel<T, true>), dim3(grid), dim3(GSW_WG), 0, st, (const T*)x, (const T*)e0, (const T*)e1, (T*)out, a, b, g, (uint64_t)n);
    else    hipLaunchKernelGGL((gsw_ddim_step_kernel<T, false>), dim3(grid), dim3(GSW_WG), 0, st, (const T*)x, (const T*)e0, (const T*)nullptr, (T*)out, a, b, g, (uint64_t)n);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

static int ddim_dispatch(const void* x, const void* e0, const void* e1, void* out, float a, float b, float g, int dtype, int64_t n, void* stream) {
    if (!x || !e0 || !out || n < 0) return GSW_ERR_BAD_ARG;
    if (n == 0) return GSW_OK;
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
        case GSW_F32: return launch_ddim<float>(x, e0, e1, out, a, b, g, n, st);
        case GSW_F16: return launch_ddim<__half>(x, e0, e1, out, a, b, g, n, st);
        case GSW_BF16: return launch_ddim<__hip_bfloat16>(x, e0, e1, out, a, b, g, n, st);
        default: return GSW_ERR_BAD_ARG;
    }
}

int gsw_ddim_step(const void* x_dev, const void* model_out_dev, void* out_dev, float a, float b, int dtype, int64_t n, void* stream) {
    return ddim_dispatch(x_dev, model_out_dev, nullptr, out_dev, a, b, 0.0f, dtype, n, stream);
}

int gsw_ddim_step_cfg(const void* x_dev, const void* e_uncond_dev, const void* e_text_dev, void* out_dev, float a, float b,
                      float guidance, int dtype, int64_t n, void* stream) {
    if (!e_text_dev) return GSW_ERR_BAD_ARG;
    return ddim_dispatch(x_dev, e_uncond_dev, e_text_dev, out_dev, a, b, guidance, dtype, n, stream);
}

template <typename T>
static int launch_dpm(const void* x, const void* e0, const void* e1, const void* mp, void* xo, void* mo, float P, float Q, float A, float B, float C, float g,
                      int64_t n, hipStream_t st) {
    const uint64_t nvec = (uint64_t)n >> 3;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((nvec + GSW_WG - 1) / GSW_WG, (uint64_t)device_cus() * 8));
#define GSW_DPM(CFG, O2) hipLaunchKernelGGL((gsw_dpm_step_kernel<T, CFG, O2>), dim3(grid), dim3(GSW_WG), 0, st, (const T*)x, (const T*)e0, (const T*)e1, \
                                            (const T*)mp, (T*)xo, (T*)mo, P, Q, A, B, C, g, (uint64_t)n)
    if (e1) { if (mp) GSW_DPM(true, true); else GSW_DPM(true, false); }
    else    { if (mp) GSW_DPM(false, true); else GSW_DPM(false, false); }
#undef GSW_DPM
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

int gsw_dpm_step(const void* x_dev, const void* e_uncond_dev, const void* e_text_dev, const void* m_prev_dev, void* x_out_dev, void* m_out_dev,
                 float P, float Q, float A, float B, float C, float guidance, int dtype, int64_t n, void* stream) {
    if (!x_dev || !e_uncond_dev || !x_out_dev || !m_out_dev || n < 0) return GSW_ERR_BAD_ARG;
    if (dtype != GSW_F32 && dtype != GSW_F16 && dtype != GSW_BF16) return GSW_ERR_BAD_ARG;
    if (!m_prev_dev && C != 0.0f) return GSW_ERR_BAD_ARG;
    if (n == 0) return GSW_OK;
    if (C == 0.0f) m_prev_dev = nullptr;      // first order: m_prev is not read at all (0 * NaN would be NaN)
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
        case GSW_F32: return launch_dpm<float>(x_dev, e_uncond_dev, e_text_dev, m_prev_dev, x_out_dev, m_out_dev, P, Q, A, B, C, guidance, n, st);
        case GSW_F16: return launch_dpm<__half>(x_dev, e_uncond_dev, e_text_dev, m_prev_dev, x_out_dev, m_out_dev, P, Q, A, B, C, guidance, n, st);
        default: return launch_dpm<__hip_bfloat16>(x_dev, e_uncond_dev, e_text_dev, m_prev_dev, x_out_dev, m_out_dev, P, Q, A, B, C, guidance, n, st);
    }
}


template <typename T>
static int launch_gn(const void* x, const void* pb, const void* ga, const void* be, void* y, int B, int C, int HW, int G, float eps, int act, hipStream_t st) {
    const uint32_t n = (uint32_t)(C / G) * (uint32_t)HW;
    const uint32_t nvec = n / 8u;
    const dim3 grid((uint32_t)B * (uint32_t)G), block(256);
#define GSW_GN(MV) hipLaunchKernelGGL((gsw_groupnorm_silu_kernel<T, MV>), grid, block, 0, st, (const T*)x, (const T*)pb, (const T*)ga, (const T*)be, (T*)y, \
                                      (uint32_t)C, (uint32_t)HW, (uint32_t)G, eps, act)
    if (nvec <= 256u * 2u) GSW_GN(2);
    else if (nvec <= 256u * 5u) GSW_GN(5);
    else if (nvec <= 256u * 10u) GSW_GN(10);
    else if (nvec <= 256u * 20u) GSW_GN(20);
    else GSW_GN(0);
#undef GSW_GN
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

int gsw_groupnorm_silu(const void* x_dev, const void* pre_bias_dev, const void* gamma_dev, const void* beta_dev, void* out_dev, int B, int C,
                       int HW, int groups, float eps, int act, int dtype, void* stream) {
    if (!x_dev || !gamma_dev || !beta_dev || !out_dev || B < 0 || C <= 0 || HW <= 0 || groups <= 0 || C % groups || (HW & 7)) return GSW_ERR_BAD_ARG;
    if (B == 0) return GSW_OK;
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
        case GSW_F32: return launch_gn<float>(x_dev, pre_bias_dev, gamma_dev, beta_dev, out_dev, B, C, HW, groups, eps, act, st);
        case GSW_F16: return launch_gn<__half>(x_dev, pre_bias_dev, gamma_dev, beta_dev, out_dev, B, C, HW, groups, eps, act, st);
        case GSW_BF16: return launch_gn<__hip_bfloat16>(x_dev, pre_bias_dev, gamma_dev, beta_dev, out_dev, B, C, HW, groups, eps, act, st);
        default: return GSW_ERR_BAD_ARG;
    }
}

int gsw_geglu(const void* in_dev, void* out_dev, int64_t rows, int inner, int dtype, void* stream) {
    if (!in_dev || !out_dev || rows < 0 || inner <= 0 || (inner & 7)) return GSW_ERR_BAD_ARG;
    if (rows == 0) return GSW_OK;
    hipStream_t st = (hipStream_t)stream;
    const uint64_t nvec = (uint64_t)rows * (uint64_t)(inner / 8);
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((nvec + 255) / 256, (uint64_t)device_cus() * 16));
    switch (dtype) {
        case GSW_F32: hipLaunchKernelGGL((gsw_geglu_kernel<float>), dim3(grid), dim3(256), 0, st, (const float*)in_dev, (float*)out_dev, (uint64_t)rows, (uint32_t)inner); break;
        case GSW_F16: hipLaunchKernelGGL((gsw_geglu_kernel<__half>), dim3(grid), dim3(256), 0, st, (const __half*)in_dev, (__half*)out_dev, (uint64_t)rows, (uint32_t)inner); break;
        case GSW_BF16: hipLaunchKernelGGL((gsw_geglu_kernel<__hip_bfloat16>), dim3(grid), dim3(256), 0, st, (const __hip_bfloat16*)in_dev, (__hip_bfloat16*)out_dev, (uint64_t)rows, (uint32_t)inner); break;
        default: return GSW_ERR_BAD_ARG;
    }
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

// ------------------------------------------------------------------------------------------------
// Multi-bit windows (l = 2, 4): gsw_embed_l / gsw_extract_l / gsw_quant_pack, kernels and entry points
// ------------------------------------------------------------------------------------------------
#include "gswm_codec_l.inc"

// ------------------------------------------------------------------------------------------------
// One record per image (every image under its own key, nonce and message): gsw_embed_keyed / gsw_extract_keyed, kernels and entry points
// ------------------------------------------------------------------------------------------------
#include "gswm_codec_keyed.inc"

// ------------------------------------------------------------------------------------------------
// Soft-decision vote (every element weighted by an integer reliability level): gsw_extract_soft, kernel and entry point
// ------------------------------------------------------------------------------------------------
#include "gswm_codec_soft.inc"

// ------------------------------------------------------------------------------------------------
// Soft-decision vote for multi-bit windows (l = 2, 4; a level per cipher bit): gsw_extract_soft_l / gsw_level_pack_l, kernels and entry points
// ------------------------------------------------------------------------------------------------
#include "gswm_codec_soft_l.inc"

// ------------------------------------------------------------------------------------------------
// Error-corrected payloads (rate-1/2, K = 7 convolutional code under the votes): gsw_viterbi_decode, kernel and entry point
// ------------------------------------------------------------------------------------------------
#include "gswm_viterbi_plan.h"
#include "gswm_viterbi_rate_plan.h"   // the punctured codes' plan, for both reads (it brings the list read's plan with it)
#include "gswm_viterbi.inc"

// ------------------------------------------------------------------------------------------------
// The list read of error-corrected payloads (L best paths per state, the CRC picks among them): gsw_viterbi_list_decode, kernel and entry point
// ------------------------------------------------------------------------------------------------
#include "gswm_viterbi_list_plan.h"
#include "gswm_viterbi_list.inc"
