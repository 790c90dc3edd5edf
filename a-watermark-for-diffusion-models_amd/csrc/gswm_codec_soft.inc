// gswm_codec_soft.inc -- the soft-decision vote: every lattice element votes with an integer reliability level taken from its magnitude,
// B images under their own records in one launch (gfx950).  Included at the end of gswm_kernels.hip, after gswm_codec_keyed.inc: records,
// keystream, its LDS staging and the end of the vote are gsw_extract_keyed's own (gswm_record.h), the hard bit q_j is gsw_extract's
// quantiser (quantise8 / quantise8d).  The kernels here are l = 1; the host side at the end of the namespace (one argument struct per operation, level_check /
// vote_check, vote_args / pack_args, launch_vote / launch_pack, with_dtype / with_steps) also serves the l = 2, 4 entry points of gswm_codec_soft_l.inc.
//
// Definition, image b with thresholds thr[b][0 .. levels) (fp32; row b * thr_stride of thr_dev, thr_stride == 0: one row for all), M = 8 msg_bytes:
//   p_j     = q_j ^ ks_j                                  the decrypted bit of element j
//   level_j = #{ i < levels : |z_j| >= thr[b][i] }        0 .. levels, levels in 1 .. 15
//             fp16 / bf16 / fp32: z widened exactly to fp32 and compared there; fp64: compared in fp64 against the thresholds widened to
//             fp64 -- an exact function of the stored bits in every dtype.  NaN: level 0; +-inf: `levels` (finite thresholds); -0.0 is 0.0.
//   score[b, t] = sum over j = t (mod M) of level_j (2 p_j - 1)        wsum[b, t] = the same sum of level_j alone
//   wsq[b]      = sum over j of level_j^2
//   bits: MSB first, bit t = (score > 0); a tie or no weight at all gives 0, gsw_extract's tie rule
//   matches[b]  = how many recovered bits equal record b's message;  flags[b] = gsw_extract's GSW_FLAG_*.  A flagged element still votes
//                 with its level (a saturated one with the top level its magnitude reaches, a NaN with level 0).
// With levels = 1, thr = {0} every non-NaN element has level 1: on NaN-free images score = 2 counts - copies of gsw_extract_keyed and the
// bits are its bits.
//
// Kernel.  gsw_extract_soft_kernel<T, STEPS> : [B] workgroups of 256, ceil(N / 512) x 64 bytes of dynamic LDS (the keystream) + 17.1 KiB static;
// STEPS = bit length of `levels` (1 .. 4).
// The quads write the image's keystream to LDS as in gsw_extract_keyed_kernel.  N % 8 == 0 and M % 8 == 0, so the group of eight elements
// g always meets the message bits 8 (g % msg_bytes) .. + 7.  With R = 256 / msg_bytes (rounded down) the first R msg_bytes threads walk the
// groups tid, tid + R msg_bytes, ...: adjacent lanes load adjacent 16 bytes (fp32: 32, fp64: 64), a thread keeps its octet for the whole
// image and accumulates eight score and eight wsum sums in registers.  The threads of an octet then meet through LDS, one writer per slot:
// 16 x 256 int32.
// The level is a count, so the order of the thresholds does not matter: the first `levels` threads rank the row (ascending, -0.0 == 0.0, ties
// by index, NaNs last -- no magnitude reaches a NaN) into 16 LDS slots padded with NaN, and "thr[i] <= |z|" is then true exactly for the
// first level_j slots.  An element finds that count by bisection, STEPS LDS reads and compares instead of `levels` compares
// (DESIGN.md section 4.16).  Bits come from
// the wave's ballot (eight adjacent lanes hold a byte).  Integer sums throughout: no atomics, no workspace, nothing to zero first, every
// output element written, and the results do not depend on the launch geometry.
//
// gsw_level_pack_kernel<T, STEPS> (further down) is the same quantiser and the same level search without a key: the packed sign row, the bits of
// the levels as STEPS packed planes and the image's sum of levels and of squared levels, the operands of gsw_trace_keyed_soft_topk (DESIGN.md 4.17).

namespace codec_soft {

constexpr int SOFT_MAX_LEVELS = 15;

// the arguments of both vote kernels: gsw_extract_soft_kernel below and gsw_extract_soft_l_kernel (gswm_codec_soft_l.inc); filled by vote_args
struct ExtractSoftArgs {
    const void* z;          // [B][N]
    const uint8_t* records; // [B][stride]
    const float* thr;       // [B][thr_stride] or one table: a row (l = 1), [L][levels] (l = 2, 4)
    uint8_t* bits;          // [B][msg_bytes]
    int32_t* score;         // [B][msg_bits] or nullptr
    int32_t* wsum;          // [B][msg_bits] or nullptr
    int32_t* wsq;           // [B] or nullptr
    uint32_t* flags;        // [B]
    uint32_t* matches;      // [B] or nullptr
    int64_t thr_stride;     // floats
    uint32_t stride;
    uint32_t n_elems;       // N
    uint32_t msg_bytes;     // P
    uint32_t nblk;          // ChaCha blocks that cover the staged row
    uint32_t levels;
    uint32_t q;             // Q = P / gcd(P, l): the groups after which a thread's message bytes repeat (l = 1: P)
    uint32_t reps;          // R = 256 / Q: threads per octet (l = 1), per owner (l = 2, 4)
    Thr quant;              // gsw_extract's quantiser (read at l = 1; the windows of l = 2, 4 are quantised against constants)
};

// eight elements as the type they are compared in (fp32, fp64 for fp64 inputs), their cipher byte and flags by gsw_extract's quantiser
template <typename T> struct Group8 {
    typedef float cmp_t;
    static __device__ __forceinline__ uint32_t ld(const T* p, const Thr& q, float (&v)[8], uint32_t& flags) {
        Load8<T>::ld(p, v);
        return quantise8(v, q, flags);
    }
};
template <> struct Group8<double> {
    typedef double cmp_t;
    static __device__ __forceinline__ uint32_t ld(const double* p, const Thr&, double (&v)[8], uint32_t& flags) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { const double2 d = reinterpret_cast<const double2*>(p)[i]; v[2 * i] = d.x; v[2 * i + 1] = d.y; }
        return quantise8d(v, flags);
    }
};

// The level search, shared by the vote and by gsw_level_pack.
// The first `levels` threads rank the row thr[0 .. levels) into s_thr[16]: ascending, -0.0 == 0.0, ties by index, NaNs last, the padding (NaN)
// after them; the caller's barrier follows.
__device__ __forceinline__ void rank_thresholds(const float* __restrict__ thr, uint32_t levels, float* s_thr, uint32_t tid) {
    if (tid <= (uint32_t)SOFT_MAX_LEVELS) {
        uint32_t rank = tid;                                         // the padding stays where it is
        float t = __uint_as_float(0x7FC00000u);
        if (tid < levels) {
            t = thr[tid];
            rank = 0;
            for (uint32_t j = 0; j < levels; ++j) {
                const float u = thr[j];
                const bool before = t != t ? (u == u || j < tid) : (u < t || (u == t && j < tid));
                rank += before ? 1u : 0u;
            }
        }
        s_thr[rank] = t;
    }
}

// lv[k] = #{ i : |v[k]| >= s_thr[i] } by bisection over the ranked row, STEPS = bit length of `levels`; v is left as |v|
template <int STEPS, typename cmp_t>
__device__ __forceinline__ void levels8(cmp_t (&v)[8], const float* s_thr, uint32_t (&lv)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) { v[k] = fabs(v[k]); lv[k] = 0; }   // NaN stays NaN: no threshold counts it
#pragma unroll
    for (int h = 1 << (STEPS - 1); h > 0; h >>= 1) {                 // slots lv .. lv + h - 1 hold thresholds <= |z| iff the last of them does
#pragma unroll
        for (int k = 0; k < 8; ++k) lv[k] += v[k] >= (cmp_t)s_thr[lv[k] + (uint32_t)h - 1u] ? (uint32_t)h : 0u;
    }
}

template <typename T, int STEPS>
__global__ __launch_bounds__(GSW_WG) void gsw_extract_soft_kernel(ExtractSoftArgs p) {
    typedef typename Group8<T>::cmp_t cmp_t;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];   // the keystream of the image, p.nblk * 16 words
    __shared__ int32_t s_part[16][GSW_WG];                           // [k] score, [8 + k] wsum of every thread's octet
    __shared__ float s_thr[SOFT_MAX_LEVELS + 1];                     // the row in ascending order, NaNs and the padding last
    __shared__ uint32_t s_flags[GSW_WG / 64], s_wsq[GSW_WG / 64];
    __shared__ uint32_t s_match[GSW_MSG_INLINE_MAX];                 // matching bits per message byte
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t b = blockIdx.x;
    const uint32_t N = p.n_elems, P = p.msg_bytes, M = P * 8u;
    const uint8_t* rec = p.records + (int64_t)b * p.stride;
    const uint8_t* row = reinterpret_cast<const uint8_t*>(lds);

    rank_thresholds(p.thr + (int64_t)b * p.thr_stride, p.levels, s_thr, tid);
    record_keystream_to_lds<GSW_WG>(rec, p.nblk, lds);
    __syncthreads();

    const T* z = reinterpret_cast<const T*>(p.z) + (size_t)b * N;
    const uint32_t step = p.reps * P;                                // <= 256, a multiple of msg_bytes: a thread keeps its octet
    int32_t sc[8], ws[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { sc[k] = 0; ws[k] = 0; }
    uint32_t flags = 0, wsq = 0;
    if (tid < step) {
        for (uint32_t g = tid; g < (N >> 3); g += step) {            // N % 8 == 0: whole, 16-byte aligned groups
            cmp_t v[8];
            const uint32_t c = Group8<T>::ld(z + ((size_t)g << 3), p.quant, v, flags) ^ (uint32_t)row[g];
            uint32_t lv[8];
            levels8<STEPS>(v, s_thr, lv);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int32_t w = (int32_t)lv[k];
                sc[k] += (c >> (7 - k)) & 1u ? w : -w;
                ws[k] += w;
                wsq += lv[k] * lv[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) { s_part[k][tid] = sc[k]; s_part[8 + k][tid] = ws[k]; }
    for (int s = 32; s > 0; s >>= 1) { flags |= __shfl_xor(flags, s, 64); wsq += __shfl_xor(wsq, s, 64); }
    if (lane == 0) { s_flags[tid >> 6] = flags; s_wsq[tid >> 6] = wsq; }
    __syncthreads();

    for (uint32_t t0 = 0; t0 < M; t0 += GSW_WG) {                    // the same trip count for every lane: the ballot runs with all lanes on
        const uint32_t t = t0 + tid;
        int32_t s = 0, w = 0;
        if (t < M) {
            for (uint32_t r = 0, th = t >> 3; r < p.reps; ++r, th += P) { s += s_part[t & 7u][th]; w += s_part[8u + (t & 7u)][th]; }
            if (p.score) p.score[(size_t)b * M + t] = s;
            if (p.wsum) p.wsum[(size_t)b * M + t] = w;
        }
        const uint64_t ball = __ballot(t < M && s > 0);              // ties and no weight -> 0
        if (t < M && (t & 7u) == 0) {                                // M % 8 == 0: the seven bits after t are this wave's as well
            const uint32_t v = ballot_byte(ball, lane, 0u);
            p.bits[(size_t)b * P + (t >> 3)] = (uint8_t)v;
            s_match[t >> 3] = 8u - __popc(v ^ (uint32_t)rec[GSW_REC_HEAD + (t >> 3)]);
        }
    }
    __syncthreads();
    store_matches_flags<GSW_WG / 64>(s_match, s_flags, P, p.matches, p.flags, b);
    if (tid == 0 && p.wsq) p.wsq[b] = (int32_t)(s_wsq[0] + s_wsq[1] + s_wsq[2] + s_wsq[3]);
}

// ---- gsw_level_pack: the operands of the level-weighted keyed search (gswm_keyed_soft.inc) -- the sign row of gsw_sign_pack, the bits of the
// levels as P = STEPS packed planes, and the two sums of the levels.  [B] workgroups of 256; thread tid walks the groups of eight elements tid,
// tid + 256, ... and writes one byte of the sign row and of every plane per group (adjacent lanes adjacent bytes).  The quantiser is the vote's
// (Group8), the level search is levels8 above.  Integer sums, reduced by shuffles and one LDS round: no atomics, no workspace, nothing to zero.
// the arguments of both pack kernels: gsw_level_pack_kernel below and gsw_level_pack_l_kernel (gswm_codec_soft_l.inc); filled by pack_args
struct LevelPackArgs {
    const void* z;          // [B][N]
    const float* thr;       // [B][thr_stride] or one table: a row (l = 1), [L][levels] (l = 2, 4)
    uint8_t* signs;         // [B][N l / 8]
    uint8_t* planes;        // [B][STEPS][N l / 8], plane k = bit k of the levels
    int32_t* wsum;          // [B]
    int32_t* wsq;           // [B]
    uint32_t* flags;        // [B]
    int64_t thr_stride;     // floats
    uint32_t n_elems;       // N
    uint32_t levels;
    Thr quant;              // gsw_extract's quantiser (read at l = 1)
};

template <typename T, int STEPS>
__global__ __launch_bounds__(GSW_WG) void gsw_level_pack_kernel(LevelPackArgs p) {
    typedef typename Group8<T>::cmp_t cmp_t;
    __shared__ float s_thr[SOFT_MAX_LEVELS + 1];
    __shared__ uint32_t s_flags[GSW_WG / 64], s_wsum[GSW_WG / 64], s_wsq[GSW_WG / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t b = blockIdx.x;
    const uint32_t N = p.n_elems, nbytes = N >> 3;
    rank_thresholds(p.thr + (int64_t)b * p.thr_stride, p.levels, s_thr, tid);
    __syncthreads();

    const T* z = reinterpret_cast<const T*>(p.z) + (size_t)b * N;
    uint8_t* signs = p.signs + (size_t)b * nbytes;
    uint8_t* planes = p.planes + (size_t)b * STEPS * nbytes;
    uint32_t flags = 0, wsum = 0, wsq = 0;
    for (uint32_t g = tid; g < nbytes; g += GSW_WG) {               // N % 8 == 0: whole, 16-byte aligned groups
        cmp_t v[8];
        signs[g] = (uint8_t)Group8<T>::ld(z + ((size_t)g << 3), p.quant, v, flags);
        uint32_t lv[8];
        levels8<STEPS>(v, s_thr, lv);
        uint32_t pl[STEPS];
#pragma unroll
        for (int s = 0; s < STEPS; ++s) pl[s] = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
#pragma unroll
            for (int s = 0; s < STEPS; ++s) pl[s] |= ((lv[k] >> s) & 1u) << (7 - k);
            wsum += lv[k];
            wsq += lv[k] * lv[k];
        }
#pragma unroll
        for (int s = 0; s < STEPS; ++s) planes[(size_t)s * nbytes + g] = (uint8_t)pl[s];
    }
    for (int s = 32; s > 0; s >>= 1) { flags |= __shfl_xor(flags, s, 64); wsum += __shfl_xor(wsum, s, 64); wsq += __shfl_xor(wsq, s, 64); }
    if (lane == 0) { s_flags[tid >> 6] = flags; s_wsum[tid >> 6] = wsum; s_wsq[tid >> 6] = wsq; }
    __syncthreads();
    if (tid == 0) {
        p.flags[b] = s_flags[0] | s_flags[1] | s_flags[2] | s_flags[3];
        p.wsum[b] = (int32_t)(s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3]);
        p.wsq[b] = (int32_t)(s_wsq[0] + s_wsq[1] + s_wsq[2] + s_wsq[3]);
    }
}

// ---- the host side of the four entry points (l = 1 here, l = 2 and 4 in gswm_codec_soft_l.inc): one check, one filling function per struct, one launch each.

// f(TypeTag<the element type of z_dtype>{}); z_dtype was checked
template <typename T> struct TypeTag { typedef T type; };
template <typename F> static int with_dtype(int z_dtype, F&& f) {
    switch (z_dtype) {
        case GSW_F32: return f(TypeTag<float>{});
        case GSW_F16: return f(TypeTag<__half>{});
        case GSW_BF16: return f(TypeTag<__hip_bfloat16>{});
        default: return f(TypeTag<double>{});
    }
}

// f(std::integral_constant<int, STEPS>{}), STEPS = the bit length of `levels`: 2^STEPS - 1 >= levels
template <typename F> static int with_steps(uint32_t levels, F&& f) {
    if (levels < 2u) return f(std::integral_constant<int, 1>{});
    if (levels < 4u) return f(std::integral_constant<int, 2>{});
    if (levels < 8u) return f(std::integral_constant<int, 3>{});
    return f(std::integral_constant<int, 4>{});
}

// what the entry points ask of z, the table and the lattice, l in {1, 2, 4} (the l entries refuse l = 1 themselves)
static int level_check(const void* z_dev, int z_dtype, const float* thr_dev, int64_t thr_stride, int levels, int l, int64_t n_elems) {
    if (!z_dev || !thr_dev || n_elems < 1) return GSW_ERR_BAD_ARG;
    if (l != 1 && l != 2 && l != 4) return GSW_ERR_BAD_ARG;
    if (z_dtype < GSW_F32 || z_dtype > GSW_F64) return GSW_ERR_BAD_ARG;
    if ((uintptr_t)z_dev & 15u) return GSW_ERR_BAD_ARG;                                      // 16-byte loads
    if ((uintptr_t)thr_dev & 3u) return GSW_ERR_BAD_ARG;
    if (levels < 1 || levels > SOFT_MAX_LEVELS) return GSW_ERR_BAD_ARG;
    if (thr_stride != 0 && thr_stride < (int64_t)l * levels) return GSW_ERR_BAD_ARG;
    if (n_elems % 8 || n_elems * l > GSW_ROW_MAX_BITS) return GSW_ERR_UNSUPPORTED;           // (15^2 n l fits int32 far beyond this)
    return GSW_OK;
}

// the vote's check: the records first, then the outputs that must be there, level_check, and whole copies of the message in the n l bits
static int vote_check(const void* z_dev, int z_dtype, const uint8_t* records_dev, int64_t record_stride, int msg_bytes, const float* thr_dev, int64_t thr_stride,
                      int levels, int l, const uint8_t* bits_dev, const uint32_t* flags_dev, int B, int64_t n_elems) {
    const int rc = records_check32(records_dev, record_stride, msg_bytes, B);
    if (rc != GSW_OK) return rc;
    if (!bits_dev || !flags_dev) return GSW_ERR_BAD_ARG;
    const int lc = level_check(z_dev, z_dtype, thr_dev, thr_stride, levels, l, n_elems);
    if (lc != GSW_OK) return lc;
    return (n_elems * l) % ((int64_t)msg_bytes * 8) ? GSW_ERR_RAGGED : GSW_OK;
}

static ExtractSoftArgs vote_args(const void* z_dev, int z_dtype, const uint8_t* records_dev, int64_t record_stride, int msg_bytes, const float* thr_dev,
                                 int64_t thr_stride, int levels, int l, uint8_t* bits_dev, int32_t* score_dev, int32_t* wsum_dev, int32_t* wsq_dev,
                                 uint32_t* flags_dev, uint32_t* matches_dev, int64_t n_elems) {
    ExtractSoftArgs a;
    memset(&a, 0, sizeof(a));
    a.z = z_dev;
    a.records = records_dev;
    a.thr = thr_dev;
    a.bits = bits_dev;
    a.score = score_dev;
    a.wsum = wsum_dev;
    a.wsq = wsq_dev;
    a.flags = flags_dev;
    a.matches = matches_dev;
    a.thr_stride = thr_stride;
    a.stride = (uint32_t)record_stride;
    a.n_elems = (uint32_t)n_elems;
    a.msg_bytes = (uint32_t)msg_bytes;
    a.nblk = (uint32_t)((n_elems / 8 * l + 63) / 64);
    a.levels = (uint32_t)levels;
    uint32_t gcd = (uint32_t)l;                                      // l is 1, 2 or 4
    while ((uint32_t)msg_bytes % gcd) gcd >>= 1;
    a.q = (uint32_t)msg_bytes / gcd;                                 // <= 256 = GSW_WG: reps is at least 1
    a.reps = (uint32_t)GSW_WG / a.q;
    a.quant = make_thr(z_dtype);
    return a;
}

static LevelPackArgs pack_args(const void* z_dev, int z_dtype, const float* thr_dev, int64_t thr_stride, int levels, uint8_t* signs_dev, uint8_t* planes_dev,
                               int32_t* wsum_dev, int32_t* wsq_dev, uint32_t* flags_dev, int64_t n_elems) {
    LevelPackArgs a;
    memset(&a, 0, sizeof(a));
    a.z = z_dev;
    a.thr = thr_dev;
    a.signs = signs_dev;
    a.planes = planes_dev;
    a.wsum = wsum_dev;
    a.wsq = wsq_dev;
    a.flags = flags_dev;
    a.thr_stride = thr_stride;
    a.n_elems = (uint32_t)n_elems;
    a.levels = (uint32_t)levels;
    a.quant = make_thr(z_dtype);
    return a;
}

// [B] workgroups of 256 with the image's keystream in dynamic LDS; lds_threshold: from where on the kernel must be allowed that much next to its static LDS
static int launch_vote(void (*kernel)(ExtractSoftArgs), uint32_t lds_threshold, const ExtractSoftArgs& a, int B, hipStream_t st) {
    const uint32_t lds = a.nblk * 64u;
    GSW_HIP(allow_dynamic_lds((const void*)kernel, lds, lds_threshold));
    hipLaunchKernelGGL(kernel, dim3((uint32_t)B), dim3(GSW_WG), lds, st, a);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

static int launch_pack(void (*kernel)(LevelPackArgs), const LevelPackArgs& a, int B, hipStream_t st) {
    hipLaunchKernelGGL(kernel, dim3((uint32_t)B), dim3(GSW_WG), 0, st, a);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

}  // namespace codec_soft

int gsw_level_pack(const void* z_dev, int z_dtype, const float* thr_dev, int64_t thr_stride, int levels, uint8_t* signs_dev, uint8_t* planes_dev,
                   int32_t* wsum_dev, int32_t* wsq_dev, uint32_t* flags_dev, int B, int64_t n_elems, void* stream) {
    using namespace codec_soft;
    if (!signs_dev || !planes_dev || !wsum_dev || !wsq_dev || !flags_dev || B < 1) return GSW_ERR_BAD_ARG;
    const int rc = level_check(z_dev, z_dtype, thr_dev, thr_stride, levels, 1, n_elems);
    if (rc != GSW_OK) return rc;
    const LevelPackArgs a = pack_args(z_dev, z_dtype, thr_dev, thr_stride, levels, signs_dev, planes_dev, wsum_dev, wsq_dev, flags_dev, n_elems);
    return with_dtype(z_dtype, [&](auto t) {
        return with_steps(a.levels, [&](auto steps) {
            return launch_pack(gsw_level_pack_kernel<typename decltype(t)::type, decltype(steps)::value>, a, B, (hipStream_t)stream);
        });
    });
}

int gsw_extract_soft(const void* z_dev, int z_dtype, const uint8_t* records_dev, int64_t record_stride, int msg_bytes, const float* thr_dev,
                     int64_t thr_stride, int levels, uint8_t* bits_dev, int32_t* score_dev, int32_t* wsum_dev, int32_t* wsq_dev,
                     uint32_t* flags_dev, uint32_t* matches_dev, int B, int64_t n_elems, void* stream) {
    using namespace codec_soft;
    const int rc = vote_check(z_dev, z_dtype, records_dev, record_stride, msg_bytes, thr_dev, thr_stride, levels, 1, bits_dev, flags_dev, B, n_elems);
    if (rc != GSW_OK) return rc;
    const ExtractSoftArgs a = vote_args(z_dev, z_dtype, records_dev, record_stride, msg_bytes, thr_dev, thr_stride, levels, 1, bits_dev, score_dev, wsum_dev, wsq_dev,
                                        flags_dev, matches_dev, n_elems);
    return with_dtype(z_dtype, [&](auto t) {
        return with_steps(a.levels, [&](auto steps) {                  // 32 KiB: next to 17.1 KiB of static LDS
            return launch_vote(gsw_extract_soft_kernel<typename decltype(t)::type, decltype(steps)::value>, 32u * 1024u, a, B, (hipStream_t)stream);
        });
    });
}
