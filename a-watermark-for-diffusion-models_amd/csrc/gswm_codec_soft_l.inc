// gswm_codec_soft_l.inc -- the soft-decision vote for multi-bit windows (l = 2, 4): every CIPHER BIT of a lattice element votes with an
// integer reliability level, B images under their own records in one launch (gfx950).  Included at the end of gswm_kernels.hip, after
// gswm_codec_soft.inc: records, keystream staging and the end of the vote are gswm_record.h's, the hard window y is gswm_codec_l.inc's
// quantiser (quant1), the ranking of a threshold row is gswm_codec_soft.inc's (rank_thresholds), and so are the argument structs (ExtractSoftArgs,
// LevelPackArgs) and the whole host side of the two entry points at the end of this file.  DESIGN.md section 4.23.
//
// Definition, image b, element e with stored value z (Z = z widened exactly to fp64), y = #{ j : z >= T_j } its window, T = quant_thresholds:
//   window bit w (0 = first = MSB of y, cipher position e l + w) has the value s = 2^(l-1-w) in y and flips exactly at the boundaries T_i, s | i
//   a = (y / s) s        the nearest flip boundary at or below z (none if a == 0)         c = a + s      the nearest above (none if c == 2^l)
//   level(e, w) = #{ i < levels : (a == 0 or Z >= fl64(T_a + t_i)) and (c == 2^l or Z <= fl64(T_c - t_i)) },    t_i = (double)thr[b][w][i]
//   NaN z: level 0.  A NaN threshold never counts.  +-inf: `levels` for finite thresholds.
//   p = (bit w of y) ^ keystream bit (e l + w), t = (e l + w) mod M:  score[b, t] = sum level (2 p - 1), wsum[b, t] = sum level,
//   wsq[b] = sum of level^2 over all Nb = n l bits; bits, matches, flags as gsw_extract_soft.
//
// The edges.  The condition is monotone in t_i (rounding is monotone), so with the row of window bit w ranked ascending (NaNs and the padding
// last) the level is the length of the satisfied prefix, found by bisection with two compares per step.  Once per image the workgroup writes
// the edges into LDS in the compare type (fp32 for fp16 / bf16 / fp32 inputs, fp64 for fp64): lo = the smallest value >= fl64(T_j + t), hi =
// the largest value <= fl64(T_j - t), so that "z >= lo" is "Z >= fl64(T_j + t)" and "z <= hi" is "Z <= fl64(T_j - t)" for every z of the
// compare type.  A side without a boundary holds -inf / +inf (a NaN z still fails it), a NaN threshold or a padding slot holds NaN.  Window
// bit w has 2^(w+1) intervals between neighbouring flip boundaries (m = y >> (l-1-w) = 0 .. 2^(w+1) - 1, from boundary m s to (m + 1) s); interval
// m of bit w is row (2 << w) - 2 + m, 6 rows at l = 2, 30 at l = 4, 16 slots each, a slot the pair (lo of the lower boundary, hi of the upper
// one): one LDS read per bisection step.  The table is stored slot-major, s_edge[slot][row]: the lanes of a wave are at the same step of the
// bisection but in different intervals, and the rows of one slot lie in different LDS banks (lanes in the same interval read one address).
//
// gsw_extract_soft_l_kernel<T, L, STEPS> : [B] workgroups of 256, ceil(N L / 512) x 64 bytes of dynamic LDS (the keystream) + static LDS.
// Ownership.  The group of eight elements g is the cipher bytes g L .. g L + L - 1, which meet the message bytes (g L + i) mod P, P =
// msg_bytes.  With Q = P / gcd(P, L) the start (g L) mod P repeats every Q groups; R = 256 / Q (rounded down); the first R Q threads walk
// the groups tid, tid + R Q, ...: a thread keeps its L message bytes ((tid L + i) mod P, which wrap where L does not divide P) for the whole
// image and accumulates 8 L score and 8 L wsum sums in registers.  The partial sums then meet through LDS in L rounds, one per cipher byte
// i of the group: in round i every thread writes the 16 sums of its byte i to its own column, and message byte m is read from the R columns
// q, q + Q, ... of its owner q = s_own[i][m] (for a fixed i, q -> (q L + i) mod P is one to one on q < Q; a byte that no thread meets as its
// byte i has no owner in that round).  One 16 KiB buffer serves all rounds.  Integer sums throughout: no atomics, no workspace, nothing to
// zero first, every output element written, and the results do not depend on the launch geometry.
//
// gsw_level_pack_l_kernel<T, L, STEPS> : the same quantiser and level search without a key.  Thread tid walks the groups tid, tid + 256, ...
// and writes L bytes of the sign row (gsw_quant_pack's bytes) and L bytes of each of the STEPS planes per group.

namespace codec_soft_l {

using codec_soft::SOFT_MAX_LEVELS;

template <int L> struct Geo {
    static constexpr int FULL = 1 << L;
    static constexpr int ROWS = (2 << L) - 2;                        // sum over w of 2^(w+1)
    static __device__ __forceinline__ constexpr uint32_t row0(int w) { return (uint32_t)((2 << w) - 2); }
};

// (lo, hi) of one slot in the compare type
template <typename F> struct EdgePair { typedef float2 V; };
template <> struct EdgePair<double> { typedef double2 V; };

// a double edge in the compare type, rounded towards the side that keeps the compare exact
template <typename F> struct Edge;
template <> struct Edge<double> {
    static __device__ __forceinline__ double up(double e) { return e; }
    static __device__ __forceinline__ double down(double e) { return e; }
};
template <> struct Edge<float> {
    static __device__ __forceinline__ float up(double e) {            // the smallest float >= e; NaN stays NaN
        float f = (float)e;
        if ((double)f < e) {
            const uint32_t u = __float_as_uint(f);
            f = __uint_as_float((u << 1) == 0u ? 1u : (u >> 31) ? u - 1u : u + 1u);
        }
        return f;
    }
    static __device__ __forceinline__ float down(double e) {          // the largest float <= e
        float f = (float)e;
        if ((double)f > e) {
            const uint32_t u = __float_as_uint(f);
            f = __uint_as_float((u << 1) == 0u ? 0x80000001u : (u >> 31) ? u + 1u : u - 1u);
        }
        return f;
    }
};

template <int L> __device__ __forceinline__ double boundary(uint32_t j) {   // T_j, j in 1 .. 2^L - 1
    if constexpr (L == 2) return GSW_QT_D_L2[j - 1]; else return GSW_QT_D_L4[j - 1];
}

// The image's thresholds thr[L][levels] ranked per window bit into s_thr[L][16], then the edge rows s_edge[16][ROWS].  Ends with a barrier.
template <int L, typename F>
__device__ __forceinline__ void edges_to_lds(const float* __restrict__ thr, uint32_t levels, float (*s_thr)[SOFT_MAX_LEVELS + 1],
                                             typename EdgePair<F>::V (*s_edge)[Geo<L>::ROWS], uint32_t tid) {
#pragma unroll
    for (int w = 0; w < L; ++w) codec_soft::rank_thresholds(thr + (uint32_t)w * levels, levels, s_thr[w], tid - 16u * (uint32_t)w);
    __syncthreads();
    const F nan = (F)__uint_as_float(0x7FC00000u), inf = (F)__builtin_inff();
    for (uint32_t idx = tid; idx < (uint32_t)Geo<L>::ROWS * 16u; idx += GSW_WG) {
        const uint32_t row = idx >> 4, slot = idx & 15u;
        uint32_t w = 0;
#pragma unroll
        for (int x = 1; x < L; ++x) w = row >= Geo<L>::row0(x) ? (uint32_t)x : w;
        const uint32_t a = (row - ((2u << w) - 2u)) << ((uint32_t)L - 1u - w), c = a + (1u << ((uint32_t)L - 1u - w));
        const float t = s_thr[w][slot];
        const bool real = t == t;
        typename EdgePair<F>::V e;
        e.x = a == 0u ? (real ? -inf : nan) : Edge<F>::up(boundary<L>(a) + (double)t);
        e.y = c == (uint32_t)Geo<L>::FULL ? (real ? inf : nan) : Edge<F>::down(boundary<L>(c) - (double)t);
        s_edge[slot][row] = e;
    }
    __syncthreads();
}

// lv[e L + w] = level(e, w) of the eight values v with windows y: the satisfied prefix of the ranked row, by bisection.  Step-major as levels8:
// the 8 L searches of a group are independent, so every step issues 8 L LDS reads before the first compare waits.
template <int L, int STEPS, typename F>
__device__ __forceinline__ void levels_group(const F (&v)[8], const uint32_t (&y)[8], const typename EdgePair<F>::V (*s_edge)[Geo<L>::ROWS],
                                             uint32_t (&lv)[8 * L]) {
    uint32_t row[8 * L];
#pragma unroll
    for (int j = 0; j < 8 * L; ++j) {
        row[j] = Geo<L>::row0(j % L) + (y[j / L] >> (L - 1 - j % L));     // the interval of bit w that holds z
        lv[j] = 0;
    }
#pragma unroll
    for (int h = 1 << (STEPS - 1); h > 0; h >>= 1) {
        typename EdgePair<F>::V e[8 * L];
#pragma unroll
        for (int j = 0; j < 8 * L; ++j) e[j] = s_edge[lv[j] + (uint32_t)h - 1u][row[j]];
#pragma unroll
        for (int j = 0; j < 8 * L; ++j) lv[j] += (v[j / L] >= e[j].x && v[j / L] <= e[j].y) ? (uint32_t)h : 0u;
    }
}

using codec_soft::ExtractSoftArgs;
using codec_soft::LevelPackArgs;

constexpr uint32_t NO_OWNER = 0xFFFFu;
static_assert(GSW_MSG_INLINE_MAX == GSW_WG, "s_own is initialised one column per thread");
constexpr int SOFT_L_TRIPS = GSW_MSG_INLINE_MAX * 8 / GSW_WG;        // message bits per thread at the longest message

template <typename T, int L, int STEPS>
__global__ __launch_bounds__(GSW_WG) void gsw_extract_soft_l_kernel(ExtractSoftArgs p) {
    typedef typename codec_l::QLoad<T>::F F;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];   // the keystream of the image, p.nblk * 16 words
    __shared__ int32_t s_part[16][GSW_WG];                           // one round: [k] score, [8 + k] wsum of every thread's byte i
    __shared__ float s_thr[L][SOFT_MAX_LEVELS + 1];
    __shared__ typename EdgePair<F>::V s_edge[SOFT_MAX_LEVELS + 1][Geo<L>::ROWS];
    __shared__ uint16_t s_own[L][GSW_MSG_INLINE_MAX];                // round i: the first thread that holds message byte m as its byte i
    __shared__ uint32_t s_flags[GSW_WG / 64], s_wsq[GSW_WG / 64];
    __shared__ uint32_t s_match[GSW_MSG_INLINE_MAX];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t b = blockIdx.x;
    const uint32_t N = p.n_elems, P = p.msg_bytes, M = P * 8u, Q = p.q;
    const uint8_t* rec = p.records + (int64_t)b * p.stride;
    const uint8_t* row = reinterpret_cast<const uint8_t*>(lds);

#pragma unroll
    for (int i = 0; i < L; ++i) s_own[i][tid] = (uint16_t)NO_OWNER;  // GSW_MSG_INLINE_MAX == GSW_WG
    record_keystream_to_lds<GSW_WG>(rec, p.nblk, lds);
    edges_to_lds<L, F>(p.thr + (int64_t)b * p.thr_stride, p.levels, s_thr, s_edge, tid);

    const T* z = reinterpret_cast<const T*>(p.z) + (size_t)b * N;
    const uint32_t step = p.reps * Q;                                // <= 256, step L = 0 (mod P): a thread keeps its L message bytes
    int32_t sc[8 * L], ws[8 * L];
#pragma unroll
    for (int j = 0; j < 8 * L; ++j) { sc[j] = 0; ws[j] = 0; }
    uint32_t flags = 0, wsq = 0;
    if (tid < step) {
        for (uint32_t g = tid; g < (N >> 3); g += step) {            // N % 8 == 0: whole, 16-byte aligned groups
            F v[8];
            codec_l::QLoad<T>::ld8(z + ((size_t)g << 3), v);
            uint32_t ks = 0;                                         // the group's L keystream bytes, first byte on top
#pragma unroll
            for (int i = 0; i < L; ++i) ks = (ks << 8) | (uint32_t)row[g * L + i];
            uint32_t y[8], lvs[8 * L], yb = 0;                      // yb: the group's 8 L window bits, first bit on top
#pragma unroll
            for (int e = 0; e < 8; ++e) { y[e] = codec_l::quant1<L, F>(v[e], flags); yb |= y[e] << (L * (7 - e)); }
            levels_group<L, STEPS, F>(v, y, s_edge, lvs);
            const uint32_t pb = yb ^ ks;
#pragma unroll
            for (int j = 0; j < 8 * L; ++j) {                        // the bit's place in the group, 0 = first
                const int32_t lv = (int32_t)lvs[j];
                sc[j] += (pb >> (8 * L - 1 - j)) & 1u ? lv : -lv;
                ws[j] += lv;
                wsq += (uint32_t)(lv * lv);
            }
        }
    }
    if (tid < Q) {
#pragma unroll
        for (int i = 0; i < L; ++i) s_own[i][(tid * L + i) % P] = (uint16_t)tid;
    }
    for (int s = 32; s > 0; s >>= 1) { flags |= __shfl_xor(flags, s, 64); wsq += __shfl_xor(wsq, s, 64); }
    if (lane == 0) { s_flags[tid >> 6] = flags; s_wsq[tid >> 6] = wsq; }

    int32_t as[SOFT_L_TRIPS], aw[SOFT_L_TRIPS];                      // message bit tid + 256 j
#pragma unroll
    for (int j = 0; j < SOFT_L_TRIPS; ++j) { as[j] = 0; aw[j] = 0; }
#pragma unroll
    for (int i = 0; i < L; ++i) {
        if (i) __syncthreads();                                      // the readers of the round before are done
#pragma unroll
        for (int k = 0; k < 8; ++k) { s_part[k][tid] = sc[8 * i + k]; s_part[8 + k][tid] = ws[8 * i + k]; }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < SOFT_L_TRIPS; ++j) {
            const uint32_t t = (uint32_t)j * GSW_WG + tid;
            if (t < M) {
                const uint32_t own = s_own[i][t >> 3];
                if (own != NO_OWNER)
                    for (uint32_t r = 0, th = own; r < p.reps; ++r, th += Q) { as[j] += s_part[t & 7u][th]; aw[j] += s_part[8u + (t & 7u)][th]; }
            }
        }
    }

#pragma unroll
    for (int j = 0; j < SOFT_L_TRIPS; ++j) {
        if ((uint32_t)j * GSW_WG < M) {                              // the same for every lane: the ballot runs with all lanes on
            const uint32_t t = (uint32_t)j * GSW_WG + tid;
            if (t < M) {
                if (p.score) p.score[(size_t)b * M + t] = as[j];
                if (p.wsum) p.wsum[(size_t)b * M + t] = aw[j];
            }
            const uint64_t ball = __ballot(t < M && as[j] > 0);      // ties and no weight -> 0
            if (t < M && (t & 7u) == 0) {
                const uint32_t v = ballot_byte(ball, lane, 0u);
                p.bits[(size_t)b * P + (t >> 3)] = (uint8_t)v;
                s_match[t >> 3] = 8u - __popc(v ^ (uint32_t)rec[GSW_REC_HEAD + (t >> 3)]);
            }
        }
    }
    __syncthreads();
    store_matches_flags<GSW_WG / 64>(s_match, s_flags, P, p.matches, p.flags, b);
    if (tid == 0 && p.wsq) p.wsq[b] = (int32_t)(s_wsq[0] + s_wsq[1] + s_wsq[2] + s_wsq[3]);
}

// the 8 L bits of group g (first bit on top) as L bytes at row[g L ..], first byte at the lower address; one store where the row allows it
template <int L>
__device__ __forceinline__ void store_group(uint8_t* row, uint32_t g, uint32_t bits, bool aligned) {
    if (aligned) {
        if constexpr (L == 2) reinterpret_cast<uint16_t*>(row)[g] = (uint16_t)(((bits >> 8) & 0xFFu) | ((bits & 0xFFu) << 8));
        else reinterpret_cast<uint32_t*>(row)[g] = __builtin_bswap32(bits);
    } else {
#pragma unroll
        for (int i = 0; i < L; ++i) row[g * L + i] = (uint8_t)(bits >> (8 * (L - 1 - i)));
    }
}

template <typename T, int L, int STEPS>
__global__ __launch_bounds__(GSW_WG) void gsw_level_pack_l_kernel(LevelPackArgs p) {
    typedef typename codec_l::QLoad<T>::F F;
    __shared__ float s_thr[L][SOFT_MAX_LEVELS + 1];
    __shared__ typename EdgePair<F>::V s_edge[SOFT_MAX_LEVELS + 1][Geo<L>::ROWS];
    __shared__ uint32_t s_flags[GSW_WG / 64], s_wsum[GSW_WG / 64], s_wsq[GSW_WG / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t b = blockIdx.x;
    const uint32_t N = p.n_elems, ngroups = N >> 3, rowbytes = ngroups * L;
    edges_to_lds<L, F>(p.thr + (int64_t)b * p.thr_stride, p.levels, s_thr, s_edge, tid);

    const T* z = reinterpret_cast<const T*>(p.z) + (size_t)b * N;
    uint8_t* signs = p.signs + (size_t)b * rowbytes;
    uint8_t* planes = p.planes + (size_t)b * STEPS * rowbytes;
    // rowbytes is a multiple of L: every row of an aligned operand starts on an L-byte boundary
    const bool sa = (reinterpret_cast<uintptr_t>(p.signs) & (uintptr_t)(L - 1)) == 0, pa = (reinterpret_cast<uintptr_t>(p.planes) & (uintptr_t)(L - 1)) == 0;
    uint32_t flags = 0, wsum = 0, wsq = 0;
    for (uint32_t g = tid; g < ngroups; g += GSW_WG) {               // N % 8 == 0: whole, 16-byte aligned groups
        F v[8];
        codec_l::QLoad<T>::ld8(z + ((size_t)g << 3), v);
        uint32_t yb = 0, pl[STEPS], y[8], lvs[8 * L];
#pragma unroll
        for (int s = 0; s < STEPS; ++s) pl[s] = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) { y[e] = codec_l::quant1<L, F>(v[e], flags); yb |= y[e] << (L * (7 - e)); }
        levels_group<L, STEPS, F>(v, y, s_edge, lvs);
#pragma unroll
        for (int j = 0; j < 8 * L; ++j) {
#pragma unroll
            for (int s = 0; s < STEPS; ++s) pl[s] |= ((lvs[j] >> s) & 1u) << (8 * L - 1 - j);
            wsum += lvs[j];
            wsq += lvs[j] * lvs[j];
        }
        store_group<L>(signs, g, yb, sa);
#pragma unroll
        for (int s = 0; s < STEPS; ++s) store_group<L>(planes + (size_t)s * rowbytes, g, pl[s], pa);
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

// f(std::integral_constant<int, L>{}); l is 2 or 4
template <typename F> static int with_window(int l, F&& f) {
    return l == 2 ? f(std::integral_constant<int, 2>{}) : f(std::integral_constant<int, 4>{});
}

}  // namespace codec_soft_l

// The host side is gswm_codec_soft.inc's with l = 2 or 4: level_check / vote_check, pack_args / vote_args, launch_pack / launch_vote.
int gsw_level_pack_l(const void* z_dev, int z_dtype, const float* thr_dev, int64_t thr_stride, int levels, int l, uint8_t* signs_dev,
                     uint8_t* planes_dev, int32_t* wsum_dev, int32_t* wsq_dev, uint32_t* flags_dev, int B, int64_t n_elems, void* stream) {
    using namespace codec_soft;
    if (!signs_dev || !planes_dev || !wsum_dev || !wsq_dev || !flags_dev || B < 1 || l == 1) return GSW_ERR_BAD_ARG;
    const int rc = level_check(z_dev, z_dtype, thr_dev, thr_stride, levels, l, n_elems);
    if (rc != GSW_OK) return rc;
    const LevelPackArgs a = pack_args(z_dev, z_dtype, thr_dev, thr_stride, levels, signs_dev, planes_dev, wsum_dev, wsq_dev, flags_dev, n_elems);
    return with_dtype(z_dtype, [&](auto t) {
        return codec_soft_l::with_window(l, [&](auto w) {
            return with_steps(a.levels, [&](auto steps) {
                return launch_pack(codec_soft_l::gsw_level_pack_l_kernel<typename decltype(t)::type, decltype(w)::value, decltype(steps)::value>, a, B,
                                   (hipStream_t)stream);
            });
        });
    });
}

int gsw_extract_soft_l(const void* z_dev, int z_dtype, const uint8_t* records_dev, int64_t record_stride, int msg_bytes, const float* thr_dev,
                       int64_t thr_stride, int levels, int l, uint8_t* bits_dev, int32_t* score_dev, int32_t* wsum_dev, int32_t* wsq_dev,
                       uint32_t* flags_dev, uint32_t* matches_dev, int B, int64_t n_elems, void* stream) {
    using namespace codec_soft;
    if (l == 1) return GSW_ERR_BAD_ARG;                              // that is gsw_extract_soft; every refusal before GSW_ERR_UNSUPPORTED is GSW_ERR_BAD_ARG
    const int rc = vote_check(z_dev, z_dtype, records_dev, record_stride, msg_bytes, thr_dev, thr_stride, levels, l, bits_dev, flags_dev, B, n_elems);
    if (rc != GSW_OK) return rc;
    const ExtractSoftArgs a = vote_args(z_dev, z_dtype, records_dev, record_stride, msg_bytes, thr_dev, thr_stride, levels, l, bits_dev, score_dev, wsum_dev, wsq_dev,
                                        flags_dev, matches_dev, n_elems);
    return with_dtype(z_dtype, [&](auto t) {
        return codec_soft_l::with_window(l, [&](auto w) {
            return with_steps(a.levels, [&](auto steps) {              // 16 KiB: next to up to 26.8 KiB of static LDS
                return launch_vote(codec_soft_l::gsw_extract_soft_l_kernel<typename decltype(t)::type, decltype(w)::value, decltype(steps)::value>, 16u * 1024u, a,
                                   B, (hipStream_t)stream);
            });
        });
    });
}
