// gswm_keysearch_soft.inc -- the blind key search ranked by reliability levels: score a batch of packed sign rows WITH their level planes under every key
// of a keyring, without a message (gfx950).  Included at the end of gswm_keyed.hip after gswm_keysearch.inc: KeyedArgs, launch_search, the finish kernel,
// gswm_chacha.h's block function and gswm_topk.h are that file's.
//
//   d       = h[b] ^ keystream(key_u, nonce_u)                  h: the sign row of gsw_level_pack, n_bits of them (l = 1)
//   w_j     = sum_k 2^k plane_k[j]                              the element's level, 0 .. 2^P - 1, from the P plane rows of gsw_level_pack
//   X_t     = sum_{j mod M == t} w_j (2 d_j - 1) = 2 A_t - W_t  A_t = sum_k 2^k #{ j mod M == t : plane_k[j] & d_j },  W_t = sum_{j mod M == t} w_j
//   S[b, u] = sum_t |X_t|                                       sum_t |score[t]| of gsw_extract_soft under that key; with one plane of all ones gsw_key_search_topk's S
//   out     = the k best keys per image by (S descending, index ascending)
//
// The shape is gsw_key_search_scan_kernel's: a workgroup stages the 1 + P rows of each of its T images in LDS once and walks its range of keys, kpi keys per step;
// every quad computes ChaCha20 blocks of the step's keys into LDS, every (key, image) pair of the step is counted by G adjacent lanes whose partial sums meet in a
// shuffle butterfly, lane 0 of the group keeps the running top-8 list of its image.
//
// Counting, msg_bytes % 4 == 0 (CP > 0).  A lane takes message word m and adds the V words of the row that vote on its 32 positions into CP bit-sliced vertical
// counters.  The P one-bit values plane_k & d of a word are the bits of a P-bit number per position: they enter the counters through P full adders (plane k into
// counter plane k) and the carry ripples through the other CP - P planes, 5 P + 2 (CP - P) operations per word where the sign search spends 2 PL.  The counters then
// hold A_t.  W_t does not depend on the key: it is counted the same way once in front of the key loop (d = all ones) and kept bit-sliced in LDS, nb = bit length of
// (2^P - 1) V planes per message word.  With the mask ge = (2 A >= W), found by a bit-sliced compare of the shifted counters with those planes,
//   sum over the word's 32 positions of |2 A - W| = 2 sum_p 2^p (2 popcount(A_p & ge) - popcount(A_p)) - sum_p 2^p (2 popcount(W_p & ge) - popcount(W_p)).
// CP is a class -- 4, 8, 12, 16, 18, the smallest with (2^P - 1) V < 2^CP -- not the count.
// Counting, any other msg_bytes (CP == 0).  A lane takes position t and adds +- w_j over its V copies bit by bit; P is a run-time value there.
//
// Rows that do not fit the LDS with one keystream and W_t (SG) are read from global memory; the tile is then one image.
//
// key_soft_decide (gswm_keysearch_soft_plan.h, host only) is the whole launch policy and every refusal; the entry point fills the arguments from its plan.
// All arithmetic is integer; the result depends on neither geometry nor arrival order.
//
// Kernel
//   gsw_key_search_soft_scan_kernel<CP, P, SG> : CP counter planes and P level planes (0, 0: the bit-by-bit path), SG: rows read from global memory
//   (gsw_trace_keyed_finish_kernel of gswm_keyed.hip finishes)

namespace {

struct KeySearchSoftArgs {
    KeyedArgs base;           // signs, records (= the key rows), partial, idx, score, stride, U, B, k, n_bits, rowbytes, nblk, msg_bytes, grid_x, signs_aligned (the planes too)
    const uint8_t* planes;    // [B, P, rowbytes]
    int P;                    // level planes
    int T, G, kpi;            // images per workgroup, lanes per (key, image) pair, keys per step
    int istride;              // words between the rows of two images in LDS (>= (1 + P) nblk 16, offset against bank conflicts)
    int copies;               // V
    int nb;                   // planes of W_t in LDS
    uint32_t ks_off, w_off;   // byte offsets of the keystreams and of W_t in LDS
};

// adds the 32 P-bit values x (bit k of a value in x[k]) to the 32 vertical counters
template <int CP, int P>
__device__ __forceinline__ void level_planes_add(uint32_t (&pl)[CP], const uint32_t (&x)[P]) {
    uint32_t carry = 0u;
#pragma unroll
    for (int k = 0; k < P; ++k) {
        const uint32_t t = pl[k] ^ x[k];
        const uint32_t c = (pl[k] & x[k]) | (carry & t);
        pl[k] = t ^ carry;
        carry = c;
    }
#pragma unroll
    for (int p = P; p < CP; ++p) {
        const uint32_t t = pl[p] & carry;
        pl[p] ^= carry;
        carry = t;
    }
}

// sum over the 32 counters A of |2 A - W|; W bit-sliced at wp[q * wstride], q < nb (the planes above are zero: W < 2^CP)
template <int CP>
__device__ __forceinline__ int level_abs_margin(const uint32_t (&a)[CP], const uint32_t* wp, int wstride, int nb) {
    uint32_t w[CP];
#pragma unroll
    for (int q = 0; q < CP; ++q) w[q] = q < nb ? wp[q * wstride] : 0u;
    uint32_t gt = a[CP - 1], eq = ~a[CP - 1];                       // plane CP of 2 A against a zero plane of W
#pragma unroll
    for (int q = CP - 1; q >= 1; --q) {                             // plane q of 2 A is plane q - 1 of A
        gt |= eq & a[q - 1] & ~w[q];
        eq &= ~(a[q - 1] ^ w[q]);
    }
    eq &= ~w[0];                                                    // plane 0 of 2 A is zero
    const uint32_t ge = gt | eq;
    int sa = 0, sw = 0;
#pragma unroll
    for (int p = 0; p < CP; ++p) {
        sa += (2 * __popc(a[p] & ge) - __popc(a[p])) * (1 << p);
        sw += (2 * __popc(w[p] & ge) - __popc(w[p])) * (1 << p);
    }
    return 2 * sa - sw;
}

template <int CP, int P, bool SG>
__global__ __launch_bounds__(KS_WG) void gsw_key_search_soft_scan_kernel(KeySearchSoftArgs s) {
    const KeyedArgs& a = s.base;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const int tid = threadIdx.x;
    const int rowwords = a.nblk * 16;
    const int T = s.T, G = s.G, NP = CP > 0 ? P : s.P;
    const int img0 = blockIdx.y * T;
    uint32_t* sw = (uint32_t*)lds_raw;                              // [T][istride]: per image the sign row and the plane rows, [1 + P][rowwords] (not with SG)
    uint32_t* kw = (uint32_t*)(lds_raw + s.ks_off);                 // [kpi][rowwords] keystream words of the step
    uint32_t* wpl = (uint32_t*)(lds_raw + s.w_off);                 // [T][nb][W] the planes of W_t (word path)

    // ---- stage the rows of this image tile (zero-padded to whole blocks)
    if constexpr (!SG) {
        for (int tr = 0; tr < T * (1 + NP); ++tr) {
            const int t = tr / (1 + NP), r = tr - t * (1 + NP);
            const int b = img0 + t;
            const uint8_t* row = r == 0 ? a.signs + (int64_t)b * a.rowbytes : s.planes + ((int64_t)b * NP + (r - 1)) * a.rowbytes;
            for (int w = tid; w < rowwords; w += KS_WG) {
                const int byte0 = 4 * w;
                uint32_t x = 0u;
                if (b < a.B) {
                    if (a.signs_aligned) {
                        if (byte0 < a.rowbytes) x = *(const uint32_t*)(row + byte0);
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (byte0 + i < a.rowbytes) x |= (uint32_t)row[byte0 + i] << (8 * i);
                    }
                }
                sw[t * s.istride + r * rowwords + w] = x;
            }
        }
        __syncthreads();
    }

    int64_t L[TR_LIST];
#pragma unroll
    for (int j = 0; j < TR_LIST; ++j) L[j] = TR_EMPTY;
    const int group = tid / G, g = tid % G;
    const int t = group % T, kk = group / T;                        // this group's image of the tile and key of the step
    const bool image_ok = kk < s.kpi && img0 + t < a.B;
    const int M = 8 * a.msg_bytes, V = s.copies;
    const int W = a.msg_bytes >> 2;
    const uint32_t col = (uint32_t)tid & 3u;

    // the group's image: its sign row, its plane rows (plane k at pp + k * prow)
    const uint32_t* sp;
    const uint32_t* pp;
    int prow;
    if constexpr (SG) {
        sp = (const uint32_t*)(a.signs + (int64_t)(img0 + t) * a.rowbytes);
        pp = (const uint32_t*)(s.planes + (int64_t)(img0 + t) * NP * a.rowbytes);
        prow = a.rowbytes >> 2;                                     // (the bit-by-bit path uses bytes: 4 * prow is not used there)
    } else {
        sp = sw + t * s.istride;
        pp = sp + rowwords;
        prow = rowwords;
    }

    // ---- W_t of the tile's images, once: the levels of every message word's 32 positions, counted like A_t with d = all ones
    if constexpr (CP > 0) {
        if (image_ok && kk == 0) {
            for (int m = g; m < W; m += G) {
                uint32_t pl[CP];
#pragma unroll
                for (int p = 0; p < CP; ++p) pl[p] = 0u;
                for (int w = m; w < V * W; w += W) {
                    uint32_t x[P];
#pragma unroll
                    for (int k = 0; k < P; ++k) x[k] = pp[k * prow + w];
                    level_planes_add<CP, P>(pl, x);
                }
#pragma unroll
                for (int q = 0; q < CP; ++q)
                    if (q < s.nb) wpl[(t * s.nb + q) * W + m] = pl[q];
            }
        }
    }

    const int64_t u0 = a.U * blockIdx.x / a.grid_x, u1 = a.U * (blockIdx.x + 1) / a.grid_x;
    for (int64_t ub = u0; ub < u1; ub += s.kpi) {
        __syncthreads();                                            // the previous step's keystreams have been read (first step: W_t is in place)
        for (int bi = tid >> 2; bi < s.kpi * a.nblk; bi += KS_WG >> 2) {
            const int key = bi / a.nblk, blk = bi - key * a.nblk;
            if (ub + key < u1) {                                    // (the same for the four lanes of a quad)
                const CipherLane ck = cipher_lane_of_record((const uint32_t*)(a.records + (ub + key) * a.stride), col);
                uint32_t ks[4];
                chacha20_block(ck, (uint64_t)blk, col, ks);
#pragma unroll
                for (int r = 0; r < 4; ++r) kw[key * rowwords + 16 * blk + 4 * r + (int)col] = ks[r];
            }
        }
        __syncthreads();

        const int64_t u = ub + kk;
        const bool active = image_ok && u < u1;
        int sum = 0;
        if (active) {
            const uint32_t* kp = kw + kk * rowwords;
            if constexpr (CP > 0) {
                for (int m = g; m < W; m += G) {
                    uint32_t pl[CP];
#pragma unroll
                    for (int p = 0; p < CP; ++p) pl[p] = 0u;
                    for (int w = m; w < V * W; w += W) {
                        const uint32_t d = sp[w] ^ kp[w];
                        uint32_t x[P];
#pragma unroll
                        for (int k = 0; k < P; ++k) x[k] = pp[k * prow + w] & d;
                        level_planes_add<CP, P>(pl, x);
                    }
                    sum += level_abs_margin<CP>(pl, wpl + t * s.nb * W + m, W, s.nb);
                }
            } else {
                const uint8_t* kb = (const uint8_t*)kp;
                const uint8_t* sb = (const uint8_t*)sp;
                const uint8_t* pb = (const uint8_t*)pp;
                const int prowbytes = SG ? a.rowbytes : 4 * rowwords;
                for (int pos = g; pos < M; pos += G) {
                    int x = 0;
                    for (int j = pos; j < a.n_bits; j += M) {
                        const int byte = j >> 3, sh = 7 - (j & 7);
                        int lv = 0;
                        for (int k = 0; k < NP; ++k) lv |= ((pb[k * prowbytes + byte] >> sh) & 1) << k;
                        x += ((sb[byte] ^ kb[byte]) >> sh) & 1 ? lv : -lv;
                    }
                    sum += x < 0 ? -x : x;
                }
            }
        }
        for (int step = G >> 1; step >= 1; step >>= 1) sum += __shfl_xor(sum, step);   // G <= 64 divides 64: a group lies in one wave
        if (active && g == 0) list_insert(L, make_key(sum, u));
    }

    // ---- one list per group -> LDS -> one per (workgroup, image)
    __syncthreads();                                                // every wave is done with the rows, the keystreams and W_t: reuse the LDS
    int64_t* wlist = (int64_t*)lds_raw;                             // [KS_WG / G][TR_LIST]
    if (g == 0) put_list(wlist, group, L);
    __syncthreads();
    if (tid < T) {
        int64_t F[TR_LIST];
#pragma unroll
        for (int j = 0; j < TR_LIST; ++j) F[j] = wlist[tid * TR_LIST + j];
        for (int q = 1; q < KS_WG / G / T; ++q)
#pragma unroll
            for (int j = 0; j < TR_LIST; ++j) list_insert(F, wlist[(q * T + tid) * TR_LIST + j]);
        const int b = img0 + tid;
        if (b < a.B) {
            int64_t* dst = a.partial + ((int64_t)b * a.grid_x + blockIdx.x) * a.k;
#pragma unroll
            for (int j = 0; j < TR_LIST; ++j)
                if (j < a.k) dst[j] = F[j];
        }
    }
}

// the word path: the plan's class of counter planes.  Never planned, so not instantiated: 4 planes for rows in global memory (those have V > 15), 18 planes below
// P = 4 (7 V < 65536 in the domain)
template <int P, bool SG>
int launch_key_search_soft_counters(const KeySearchSoftArgs& s, const SearchPlan& g, int cp, hipStream_t st) {
    if constexpr (!SG) {
        if (cp == 4) return launch_search(gsw_key_search_soft_scan_kernel<4, P, SG>, s, s.base, g, st);
    }
    if constexpr (P == 4) {
        if (cp == 18) return launch_search(gsw_key_search_soft_scan_kernel<18, P, SG>, s, s.base, g, st);
    }
    switch (cp) {
        case 8: return launch_search(gsw_key_search_soft_scan_kernel<8, P, SG>, s, s.base, g, st);
        case 12: return launch_search(gsw_key_search_soft_scan_kernel<12, P, SG>, s, s.base, g, st);
        case 16: return launch_search(gsw_key_search_soft_scan_kernel<16, P, SG>, s, s.base, g, st);
        default: return GSW_ERR_UNSUPPORTED;
    }
}

template <bool SG>
int launch_key_search_soft(const KeySearchSoftArgs& s, const SearchPlan& g, int cp, hipStream_t st) {
    if (cp == 0) return launch_search(gsw_key_search_soft_scan_kernel<0, 0, SG>, s, s.base, g, st);
    switch (s.P) {
        case 1: return launch_key_search_soft_counters<1, SG>(s, g, cp, st);
        case 2: return launch_key_search_soft_counters<2, SG>(s, g, cp, st);
        case 3: return launch_key_search_soft_counters<3, SG>(s, g, cp, st);
        default: return launch_key_search_soft_counters<4, SG>(s, g, cp, st);
    }
}

}  // namespace

extern "C" {

size_t gsw_key_search_soft_workspace_bytes(int B, int64_t n_keys, int k) {
    return search_workspace_bytes(SEARCH_KEY, B, n_keys, k);
}

int gsw_key_search_soft_topk(const uint8_t* signs_dev, const uint8_t* planes_dev, int P, int B, int64_t n_bits, const uint8_t* keys_dev, int64_t key_stride,
                             int msg_bytes, int64_t n_keys, int k, int32_t* idx_dev, int32_t* stat_dev, void* workspace_dev, void* stream) {
    auto aligned = [](const void* p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) == 0; };
    const KeySoftQuery q{B, P, n_bits, key_stride, n_keys, msg_bytes, k, aligned(signs_dev, 4), aligned(planes_dev, 4), aligned(keys_dev, 16),
                         !signs_dev, !planes_dev, !keys_dev, !(idx_dev && stat_dev && workspace_dev)};
    const KeySoftPlan p = key_soft_decide(q);
    if (p.status != GSW_OK) return p.status;
    const KeySearchSoftArgs s{KeyedArgs{signs_dev, keys_dev, (int64_t*)workspace_dev, idx_dev, stat_dev, key_stride, n_keys, B, k, (int)n_bits, p.rowbytes, p.nblk,
                                        msg_bytes, p.grid_x, p.rows_aligned},
                              planes_dev, P, p.T, p.G, p.kpi, p.istride, p.copies, p.nb, p.ks_off, p.w_off};
    SearchPlan g{};                                                 // what launch_search reads: the grid and the LDS
    g.grid_x = p.grid_x, g.grid_y = p.grid_y, g.wg = p.wg, g.lds = p.lds;
    return p.sg ? launch_key_search_soft<true>(s, g, p.cp, (hipStream_t)stream) : launch_key_search_soft<false>(s, g, p.cp, (hipStream_t)stream);
}

}  // extern "C"
