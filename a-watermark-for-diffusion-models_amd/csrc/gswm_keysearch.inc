// gswm_keysearch.inc -- blind key search: score a batch of packed sign rows under every key of a keyring WITHOUT a message (gfx950).
// Included at the end of gswm_keyed.hip: KeyedArgs, the finish kernel, gswm_chacha.h's block function and gswm_topk.h are that file's.
//
//   d       = h[b] ^ keystream(key_u, nonce_u)                  h: the image's quantised bits (gsw_sign_pack / gsw_quant_pack), n_bits of them
//   c_t     = #{ j < n_bits : j mod M == t, d_j = 1 }           M = 8 msg_bytes message positions, V = n_bits / M copies of each
//   S[b, u] = sum_t |2 c_t - V|                                 the score gsw_trace_keyed_topk gives the image's own majority-voted message
//   out     = the k best keys per image by (S descending, index ascending)
//
// Work split.  A workgroup stages the sign rows of its tile of T images in LDS once and walks its range of keys, KPI keys per step: every
// quad of the workgroup computes ChaCha20 blocks of the step's keys into LDS (gswm_chacha.h, four lanes per block), then every (key, image)
// pair of the step is counted by a group of G adjacent lanes (G a power of two, G T KPI <= the workgroup), whose partial sums meet in a
// shuffle butterfly; lane 0 of the group keeps the running top-8 list of ITS image (the group -> image assignment never changes).
//
// Counting, msg_bytes % 4 == 0 (PL > 0).  Words of the row that are W = M / 32 apart vote on the same 32 positions.  A lane takes message
// word m and adds the V words d[m + j W] into PL bit-sliced vertical counters (plane p = bit p of the 32 counts; a ripple-carry add of
// one word is 2 PL ops and replaces 32 scalar counts).  The 32 counts are never un-sliced one by one: with the mask ge = (c >= ceil(V/2)),
// found by a bit-sliced compare,
//   sum over the word's 32 positions of |2 c - V| = 2 sum_p 2^p (2 popcount(plane_p & ge) - popcount(plane_p)) - V (2 popcount(ge) - 32)
// (a tie has 2 c = V and adds 0 on either side of the mask).  PL in {4, 8, 12, 16} is the smallest with V < 2^PL.
// Counting, any other msg_bytes (PL == 0).  A lane takes position t and counts its V copies bit by bit from the bytes in LDS.
//
// The lattice limit is gsw_trace_keyed_topk's (1 048 576 bits).  A row and one key's keystream of it fit the 128 KiB of LDS together up to
// 523 264 bits; beyond that (SG) the tile is one image whose row is read from global memory and LDS holds the keystream alone.
//
// T, G, KPI, the row offset, PL and SG are search_decide's (gswm_search_plan.h), with the refusals; the entry point here fills KeySearchArgs from its plan.
//
// Top-k.  gswm_topk.h: group lists -> LDS -> one list per (workgroup, image) in the caller's workspace -> gsw_trace_keyed_finish_kernel.
// All arithmetic is integer; the result depends on neither geometry nor arrival order.
//
// Kernel
//   gsw_key_search_scan_kernel<PL, SG> : PL counter planes (0: the bit-by-bit path), SG: sign rows read from global memory

namespace {

struct KeySearchArgs {
    KeyedArgs base;           // signs, records (= the key rows), partial, idx, score, stride, U, B, k, n_bits, rowbytes, nblk, msg_bytes, grid_x, signs_aligned
    int T;                    // images per workgroup
    int G;                    // lanes per (key, image) pair
    int kpi;                  // keys per step
    int srow;                 // words between the sign rows of two images in LDS (>= nblk * 16, offset against bank conflicts)
    int copies;               // V
};

// adds the 32 one-bit values of x to the 32 vertical counters
template <int PL>
__device__ __forceinline__ void planes_add(uint32_t (&pl)[PL], uint32_t x) {
    uint32_t carry = x;
#pragma unroll
    for (int p = 0; p < PL; ++p) {
        const uint32_t t = pl[p] & carry;
        pl[p] ^= carry;
        carry = t;
    }
}

// sum over the 32 counters c of |2 c - V|; half = ceil(V / 2)
template <int PL>
__device__ __forceinline__ int planes_abs_margin(const uint32_t (&pl)[PL], int V, uint32_t half) {
    uint32_t gt = 0u, eq = 0xFFFFFFFFu;
#pragma unroll
    for (int p = PL - 1; p >= 0; --p) {
        const uint32_t kb = (half >> p) & 1u ? 0xFFFFFFFFu : 0u;
        gt |= eq & pl[p] & ~kb;
        eq &= ~(pl[p] ^ kb);
    }
    const uint32_t ge = gt | eq;
    int s = 0;
#pragma unroll
    for (int p = 0; p < PL; ++p) s += (2 * __popc(pl[p] & ge) - __popc(pl[p])) << p;
    return 2 * s - V * (2 * __popc(ge) - 32);
}

template <int PL, bool SG>
__global__ __launch_bounds__(KS_WG) void gsw_key_search_scan_kernel(KeySearchArgs s) {
    const KeyedArgs& a = s.base;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    const int tid = threadIdx.x;
    const int rowwords = a.nblk * 16;
    const int T = s.T, G = s.G;
    const int img0 = blockIdx.y * T;
    uint32_t* sw = (uint32_t*)lds_raw;                              // [T][srow] sign words (not with SG)
    uint32_t* kw = sw + (SG ? 0 : T * s.srow);                      // [kpi][rowwords] keystream words of the step

    // ---- stage the sign rows of this image tile (zero-padded to whole blocks)
    if constexpr (!SG) {
        for (int t = 0; t < T; ++t) {
            const int b = img0 + t;
            const uint8_t* row = a.signs + (int64_t)b * a.rowbytes;
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
                sw[t * s.srow + w] = x;
            }
        }
    }

    int64_t L[TR_LIST];
#pragma unroll
    for (int j = 0; j < TR_LIST; ++j) L[j] = TR_EMPTY;
    const int group = tid / G, g = tid % G;
    const int t = group % T, kk = group / T;                        // this group's image of the tile and key of the step
    const bool image_ok = kk < s.kpi && img0 + t < a.B;
    const int M = 8 * a.msg_bytes, V = s.copies;
    const uint32_t half = (uint32_t)(V + 1) >> 1;
    const uint32_t col = (uint32_t)tid & 3u;

    const int64_t u0 = a.U * blockIdx.x / a.grid_x, u1 = a.U * (blockIdx.x + 1) / a.grid_x;
    for (int64_t ub = u0; ub < u1; ub += s.kpi) {
        __syncthreads();                                            // the previous step's keystreams have been read (first step: the sign rows are staged)
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
            if constexpr (PL > 0) {
                const int W = a.msg_bytes >> 2;
                const uint32_t* sp;
                if constexpr (SG) sp = (const uint32_t*)(a.signs + (int64_t)(img0 + t) * a.rowbytes);
                else sp = sw + t * s.srow;
                for (int m = g; m < W; m += G) {
                    uint32_t pl[PL];
#pragma unroll
                    for (int p = 0; p < PL; ++p) pl[p] = 0u;
                    for (int w = m; w < V * W; w += W) planes_add<PL>(pl, sp[w] ^ kp[w]);
                    sum += planes_abs_margin<PL>(pl, V, half);
                }
            } else {
                const uint8_t* kb = (const uint8_t*)kp;
                const uint8_t* sb;
                if constexpr (SG) sb = a.signs + (int64_t)(img0 + t) * a.rowbytes;
                else sb = (const uint8_t*)(sw + t * s.srow);
                for (int pos = g; pos < M; pos += G) {
                    int c = 0;
                    for (int j = pos; j < a.n_bits; j += M) c += ((sb[j >> 3] ^ kb[j >> 3]) >> (7 - (j & 7))) & 1;
                    const int d = 2 * c - V;
                    sum += d < 0 ? -d : d;
                }
            }
        }
        for (int step = G >> 1; step >= 1; step >>= 1) sum += __shfl_xor(sum, step);   // G <= 64 divides 64: a group lies in one wave
        if (active && g == 0) list_insert(L, make_key(sum, u));
    }

    // ---- one list per group -> LDS -> one per (workgroup, image)
    __syncthreads();                                                // every wave is done with the rows and the keystreams: reuse the LDS
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

template <bool SG>
int launch_key_search_planes(const KeySearchArgs& s, const SearchPlan& p, hipStream_t st) {
    switch (p.planes) {
        case 0: return launch_search(gsw_key_search_scan_kernel<0, SG>, s, s.base, p, st);
        case 4: return launch_search(gsw_key_search_scan_kernel<4, SG>, s, s.base, p, st);
        case 8: return launch_search(gsw_key_search_scan_kernel<8, SG>, s, s.base, p, st);
        case 12: return launch_search(gsw_key_search_scan_kernel<12, SG>, s, s.base, p, st);
        default: return launch_search(gsw_key_search_scan_kernel<16, SG>, s, s.base, p, st);
    }
}

}  // namespace

extern "C" {

size_t gsw_key_search_workspace_bytes(int B, int64_t n_keys, int k) {
    return search_workspace_bytes(SEARCH_KEY, B, n_keys, k);
}

int gsw_key_search_topk(const uint8_t* signs_dev, int B, int64_t n_bits, const uint8_t* keys_dev, int64_t key_stride, int msg_bytes, int64_t n_keys,
                        int k, int32_t* idx_dev, int32_t* stat_dev, void* workspace_dev, void* stream) {
    const SearchQuery q = search_query(SEARCH_KEY, signs_dev, nullptr, nullptr, keys_dev, idx_dev && stat_dev && workspace_dev, B, n_bits, key_stride, msg_bytes,
                                       n_keys, k, 0);
    const SearchPlan p = search_decide(q);
    if (p.status != GSW_OK) return p.status;
    const KeySearchArgs s{keyed_args(q, p, signs_dev, keys_dev, workspace_dev, idx_dev, stat_dev), p.T, p.G, p.kpi, p.srow, p.copies};
    return p.sg ? launch_key_search_planes<true>(s, p, (hipStream_t)stream) : launch_key_search_planes<false>(s, p, (hipStream_t)stream);
}

}  // extern "C"
