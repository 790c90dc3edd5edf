// gswm_pool.inc -- pooled evidence across the images of a set (gfx950).  Included at the end of gswm_keyed.hip: the record walk's helpers (popcount_add,
// transpose_reduce, lane_image), KeyedArgs, the finish kernel, launch_search and gswm_topk.h are that file's, used as they are.
//
// Every score of the keyed searches is linear in the image: for record u with codeword e[u], image b scores sum_j lev_bj (1 - 2 h_bj)(1 - 2 e[u]_j).  The sum over
// the images of a set is therefore the score of ONE pooled row,
//   S_j      = sum_{b in set} lev_bj (1 - 2 h_bj)                h: the sign row, lev: the levels (1 without planes)
//   sign bit = S_j < 0, level = |S_j|                            S_j = 0: sign 0, level 0
//   score[g, u] = sum_j |S_j| (1 - 2 (sign_j ^ e[u]_j)) = wsum_g - 2 sum_{k < Q} 2^k popcount(plane_k[g] & (signs[g] ^ e[u]))
// so a set is pooled once and searched once, whatever its size.  All of it is integer arithmetic and exact.
//
// gsw_pool_rows_kernel<P>.  One workgroup per set, the plain form: a lane owns one 32-bit word of the row, keeps the 32 sums of its positions in registers
// (int32; |S_j| <= 1023) and walks the set's images in its inner loop, reading 1 + P words per image -- as whole dwords when the rows are 4-byte aligned,
// byte by byte otherwise (any base pointer, any row length).  Per position it forms level = sum_k 2^k bit_k and adds +-level.  At the end it writes the sign
// word and the Q plane words of its 32 positions and adds sum |S| and sum S^2 into the workgroup's totals through a wave reduction and LDS: one store of wsum and
// wsq per set, every output byte written, no atomics, nothing to zero first.  Rows longer than the workgroup are walked in steps of it.  Image indices taken
// from set_ptr are clipped to [0, B]: a wrong table reads no memory outside the batch.
//
// gsw_trace_keyed_pooled_scan_kernel<T, MSG4>.  gsw_trace_keyed_soft_scan_kernel's record walk with the planes as a RUN-TIME loop (Q in 1..10): 6 instantiations
// instead of the 60 that Q as a template parameter would take next to the soft search's 32.  The staging, the ChaCha20 block in registers, the message XOR, the
// mask of a ragged last block, the transposing reduction and the top-k tail are that kernel's, restated here because its loop body is not shared (gswm_keyed_soft.inc
// says what sharing cost).  Per codeword fragment a lane forms x = s ^ w once per set, then per plane four v_and + v_bcnt_u32_b32 into a temporary that is folded
// in by a shift; the sum is at most wsum_g < 2^31.  T in {1, 4, 16} sets per workgroup (pool_decide).
//
// Host side: pool_decide (gswm_pool_plan.h) refuses or plans; the entry points fill the arguments from the plan and launch.

namespace {

struct PoolRowsArgs {
    const uint8_t* signs;     // [B, rowbytes]
    const uint8_t* planes;    // [B, P, rowbytes], null with P = 0
    const int32_t* set_ptr;   // [G + 1]
    uint8_t* out_signs;       // [G, rowbytes]
    uint8_t* out_planes;      // [G, Q, rowbytes]
    int32_t* wsum;            // [G]
    int64_t* wsq;             // [G]
    int B, Q, rowbytes, rowwords, rows_aligned;
};

// the 32-bit word at byte0 of a row: bytes past the row's end read as zero
__device__ __forceinline__ uint32_t pool_load_word(const uint8_t* row, int byte0, int rowbytes, int aligned) {
    if (aligned) return *(const uint32_t*)(row + byte0);
    uint32_t x = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (byte0 + i < rowbytes) x |= (uint32_t)row[byte0 + i] << (8 * i);
    return x;
}

__device__ __forceinline__ void pool_store_word(uint8_t* row, int byte0, int rowbytes, int aligned, uint32_t x) {
    if (aligned) {
        *(uint32_t*)(row + byte0) = x;
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (byte0 + i < rowbytes) row[byte0 + i] = (uint8_t)(x >> (8 * i));
}

template <int P>
__global__ __launch_bounds__(POOL_ROWS_WG) void gsw_pool_rows_kernel(PoolRowsArgs a) {
    __shared__ int32_t red_sum[POOL_ROWS_WG / 64];
    __shared__ unsigned long long red_sq[POOL_ROWS_WG / 64];
    const int g = blockIdx.x, tid = threadIdx.x;
    int b0 = a.set_ptr[g], b1 = a.set_ptr[g + 1];
    b0 = b0 < 0 ? 0 : b0 > a.B ? a.B : b0;
    b1 = b1 < b0 ? b0 : b1 > a.B ? a.B : b1;
    int32_t tsum = 0;
    unsigned long long tsq = 0ull;

    for (int w = tid; w < a.rowwords; w += blockDim.x) {
        const int byte0 = 4 * w;
        int S[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) S[i] = 0;
#pragma unroll 4                                        // (four images' loads in flight: the loop is bound by their latency, not by the adds)
        for (int b = b0; b < b1; ++b) {
            const uint32_t s = pool_load_word(a.signs + (int64_t)b * a.rowbytes, byte0, a.rowbytes, a.rows_aligned);
            if constexpr (P == 0) {
#pragma unroll
                for (int i = 0; i < 32; ++i) S[i] += 1 - 2 * (int)((s >> i) & 1u);
            } else {
                uint32_t pl[P];
#pragma unroll
                for (int k = 0; k < P; ++k) pl[k] = pool_load_word(a.planes + ((int64_t)b * P + k) * a.rowbytes, byte0, a.rowbytes, a.rows_aligned);
#pragma unroll
                for (int i = 0; i < 32; ++i) {
                    int lev = 0;
#pragma unroll
                    for (int k = 0; k < P; ++k) lev += (int)((pl[k] >> i) & 1u) << k;
                    S[i] += ((s >> i) & 1u) ? -lev : lev;
                }
            }
        }
        // (bit positions past the row's end in a partial last word saw zero signs: at unit levels they hold the set's size, so they are masked out here)
        const int valid = a.rowbytes - byte0;
        const uint32_t live = valid >= 4 ? 0xFFFFFFFFu : (1u << (8 * valid)) - 1u;
        uint32_t sg = 0u;
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const int m = ((live >> i) & 1u) ? (S[i] < 0 ? -S[i] : S[i]) : 0;
            sg |= (uint32_t)(S[i] < 0) << i;
            S[i] = m;
            tsum += m;
            tsq += (unsigned long long)((uint32_t)m * (uint32_t)m);
        }
        pool_store_word(a.out_signs + (int64_t)g * a.rowbytes, byte0, a.rowbytes, a.rows_aligned, sg & live);
        for (int k = 0; k < a.Q; ++k) {
            uint32_t x = 0u;
#pragma unroll
            for (int i = 0; i < 32; ++i) x |= (((uint32_t)S[i] >> k) & 1u) << i;
            pool_store_word(a.out_planes + ((int64_t)g * a.Q + k) * a.rowbytes, byte0, a.rowbytes, a.rows_aligned, x);
        }
    }

    // ---- the set's totals: wave reduction, then one lane over the waves
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) {
        tsum += __shfl_xor(tsum, step);
        tsq += __shfl_xor(tsq, step);
    }
    if ((tid & 63) == 0) {
        red_sum[tid >> 6] = tsum;
        red_sq[tid >> 6] = tsq;
    }
    __syncthreads();
    if (tid == 0) {
        int32_t ws = 0;
        unsigned long long wq = 0ull;
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) {
            ws += red_sum[i];
            wq += red_sq[i];
        }
        a.wsum[g] = ws;
        a.wsq[g] = (int64_t)wq;
    }
}

int launch_pool_rows(const PoolRowsArgs& a, int P, const PoolPlan& p, hipStream_t st) {
    void (*kernel)(PoolRowsArgs) = P == 0 ? gsw_pool_rows_kernel<0> : P == 1 ? gsw_pool_rows_kernel<1> : P == 2 ? gsw_pool_rows_kernel<2>
                                   : P == 3 ? gsw_pool_rows_kernel<3> : gsw_pool_rows_kernel<4>;
    hipLaunchKernelGGL(kernel, dim3(p.grid_x, p.grid_y), dim3(p.wg), 0, st, a);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

struct KeyedPooledArgs {
    KeyedArgs base;           // the sign search's arguments with B = the sets (the finish kernel takes them as they are); signs_aligned covers the planes too
    const uint8_t* planes;    // [G, Q, rowbytes]
    const int32_t* wsum;      // [G]
    int Q;
};

template <int T, bool MSG4>
__global__ __launch_bounds__(KY_WG) void gsw_trace_keyed_pooled_scan_kernel(KeyedPooledArgs s) {
    const KeyedArgs& a = s.base;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    uint32_t* sw = (uint32_t*)lds_raw;                 // [T][1 + Q][nblk][4 cols][4 rows]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int quad = lane >> 2, col = lane & 3;
    const int rowwords = a.nblk * 16;
    const int img0 = blockIdx.y * T;
    const int Q = s.Q, R = 1 + Q;

    // ---- stage the sign row and the plane rows of this set tile, in operand order
    for (int tr = 0; tr < T * R; ++tr) {
        const int t = tr / R, r = tr % R;
        const int b = img0 + t;
        const uint8_t* row = r == 0 ? a.signs + (int64_t)b * a.rowbytes : s.planes + ((int64_t)b * Q + (r - 1)) * a.rowbytes;
        for (int w = tid; w < rowwords; w += KY_WG) {
            const int byte0 = 64 * (w >> 4) + 16 * (w & 3) + 4 * ((w >> 2) & 3);
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
            sw[tr * rowwords + w] = x;
        }
    }
    __syncthreads();

    int64_t L[TR_LIST];
#pragma unroll
    for (int j = 0; j < TR_LIST; ++j) L[j] = TR_EMPTY;
    const int img = lane_image<T>(lane);
    const bool owner = lane < T && img0 + img < a.B;
    const int wtotal = owner ? s.wsum[img0 + img] : 0;

    // message byte offsets of this lane's four words in its first block; every step of 16 blocks moves them by 1024 mod msg_bytes
    const int mb = a.msg_bytes;
    int off0[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) off0[r] = (64 * quad + 16 * r + 4 * col) % mb;
    const int off_step = 1024 % mb;
    const bool ragged = (a.rowbytes & 63) != 0;

    const uint32_t a0 = col == 0 ? 0x61707865u : col == 1 ? 0x3320646eu : col == 2 ? 0x79622d32u : 0x6b206574u;
    const int rowfrags = rowwords / 4;
    const uint4* sfrag = (const uint4*)lds_raw + col;  // + 4 blk + (t (1 + Q) + row) rowfrags

    const int64_t u0 = a.U * blockIdx.x / a.grid_x, u1 = a.U * (blockIdx.x + 1) / a.grid_x;
    auto fetch = [&](int64_t u, uint32_t& kb, uint32_t& kc, uint4& nn) {
        const uint32_t* rec = (const uint32_t*)(a.records + u * a.stride);
        kb = rec[col];
        kc = rec[4 + col];
        nn = *(const uint4*)(rec + 8);
    };
    uint32_t b0 = 0u, c0 = 0u, nb0, nc0;
    uint4 nonce = make_uint4(0u, 0u, 0u, 0u), nnonce;
    if (u0 + wave < u1) fetch(u0 + wave, b0, c0, nonce);

    for (int64_t u = u0 + wave; u < u1; u += KY_WAVES) {
        nb0 = b0; nc0 = c0; nnonce = nonce;
        if (u + KY_WAVES < u1) fetch(u + KY_WAVES, nb0, nc0, nnonce);     // the next record's cipher words, under this one's rounds
        const uint8_t* msg = a.records + u * a.stride + GSW_REC_HEAD;
        const uint64_t ctr_base = ((uint64_t)nonce.y << 32) | nonce.x;      // 32-bit initial counter, the carry goes into the next word
        int acc[T];
#pragma unroll
        for (int t = 0; t < T; ++t) acc[t] = 0;
        int off[4] = {off0[0], off0[1], off0[2], off0[3]};

        for (int blk = quad; blk < a.nblk; blk += 16) {
            const uint64_t ctr = ctr_base + (uint64_t)blk;
            const uint32_t d0 = col == 0 ? (uint32_t)ctr : col == 1 ? (uint32_t)(ctr >> 32) : col == 2 ? nonce.z : nonce.w;
            uint32_t x = a0, b = b0, c = c0, d = d0;
#pragma unroll
            for (int r = 0; r < 10; ++r) {
                CHACHA_QR(x, b, c, d)
                b = quad_perm<QP_ROT1>(b); c = quad_perm<QP_ROT2>(c); d = quad_perm<QP_ROT3>(d);
                CHACHA_QR(x, b, c, d)
                b = quad_perm<QP_ROT3>(b); c = quad_perm<QP_ROT2>(c); d = quad_perm<QP_ROT1>(d);
            }
            uint32_t w[4] = {x + a0, b + b0, c + c0, d + d0};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                uint32_t m;
                if constexpr (MSG4) {
                    m = *(const uint32_t*)(msg + off[r]);
                } else {
                    m = 0u;
                    int o = off[r];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        m |= (uint32_t)msg[o] << (8 * i);
                        o = o + 1 == mb ? 0 : o + 1;
                    }
                }
                w[r] ^= m;
                off[r] += off_step;
                if (off[r] >= mb) off[r] -= mb;
            }
            if (ragged && blk == a.nblk - 1) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int valid = a.rowbytes - (64 * blk + 16 * r + 4 * col);
                    w[r] &= valid >= 4 ? 0xFFFFFFFFu : valid <= 0 ? 0u : (1u << (8 * valid)) - 1u;
                }
            }
            const uint4* sp = sfrag + 4 * blk;
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const uint4* ip = sp + t * R * rowfrags;
                const uint4 sg = ip[0];
                const uint32_t x0 = sg.x ^ w[0], x1 = sg.y ^ w[1], x2 = sg.z ^ w[2], x3 = sg.w ^ w[3];
                for (int k = 0; k < Q; ++k) {                              // run-time: Q is an argument
                    const uint4 pl = ip[(1 + k) * rowfrags];
                    int tmp = popcount_add(pl.x & x0, 0);
                    tmp = popcount_add(pl.y & x1, tmp);
                    tmp = popcount_add(pl.z & x2, tmp);
                    tmp = popcount_add(pl.w & x3, tmp);
                    acc[t] += tmp << k;
                }
            }
        }

        transpose_reduce<T, T, 1>(acc, lane);
        if (owner) list_insert(L, make_key(wtotal - 2 * acc[0], u));
        b0 = nb0; c0 = nc0; nonce = nnonce;
    }

    // ---- one list per (wave, set) -> LDS -> one per (workgroup, set)
    __syncthreads();                                   // every wave is done with the rows: reuse the LDS
    int64_t* wlist = (int64_t*)lds_raw;                // [KY_WAVES][T][TR_LIST]
    if (lane < T) put_list(wlist, wave * T + img, L);
    __syncthreads();
    workgroup_lists_to_partial<KY_WAVES, T>(wlist, img0, a.B, a.partial, a.grid_x, a.k);
}

template <bool MSG4>
int launch_pooled_scan_tile(const KeyedPooledArgs& s, const SearchPlan& p, hipStream_t st) {
    switch (p.T) {
        case 16: return launch_search(gsw_trace_keyed_pooled_scan_kernel<16, MSG4>, s, s.base, p, st);
        case 4: return launch_search(gsw_trace_keyed_pooled_scan_kernel<4, MSG4>, s, s.base, p, st);
        default: return launch_search(gsw_trace_keyed_pooled_scan_kernel<1, MSG4>, s, s.base, p, st);
    }
}

bool pool_aligned(const void* p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) == 0; }

}  // namespace

extern "C" {

int gsw_pool_rows(const uint8_t* signs_dev, const uint8_t* planes_dev, int P, int B, int64_t n_bits, const int32_t* set_ptr_dev, int G, int max_set, int Q,
                  uint8_t* out_signs_dev, uint8_t* out_planes_dev, int32_t* wsum_dev, int64_t* wsq_dev, void* stream) {
    PoolQuery q{};
    q.kind = POOL_ROWS;
    q.pointers_ok = signs_dev && set_ptr_dev && out_signs_dev && out_planes_dev && wsum_dev && wsq_dev && ((planes_dev != nullptr) == (P > 0)) &&
                    pool_aligned(set_ptr_dev, 4) && pool_aligned(wsum_dev, 4) && pool_aligned(wsq_dev, 8);
    q.rows_aligned = pool_aligned(signs_dev, 4) && pool_aligned(planes_dev, 4) && pool_aligned(out_signs_dev, 4) && pool_aligned(out_planes_dev, 4);
    q.P = P; q.B = B; q.G = G; q.max_set = max_set; q.Q = Q; q.n_bits = n_bits;
    const PoolPlan p = pool_decide(q);
    if (p.status != GSW_OK) return p.status;
    const PoolRowsArgs a{signs_dev, planes_dev, set_ptr_dev, out_signs_dev, out_planes_dev, wsum_dev, wsq_dev, B, p.Q, p.rowbytes, p.rowwords, p.rows_aligned};
    return launch_pool_rows(a, P, p, (hipStream_t)stream);
}

int gsw_trace_keyed_pooled_topk(const uint8_t* signs_dev, const uint8_t* planes_dev, const int32_t* wsum_dev, int Q, int G, int64_t n_bits,
                                const uint8_t* records_dev, int64_t record_stride, int msg_bytes, int64_t n_records, int k, int32_t* idx_dev,
                                int32_t* score_dev, void* workspace_dev, void* stream) {
    PoolQuery q{};
    q.kind = POOL_SEARCH;
    q.pointers_ok = signs_dev && planes_dev && wsum_dev && idx_dev && score_dev && workspace_dev && pool_aligned(wsum_dev, 4);
    q.rows_aligned = pool_aligned(signs_dev, 4) && pool_aligned(planes_dev, 4);
    q.records_present = records_dev != nullptr;
    q.records_aligned = pool_aligned(records_dev, 16);
    q.G = G; q.Q = Q; q.n_bits = n_bits; q.record_stride = record_stride; q.n_records = n_records; q.msg_bytes = msg_bytes; q.k = k;
    const PoolPlan p = pool_decide(q);
    if (p.status != GSW_OK) return p.status;
    SearchPlan sp{};                                   // what launch_search reads of a plan: the geometry
    sp.T = p.T; sp.grid_x = p.grid_x; sp.grid_y = p.grid_y; sp.wg = p.wg; sp.lds = p.lds;
    const KeyedArgs a{signs_dev, records_dev, (int64_t*)workspace_dev, idx_dev, score_dev, record_stride, n_records, G, k, (int)n_bits, p.rowbytes, p.nblk,
                      msg_bytes, p.grid_x, p.rows_aligned};
    const KeyedPooledArgs s{a, planes_dev, wsum_dev, p.Q};
    return p.msg4 ? launch_pooled_scan_tile<true>(s, sp, (hipStream_t)stream) : launch_pooled_scan_tile<false>(s, sp, (hipStream_t)stream);
}

}  // extern "C"
