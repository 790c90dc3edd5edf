// gswm_keyed_soft.inc -- the keyed registry search ranked by reliability-weighted margins (gfx950).  Included at the end of gswm_keyed.hip: the
// record walk, transpose_reduce, lane_image, popcount_add, the finish kernel and gswm_topk.h are that file's, used as they are.
//
//   level_j     = the reliability level of lattice element j of image b, 0 .. levels (gsw_level_pack), levels in 1 .. 15
//   score[b, u] = sum_j level_j (1 - 2 (h_j ^ e[u]_j))                                    h: the sign row, e[u]: the codeword of record u
//               = W_b - 2 sum_{k < P} 2^k popcount(plane_k[b] & (h[b] ^ e[u]))            W_b = sum_j level_j (gsw_level_pack's wsum)
//   plane_k     = bit k of the levels, packed as the sign row; P = bit length of `levels`, 1 .. 4
//   out         = the k best records per image by (score descending, index ascending)
//
// The structure is gsw_trace_keyed_scan_kernel's with one more template parameter: a workgroup stages, per image of its tile, the sign row
// and the P plane rows in LDS -- [T][1 + P][nblk][4 cols][4 rows] words, every row in the operand order of the sign search, so a lane's
// four words of a block are one 16-byte fragment of every row and a wave reads 1 KiB linearly per row.  Per codeword word a lane forms
// x = s ^ w once, then per plane v_and + v_bcnt_u32_b32 into a temporary of that plane (plane 0 counts straight into the image's
// accumulator); the temporaries fold into the accumulator by shift-adds: P - 1 temporaries, not P x T accumulators.  The tile is the
// largest T in {1, 4, 16, 64} that the batch fills and whose (1 + P) T nblk 64 bytes fit the 128 KiB of the sign search's tile (search_decide): T
// decides who computes, never what.  Rows are zero-padded to whole blocks and codeword bytes past the lattice are masked, as there.
//
// The sign search itself is NOT this kernel with P = 0: its record loop stays as it was measured (profiles/trace_keyed_bench.txt).
// One shared force-inlined body with an `if constexpr (P == 0)` branch was tried at compile level: all 40 instantiations came out with other instruction
// streams (VGPRs: sign T = 64 134 -> 136 with MSG4, 146 -> 150 without; soft<4, false, *> 80 -> 95), the soft ones too, where only the wrapping changed.
//
// Host side: search_decide (gswm_search_plan.h) refuses or plans; the entry point fills the arguments from the plan and dispatches the template.
//
// Kernel
//   gsw_trace_keyed_soft_scan_kernel<T, MSG4, P> : T images per workgroup; MSG4: msg_bytes % 4 == 0; P planes
//   (gsw_trace_keyed_finish_kernel of gswm_keyed.hip finishes)

namespace {

struct KeyedSoftArgs {
    KeyedArgs base;           // the sign search's arguments (the finish kernel takes them as they are); signs_aligned covers the planes too
    const uint8_t* planes;    // [B, P, rowbytes]
    const int32_t* wsum;      // [B]
};

template <int T, bool MSG4, int P>
__global__ __launch_bounds__(KY_WG) void gsw_trace_keyed_soft_scan_kernel(KeyedSoftArgs s) {
    const KeyedArgs& a = s.base;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    uint32_t* sw = (uint32_t*)lds_raw;                 // [T][1 + P][nblk][4 cols][4 rows]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int quad = lane >> 2, col = lane & 3;
    const int rowwords = a.nblk * 16;
    const int img0 = blockIdx.y * T;

    // ---- stage the sign row and the plane rows of this image tile, in operand order
    for (int tr = 0; tr < T * (1 + P); ++tr) {
        const int t = tr / (1 + P), r = tr % (1 + P);
        const int b = img0 + t;
        const uint8_t* row = r == 0 ? a.signs + (int64_t)b * a.rowbytes : s.planes + ((int64_t)b * P + (r - 1)) * a.rowbytes;
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
    const uint4* sfrag = (const uint4*)lds_raw + col;  // + 4 blk + (t (1 + P) + row) rowfrags

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
                const uint4* ip = sp + t * (1 + P) * rowfrags;
                const uint4 sg = ip[0];
                const uint32_t x0 = sg.x ^ w[0], x1 = sg.y ^ w[1], x2 = sg.z ^ w[2], x3 = sg.w ^ w[3];
#pragma unroll
                for (int k = 0; k < P; ++k) {
                    const uint4 pl = ip[(1 + k) * rowfrags];
                    int tmp = k == 0 ? acc[t] : 0;                         // plane 0 has weight 1: straight into the accumulator
                    tmp = popcount_add(pl.x & x0, tmp);
                    tmp = popcount_add(pl.y & x1, tmp);
                    tmp = popcount_add(pl.z & x2, tmp);
                    tmp = popcount_add(pl.w & x3, tmp);
                    acc[t] = k == 0 ? tmp : acc[t] + (tmp << k);
                }
            }
        }

        transpose_reduce<T, T, 1>(acc, lane);
        if (owner) list_insert(L, make_key(wtotal - 2 * acc[0], u));
        b0 = nb0; c0 = nc0; nonce = nnonce;
    }

    // ---- one list per (wave, image) -> LDS -> one per (workgroup, image)
    __syncthreads();                                   // every wave is done with the rows: reuse the LDS
    int64_t* wlist = (int64_t*)lds_raw;                // [KY_WAVES][T][TR_LIST]
    if (lane < T) put_list(wlist, wave * T + img, L);
    __syncthreads();
    workgroup_lists_to_partial<KY_WAVES, T>(wlist, img0, a.B, a.partial, a.grid_x, a.k);
}

template <bool MSG4, int P>
int launch_soft_scan_tile(const KeyedSoftArgs& s, const SearchPlan& p, hipStream_t st) {
    switch (p.T) {
        case 64: return launch_search(gsw_trace_keyed_soft_scan_kernel<64, MSG4, P>, s, s.base, p, st);
        case 16: return launch_search(gsw_trace_keyed_soft_scan_kernel<16, MSG4, P>, s, s.base, p, st);
        case 4: return launch_search(gsw_trace_keyed_soft_scan_kernel<4, MSG4, P>, s, s.base, p, st);
        default: return launch_search(gsw_trace_keyed_soft_scan_kernel<1, MSG4, P>, s, s.base, p, st);
    }
}

template <bool MSG4>
int launch_soft_scan_planes(const KeyedSoftArgs& s, const SearchPlan& p, hipStream_t st) {
    switch (p.planes) {
        case 1: return launch_soft_scan_tile<MSG4, 1>(s, p, st);
        case 2: return launch_soft_scan_tile<MSG4, 2>(s, p, st);
        case 3: return launch_soft_scan_tile<MSG4, 3>(s, p, st);
        default: return launch_soft_scan_tile<MSG4, 4>(s, p, st);
    }
}

}  // namespace

extern "C" {

int gsw_trace_keyed_soft_topk(const uint8_t* signs_dev, const uint8_t* planes_dev, const int32_t* wsum_dev, int levels, int B, int64_t n_bits,
                              const uint8_t* records_dev, int64_t record_stride, int msg_bytes, int64_t n_records, int k, int32_t* idx_dev,
                              int32_t* score_dev, void* workspace_dev, void* stream) {
    const SearchQuery q = search_query(SEARCH_LEVEL, signs_dev, planes_dev, wsum_dev, records_dev, idx_dev && score_dev && workspace_dev, B, n_bits,
                                       record_stride, msg_bytes, n_records, k, levels);
    const SearchPlan p = search_decide(q);
    if (p.status != GSW_OK) return p.status;
    const KeyedSoftArgs s{keyed_args(q, p, signs_dev, records_dev, workspace_dev, idx_dev, score_dev), planes_dev, wsum_dev};
    return p.msg4 ? launch_soft_scan_planes<true>(s, p, (hipStream_t)stream) : launch_soft_scan_planes<false>(s, p, (hipStream_t)stream);
}

}  // extern "C"
