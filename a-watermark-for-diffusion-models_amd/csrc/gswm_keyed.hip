// gswm_keyed.hip -- trace a batch of packed sign rows to the best-matching records of a registry whose records carry their own
// ChaCha20 key and nonce, gfx950.
//
//   e[u]   = keystream(key_u, nonce_u) ^ (message_u repeated)     the cipher bits gsw_embed plants for record u (its codeword)
//   s[b,u] = n - 2 popcount(h[b] ^ e[u])                          h: the image's quantised sign bits (gsw_sign_pack), n lattice bits
//   out    = the k best records per image by (s descending, index ascending)
//
// Decrypting the image under key_u and comparing with message_u is the same as comparing h with e[u], so an image is quantised and
// packed once whatever the number of keys, and for records that share one key s is gsw_trace_topk's soft score exactly.  Neither the
// [B, U] score matrix nor any codeword exists in memory: a record is read as its 48 + msg_bytes bytes and its keystream is generated
// in registers.
//
// Work split.  A workgroup stages the packed sign rows of its tile of T images in LDS once; its waves walk the records of the
// workgroup's range, ONE record per wave at a time.  Lane = 4 quad + col: the quad computes ChaCha20 block blk = quad, quad + 16, ...
// of the record with the four-lanes-per-block code of gswm_chacha.h, so after the rounds lane col holds state words col, 4 + col,
// 8 + col, 12 + col of the block: keystream bytes 64 blk + 16 r + 4 col + (0..3), r = 0..3.  The message is XORed in at byte offset
// (64 blk + 16 r + 4 col) mod msg_bytes (offsets advance by 1024 mod msg_bytes per step and wrap by compare: no division in the loop).
//
// LDS layout.  The sign words of an image are stored in exactly that order -- word (16 blk + 4 r + col) of the row at position
// 16 blk + 4 col + r -- so a lane's four words of a block are one 16-byte fragment and the 64 lanes of a wave read 1 KiB linearly
// (ds_read_b128, conflict-free; stored naively the lanes would sit 64 bytes apart, four to a bank).  Rows are zero-padded to whole
// blocks and codeword bytes past the lattice are masked to zero, so a partial last block adds nothing.
//
// Scoring is v_xor + v_bcnt_u32_b32 (the popcount's add operand is the running sum) on the vector pipe, not the int8 matrix pipe of
// gswm_trace.hip: the operand here is born in registers one block at a time, as 1-bit values; the matrix instruction wants it
// expanded to one byte per bit (8 shift-and-mask operations per dword and image tile, as many as the xor + popcount of the whole
// comparison) and 16 records side by side per tile, which would need the keystreams of 16 records transposed through LDS.
//
// Reduction.  After the blocks a lane holds T partial sums (one per image) and the record's sum is spread over the 64 lanes.  A
// transposing butterfly (step s: the lanes with bit s clear keep the lower half of their sums and take the partner's, the others the
// upper half) ends with lane l holding the total of ONE image, img(l), after T - 1 + max(0, 6 - log2 T) shuffles instead of 6 T:
// lanes 0 .. T-1 then own one image each and keep its running top-8 list in registers, as the lanes of gswm_trace.hip do.
//
// Top-k.  gswm_topk.h: int64 keys (score << 32) | (0xFFFFFFFF - index); lane lists -> LDS -> one list per (workgroup, image) in the
// caller's workspace -> gsw_trace_keyed_finish_kernel (one wave per image).  The result depends on neither geometry nor arrival order.
//
// Host side.  search_decide (gswm_search_plan.h, host-only: tests/test_search_plan_host.py tabulates it) refuses or plans a launch of this search, of the
// level-weighted one and of the key search; an entry point fills KeyedArgs from the plan (keyed_args), dispatches the template and launches scan + finish
// (launch_search).  The workspace queries answer through the same header.
//
// Kernels
//   gsw_trace_keyed_scan_kernel<T, MSG4> : T in {1, 4, 16, 64} images per workgroup; MSG4: msg_bytes % 4 == 0 (message read as dwords)
//   gsw_trace_keyed_finish_kernel        : per image: merge the partial lists, output.
//   (gswm_keyed_soft.inc, included at the end: gsw_trace_keyed_soft_scan_kernel<T, MSG4, P>, the level-weighted search)
//   (gswm_keysearch.inc, included after it: gsw_key_search_scan_kernel<PL, SG>, the blind key search)
//   (gswm_keysearch_soft.inc, after that: gsw_key_search_soft_scan_kernel<CP, P, SG>, the blind key search ranked by reliability levels)
//   (gswm_pool.inc, last: gsw_pool_rows_kernel<P> and gsw_trace_keyed_pooled_scan_kernel<T, MSG4>, the images of a set pooled and searched as one row)
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "../../include/gswm.h"
#include "gswm_host.h"     // GSW_HIP, allow_dynamic_lds
#include "gswm_record.h"   // the record: GSW_REC_HEAD, GSW_ROW_MAX_BITS (and gswm_chacha.h: CHACHA_QR, quad_perm)
#include "gswm_search_plan.h"   // search_decide: every refusal and every launch decision of the three searches; KY_WAVES, KY_WG, KS_WG
#include "gswm_keysearch_soft_plan.h"   // key_soft_decide: the same for the level-weighted key search
#include "gswm_counts_align_plan.h"   // counts_align_decide: the same for the vote counts of every alignment under one key
#include "gswm_counts_align_soft_plan.h"   // level_counts_align_decide: the same for the level-weighted vote of every alignment under one key
#include "gswm_counts_align_soft_l_plan.h"   // level_counts_align_l_decide: the same at l = 2, 4 (rows of n l bits)
#include "gswm_pool_plan.h"   // pool_decide: the same for pooling the images of a set and for the record walk over pooled rows
#include "gswm_topk.h"

namespace {

static_assert(SEARCH_LIST == TR_LIST, "gswm_search_plan.h sizes the workspace and the top-k tail's LDS for gswm_topk.h's lists");

struct KeyedArgs {
    const uint8_t* signs;     // [B, rowbytes]
    const uint8_t* records;   // [U, stride]
    int64_t* partial;         // [B, grid_x, k]
    int32_t* idx;             // [B, k]
    int32_t* score;           // [B, k]
    int64_t stride, U;
    int B, k, n_bits;
    int rowbytes;             // n_bits / 8
    int nblk;                 // ChaCha blocks per codeword, the last one possibly partial
    int msg_bytes;
    int grid_x;
    int signs_aligned;        // sign rows are whole, 4-byte aligned dwords
};

// popcount(x) + sum in one instruction.  Written as C the compiler re-associates the four popcounts of a fragment into zero-operand
// v_bcnt_u32_b32 plus two v_add3_u32 per image; the asm keeps the running sum in the add operand.
__device__ __forceinline__ int popcount_add(uint32_t x, int sum) {
    int r;
    asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(sum));
    return r;
}

// Sums v[0..CNT) over the lanes whose ids differ in bits S, 2 S, ..: while more than one sum is left, a lane keeps one half and hands
// the other to its partner; v[0] of lane l ends as the wave's total for image lane_image<T>(l).
template <int T, int CNT, int S>
__device__ __forceinline__ void transpose_reduce(int (&v)[T], int lane) {
    if constexpr (S < 64) {
        if constexpr (CNT > 1) {
            constexpr int H = CNT / 2;
            const bool up = (lane & S) != 0;
#pragma unroll
            for (int j = 0; j < H; ++j) {
                const int send = up ? v[j] : v[j + H];
                const int keep = up ? v[j + H] : v[j];
                v[j] = keep + __shfl_xor(send, S);
            }
            transpose_reduce<T, H, S * 2>(v, lane);
        } else {
            v[0] += __shfl_xor(v[0], S);
            transpose_reduce<T, 1, S * 2>(v, lane);
        }
    }
}

template <int T>
__device__ __forceinline__ int lane_image(int lane) {
    int img = 0;
#pragma unroll
    for (int i = 0; (T >> (i + 1)) > 0; ++i) img += ((lane >> i) & 1) * (T >> (i + 1));
    return img;
}

// The record loop keeps its own copy of the block function (gswm_chacha.h's chacha20_block, with the prefetched words in a CipherLane) and
// of the repeated message word (gswm_record.h's repeated_msg_word): moved onto the shared helpers the T = 64 instantiation ran 3 to 15 %
// slower on the MI355X (the table of the discarded helper version in profiles/record_refactor_ab.txt), for a reason the resource figures
// do not show.  A change to the counter rule or the record head is made here, in chacha20_block and in chacha20_blocks_to_lds.  The tail
// after the loop is gswm_topk.h's.
template <int T, bool MSG4>
__global__ __launch_bounds__(KY_WG) void gsw_trace_keyed_scan_kernel(KeyedArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    uint32_t* sw = (uint32_t*)lds_raw;                 // [T][nblk][4 cols][4 rows]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int quad = lane >> 2, col = lane & 3;
    const int rowwords = a.nblk * 16;
    const int img0 = blockIdx.y * T;

    // ---- stage the sign rows of this image tile, in operand order
    for (int t = 0; t < T; ++t) {
        const int b = img0 + t;
        const uint8_t* row = a.signs + (int64_t)b * a.rowbytes;
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
            sw[t * rowwords + w] = x;
        }
    }
    __syncthreads();

    int64_t L[TR_LIST];
#pragma unroll
    for (int j = 0; j < TR_LIST; ++j) L[j] = TR_EMPTY;
    const int img = lane_image<T>(lane);
    const bool owner = lane < T && img0 + img < a.B;

    // message byte offsets of this lane's four words in its first block; every step of 16 blocks moves them by 1024 mod msg_bytes
    const int mb = a.msg_bytes;
    int off0[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) off0[r] = (64 * quad + 16 * r + 4 * col) % mb;
    const int off_step = 1024 % mb;
    const bool ragged = (a.rowbytes & 63) != 0;

    const uint32_t a0 = col == 0 ? 0x61707865u : col == 1 ? 0x3320646eu : col == 2 ? 0x79622d32u : 0x6b206574u;
    const uint4* sfrag = (const uint4*)lds_raw + col;  // + 4 blk + t rowwords / 4

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
                const uint4 s = sp[t * (rowwords / 4)];
                acc[t] = popcount_add(s.x ^ w[0], acc[t]);
                acc[t] = popcount_add(s.y ^ w[1], acc[t]);
                acc[t] = popcount_add(s.z ^ w[2], acc[t]);
                acc[t] = popcount_add(s.w ^ w[3], acc[t]);
            }
        }

        transpose_reduce<T, T, 1>(acc, lane);
        if (owner) list_insert(L, make_key(a.n_bits - 2 * acc[0], u));
        b0 = nb0; c0 = nc0; nonce = nnonce;
    }

    // ---- one list per (wave, image) -> LDS -> one per (workgroup, image)
    __syncthreads();                                   // every wave is done with the sign rows: reuse the LDS
    int64_t* wlist = (int64_t*)lds_raw;                // [KY_WAVES][T][TR_LIST]
    if (lane < T) put_list(wlist, wave * T + img, L);
    __syncthreads();
    workgroup_lists_to_partial<KY_WAVES, T>(wlist, img0, a.B, a.partial, a.grid_x, a.k);
}

// one wave per image: the k largest keys of the partial lists
__global__ __launch_bounds__(64) void gsw_trace_keyed_finish_kernel(KeyedArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int64_t L[TR_LIST];
    wave_merge_partial(L, a.partial + (int64_t)b * a.grid_x * a.k, a.grid_x * a.k, lane);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < TR_LIST; ++j) {
            if (j < a.k) {
                const int64_t key = L[j];
                const bool empty = key == TR_EMPTY;
                a.idx[(int64_t)b * a.k + j] = empty ? -1 : (int32_t)(0xFFFFFFFFu - (uint32_t)key);
                a.score[(int64_t)b * a.k + j] = empty ? INT_MIN : (int32_t)(key >> 32);
            }
        }
    }
}

// ---- the host side of the three searches: search_decide (gswm_search_plan.h) decides, these fill the arguments from its plan and launch

SearchQuery search_query(int kind, const void* signs, const void* planes, const void* wsum, const void* records, bool outputs, int B, int64_t n_bits,
                         int64_t record_stride, int msg_bytes, int64_t n_records, int k, int levels) {
    auto aligned = [](const void* p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) == 0; };
    return SearchQuery{kind, B, n_bits, record_stride, n_records, msg_bytes, k, levels, aligned(signs, 4), aligned(planes, 4), aligned(wsum, 4), aligned(records, 16),
                       !signs, !planes, !wsum, !records, !outputs};
}

KeyedArgs keyed_args(const SearchQuery& q, const SearchPlan& p, const uint8_t* signs, const uint8_t* records, void* workspace, int32_t* idx, int32_t* score) {
    return KeyedArgs{signs, records, (int64_t*)workspace, idx, score, q.record_stride, q.n_records, q.B, q.k, (int)q.n_bits, p.rowbytes, p.nblk, q.msg_bytes,
                     p.grid_x, p.signs_aligned};
}

// A scan kernel with the plan's grid and LDS, then the finish kernel.
template <typename Args>
int launch_search(void (*scan)(Args), const Args& args, const KeyedArgs& a, const SearchPlan& p, hipStream_t st) {
    GSW_HIP(allow_dynamic_lds((const void*)scan, p.lds));
    hipLaunchKernelGGL(scan, dim3(p.grid_x, p.grid_y), dim3(p.wg), p.lds, st, args);
    GSW_HIP(hipGetLastError());
    hipLaunchKernelGGL(gsw_trace_keyed_finish_kernel, dim3(a.B), dim3(64), 0, st, a);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

template <bool MSG4>
int launch_scan_tile(const KeyedArgs& a, const SearchPlan& p, hipStream_t st) {
    switch (p.T) {
        case 64: return launch_search(gsw_trace_keyed_scan_kernel<64, MSG4>, a, a, p, st);
        case 16: return launch_search(gsw_trace_keyed_scan_kernel<16, MSG4>, a, a, p, st);
        case 4: return launch_search(gsw_trace_keyed_scan_kernel<4, MSG4>, a, a, p, st);
        default: return launch_search(gsw_trace_keyed_scan_kernel<1, MSG4>, a, a, p, st);
    }
}

}  // namespace

extern "C" {

size_t gsw_trace_keyed_workspace_bytes(int B, int64_t n_records, int k) {
    return search_workspace_bytes(SEARCH_SIGN, B, n_records, k);
}

int gsw_trace_keyed_topk(const uint8_t* signs_dev, int B, int64_t n_bits, const uint8_t* records_dev, int64_t record_stride, int msg_bytes,
                         int64_t n_records, int k, int32_t* idx_dev, int32_t* score_dev, void* workspace_dev, void* stream) {
    const SearchQuery q = search_query(SEARCH_SIGN, signs_dev, nullptr, nullptr, records_dev, idx_dev && score_dev && workspace_dev, B, n_bits, record_stride,
                                       msg_bytes, n_records, k, 0);
    const SearchPlan p = search_decide(q);
    if (p.status != GSW_OK) return p.status;
    const KeyedArgs a = keyed_args(q, p, signs_dev, records_dev, workspace_dev, idx_dev, score_dev);
    return p.msg4 ? launch_scan_tile<true>(a, p, (hipStream_t)stream) : launch_scan_tile<false>(a, p, (hipStream_t)stream);
}

}  // extern "C"

#include "gswm_keyed_soft.inc"   // gsw_trace_keyed_soft_topk: the same search ranked by reliability-weighted margins
#include "gswm_keysearch.inc"    // gsw_key_search_topk: every key of a keyring scored without a message
#include "gswm_keysearch_soft.inc"   // gsw_key_search_soft_topk: the same search ranked by reliability levels
#include "gswm_align.inc"        // gsw_rows_align: every candidate alignment of a packed row, the input of an alignment search
#include "gswm_align_soft.inc"   // gsw_level_rows_align: the same for a sign row and its level planes, one index walk for all of them
#include "gswm_counts_align.inc" // gsw_counts_align: the vote counts of every candidate alignment under one key, the operand of an aligned registry search
#include "gswm_counts_align_soft.inc" // gsw_level_counts_align: the same for gsw_level_pack's rows, the level-weighted vote of every alignment
#include "gswm_align_soft_l.inc" // gsw_level_rows_align_l: gsw_level_rows_align for gsw_level_pack_l's rows (l = 2, 4), one index walk per element
#include "gswm_counts_align_soft_l.inc" // gsw_level_counts_align_l: gsw_level_counts_align for those rows
#include "gswm_pool.inc"         // gsw_pool_rows, gsw_trace_keyed_pooled_topk: the images of a set pooled into one row, and the record walk for its up to 10 planes
