// gswm_trace.hip -- trace a batch of extracted vote counts to the best-matching messages of a registry, gfx950.
//
//   s[b,u] = sum_t (2 r[u,t] - 1) w[b,t]         r: registry bits (packed, MSB first), w: per-image weight row
//                                                soft: w = 2 c - V (vote margin), hard: w = +1 if c > V/2 else -1
//   out    = the k best users per image by (s descending, index ascending)
//
// The [B, U] score matrix never exists in memory and the registry is never unpacked in memory: a workgroup stages the weight rows of
// its image tile in LDS once, streams packed registry rows through registers and keeps running top-8 lists in registers.
//
// Arithmetic.  Since sum_t (2r-1) w = 2 R1 - W with R1 = sum_{t: r=1} w and W = sum_t w (one constant per image), candidates are
// ranked by R1 (strictly monotone in s for a fixed image) and the A operand of the matrix instruction is the registry bit itself as a
// 0/1 byte: expanding a bit to a byte is then a shift and a mask.  R1 goes through v_mfma_i32_16x16x64_i8: users on the rows (A),
// images on the columns (B), so by the C/D lane map (col = lane & 15, row = 4 (lane >> 4) + reg) a lane owns ONE image and four
// users per tile -- the running top-8 list is per lane and needs no cross-lane traffic until the end.
//
// K order.  Any permutation of K applied to A and B alike leaves the sum unchanged, so K is ordered for the cheapest expansion.  K is
// cut into blocks of 256 bits (32 registry bytes per row, four 64-deep steps q = 0..3).  Lane group g = lane >> 4 loads the 8 bytes
// 8g .. 8g+7 of its row's block as two dwords x[0], x[1]; operand dword dd of step q is (x[q >> 1] >> (4 (q & 1) + dd)) & 0x01010101,
// i.e. byte i of it is message bit  t = 8 (32 blk + 8 g + 4 (q >> 1) + i) + 7 - 4 (q & 1) - dd.  The weight rows are staged in LDS in
// exactly that order, as one 16-byte fragment per (step, image tile, lane): the B read is a linear ds_read_b128.  M is zero-padded to a
// multiple of 256 in K (zero weights; registry bytes past the row are read as zero, never fetched).
//
// Exactness beyond int8.  |w| <= V.  V <= 127 is one int8 plane.  Larger V uses balanced base-128 digits w = d0 + 128 d1 (+ 128^2 d2),
// d0, d1 in [-64, 63], the last digit the remainder: one accumulator set per plane, combined in int32 (|R1| <= M V < 2^31).  Two planes
// reach V = 16000, three V = 2 000 000 (beyond any lattice gsw_extract accepts).
//
// Top-k.  Keys are int64 (R1 << 32) | (0xFFFFFFFF - index): the maximum of a set of keys is the best score with the LOWEST index, keys
// are unique, so the k largest of any partition's k largest are the k largest overall -- the result depends on neither the launch
// geometry nor the order of arrival.  Lane lists -> LDS -> one list per (workgroup, image) in the caller's workspace -> gsw_trace_finish_kernel
// (one wave per image) merges them, converts R1 to s = 2 R1 - W and writes idx / score.
//
// Large registries are searched twice (sample_users below): the k-th best of a sample of the rows is a floor under the final k best.
//
// Kernels
//   gsw_trace_scan_kernel<NT, P>  : NT 16-image tiles x P planes per workgroup (NT P <= 4); 4 waves, each 4 user tiles (64 users) per pass.
//   gsw_trace_finish_kernel       : per image: merge the partial lists, W, output.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>

#include "../../include/gswm.h"
#include "gswm_host.h"   // GSW_HIP, allow_dynamic_lds
#include "gswm_topk.h"   // TR_LIST, TR_EMPTY, make_key, list_insert, merge_from_lane_xor, workgroup_lists_to_partial, wave_merge_partial

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int TR_WG = 256;               // 4 waves
constexpr int TR_UT = 4;                 // user tiles (of 16) per wave and pass
constexpr int TR_PASS_USERS = 4 * TR_UT * 16;   // users a workgroup covers per pass
constexpr int TR_MAX_GRID_X = 512;       // user ranges (two workgroups per CU)
constexpr uint32_t TR_MAX_LDS = 160u * 1024u - 64u;

struct TraceArgs {
    const uint32_t* counts;   // [B, M]
    const uint8_t* registry;  // [U, M / 8]
    int64_t* partial;         // [B16, grid_x, k]
    const int* floor;         // [B16] or null: per image, an R1 that k users are known to reach (nothing below it can be among the k best)
    int* floor_out;           // the finishing pass of the sample writes it instead of idx / score
    int32_t* idx;             // [B, k]
    int32_t* score;           // [B, k]
    int B, M, V, hard, k;
    int rowbytes;             // M / 8
    int nblk;                 // 256-bit K blocks
    int grid_x;
    int64_t U;
    int64_t passes;           // ceil(U / TR_PASS_USERS)
    int aligned;              // rows are whole, 8-byte aligned qwords
};

__device__ __forceinline__ int weight_of(uint32_t c, int V, int hard) {
    const int ci = (int)min(c, (uint32_t)V);
    if (hard) return (2 * ci > V) ? 1 : -1;          // strict majority, ties -> 0 (extract.py:99)
    return 2 * ci - V;
}

__device__ __forceinline__ uint2 load_row_qword(const TraceArgs& a, int64_t u, int byte0) {
    uint2 x = make_uint2(0u, 0u);
    const uint8_t* row = a.registry + u * (int64_t)a.rowbytes;
    if (a.aligned) {
        if (byte0 < a.rowbytes) x = *(const uint2*)(row + byte0);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (byte0 + i < a.rowbytes) x.x |= (uint32_t)row[byte0 + i] << (8 * i);
            if (byte0 + 4 + i < a.rowbytes) x.y |= (uint32_t)row[byte0 + 4 + i] << (8 * i);
        }
    }
    return x;
}

// Register budget of two waves per SIMD (256): two workgroups per CU, so that one's loads and list work run under the other's MFMAs
// (measured at B = 64, U = 2^24: 698 -> 452 us against the 326 registers / one wave per SIMD the compiler takes when left alone).
template <int NT, int P>
__global__ __launch_bounds__(TR_WG) __attribute__((amdgpu_waves_per_eu(2, 2))) void gsw_trace_scan_kernel(TraceArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
    uint32_t* wl = (uint32_t*)lds_raw;                 // [P][KS][NT][64 lanes][4 dwords]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, col = lane & 15;
    const int KS = a.nblk * 4;
    const int img0 = blockIdx.y * (NT * 16);

    // ---- stage the weight rows of this image tile, in operand order
    const int frag_dwords = KS * NT * 64 * 4;
    for (int e = tid; e < frag_dwords; e += TR_WG) {
        const int dd = e & 3, ln = (e >> 2) & 63, rest = e >> 8;
        const int nt = rest % NT, ks = rest / NT;
        const int q = ks & 3, blk = ks >> 2;
        const int b = img0 + nt * 16 + (ln & 15);
        const int byte0 = blk * 32 + 8 * (ln >> 4) + 4 * (q >> 1);
        const int bit = 7 - 4 * (q & 1) - dd;
        uint32_t packed[P];
#pragma unroll
        for (int p = 0; p < P; ++p) packed[p] = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = 8 * (byte0 + i) + bit;
            int w = 0;
            if (b < a.B && t < a.M) w = weight_of(a.counts[(int64_t)b * a.M + t], a.V, a.hard);
#pragma unroll
            for (int p = 0; p < P; ++p) {
                int d = w;
                if (p < P - 1) {
                    d = ((w + 64) & 127) - 64;
                    w = (w - d) >> 7;
                }
                packed[p] |= ((uint32_t)d & 0xFFu) << (8 * i);
            }
        }
#pragma unroll
        for (int p = 0; p < P; ++p) wl[p * frag_dwords + e] = packed[p];
    }
    __syncthreads();

    // a lane owns image nt * 16 + col of every image tile: one running list per tile
    int64_t L[NT][TR_LIST];
    int thresh[NT], fl[NT];                            // max(floor of the image, score part of L[nt][7]); columns past the batch never enter
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int b = img0 + nt * 16 + col;
        fl[nt] = thresh[nt] = (b >= a.B) ? INT_MAX : a.floor ? a.floor[b] : INT_MIN;
#pragma unroll
        for (int j = 0; j < TR_LIST; ++j) L[nt][j] = TR_EMPTY;
    }

    const int64_t p0 = a.passes * blockIdx.x / a.grid_x, p1 = a.passes * (blockIdx.x + 1) / a.grid_x;
    const v4i* wfrag = (const v4i*)lds_raw;

    uint2 cur[TR_UT], nxt[TR_UT];
    auto fetch = [&](uint2 (&dst)[TR_UT], int64_t pass, int blk) {
        const int64_t ubase = pass * TR_PASS_USERS + wave * (TR_UT * 16) + col;
#pragma unroll
        for (int ut = 0; ut < TR_UT; ++ut) {
            const int64_t u = min(ubase + ut * 16, a.U - 1);
            dst[ut] = load_row_qword(a, u, blk * 32 + 8 * g);
        }
    };
    if (p0 < p1) fetch(cur, p0, 0);

    for (int64_t pass = p0; pass < p1; ++pass) {
        v4i acc[TR_UT][NT][P];
#pragma unroll
        for (int ut = 0; ut < TR_UT; ++ut)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int p = 0; p < P; ++p) acc[ut][nt][p] = (v4i){0, 0, 0, 0};

        for (int blk = 0; blk < a.nblk; ++blk) {
            const bool last_blk = blk + 1 == a.nblk;
            if (!last_blk) fetch(nxt, pass, blk + 1);
            else if (pass + 1 < p1) fetch(nxt, pass + 1, 0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ks = blk * 4 + q;
                v4i bf[NT][P];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int p = 0; p < P; ++p) bf[nt][p] = wfrag[((p * KS + ks) * NT + nt) * 64 + lane];
#pragma unroll
                for (int ut = 0; ut < TR_UT; ++ut) {
                    const uint32_t x = ((q >> 1) ? cur[ut].y : cur[ut].x) >> (4 * (q & 1));
                    v4i af;
                    af.x = (int)(x & 0x01010101u);
                    af.y = (int)((x >> 1) & 0x01010101u);
                    af.z = (int)((x >> 2) & 0x01010101u);
                    af.w = (int)((x >> 3) & 0x01010101u);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                        for (int p = 0; p < P; ++p)
                            acc[ut][nt][p] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af, bf[nt][p], acc[ut][nt][p], 0, 0, 0);
                }
            }
#pragma unroll
            for (int ut = 0; ut < TR_UT; ++ut) cur[ut] = nxt[ut];
        }

        // ---- R1 per (user, image); a cheap maximum decides whether any of this lane's scores can enter a list
        const int64_t ubase = pass * TR_PASS_USERS + wave * (TR_UT * 16) + 4 * g;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            int r1[TR_UT][4];
            int best = INT_MIN;
#pragma unroll
            for (int ut = 0; ut < TR_UT; ++ut)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    int v = acc[ut][nt][0][r];
                    if (P > 1) v += acc[ut][nt][1][r] * 128;
                    if (P > 2) v += acc[ut][nt][2][r] * 16384;
                    r1[ut][r] = v;
                    best = max(best, v);
                }
            if (best >= thresh[nt]) {
#pragma unroll
                for (int ut = 0; ut < TR_UT; ++ut)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int64_t u = ubase + ut * 16 + r;
                        if (u < a.U && r1[ut][r] >= thresh[nt]) {
                            list_insert(L[nt], make_key(r1[ut][r], u));
                            thresh[nt] = max(fl[nt], (int)(L[nt][TR_LIST - 1] >> 32));
                        }
                    }
            }
        }
    }

    // ---- the four lane groups of a wave hold lists of the same images: fold them into lanes 0..15
#pragma unroll
    for (int step = 32; step >= 16; step >>= 1)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) merge_from_lane_xor(L[nt], step);

    __syncthreads();                                   // every wave is done with the weight fragments: reuse the LDS
    int64_t* wlist = (int64_t*)lds_raw;                // [4 waves][NT * 16 images][TR_LIST]
    if (lane < 16) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) put_list(wlist, (wave * NT + nt) * 16 + lane, L[nt]);
    }
    __syncthreads();
    workgroup_lists_to_partial<TR_WG / 64, NT * 16>(wlist, img0, a.B, a.partial, a.grid_x, a.k);
}

// one wave per image: the k largest keys of the partial lists, W = sum_t w, s = 2 R1 - W
__global__ __launch_bounds__(64) void gsw_trace_finish_kernel(TraceArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int64_t L[TR_LIST];
    wave_merge_partial(L, a.partial + (int64_t)b * a.grid_x * a.k, a.grid_x * a.k, lane);
    int W = 0;
    for (int t = lane; t < a.M; t += 64) W += weight_of(a.counts[(int64_t)b * a.M + t], a.V, a.hard);
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) W += __shfl_xor(W, step);
    if (lane == 0 && a.floor_out) {
        int64_t kth = L[0];
#pragma unroll
        for (int j = 1; j < TR_LIST; ++j)
            if (j < a.k) kth = L[j];
        a.floor_out[b] = kth == TR_EMPTY ? INT_MIN : (int)(kth >> 32);
    } else if (lane == 0) {
#pragma unroll
        for (int j = 0; j < TR_LIST; ++j) {
            if (j < a.k) {
                const int64_t key = L[j];
                const bool empty = key == TR_EMPTY;
                const int64_t r1 = key >> 32;
                a.idx[(int64_t)b * a.k + j] = empty ? -1 : (int32_t)(0xFFFFFFFFu - (uint32_t)key);
                a.score[(int64_t)b * a.k + j] = empty ? INT_MIN : (int32_t)(2 * r1 - (int64_t)W);
            }
        }
    }
}

// Registries of TR_SAMPLE_FROM users and more are searched twice: first a sample (the first 1/64 of the rows, at least 65536), whose
// k-th best R1 per image is a floor no member of the final k best can be below; with it the running lists of the full search change
// a few hundred times per image instead of at every pass, and the search runs at the speed of its matrix and expansion work.
constexpr int64_t TR_SAMPLE_FROM = (int64_t)1 << 19;
int64_t sample_users(int64_t n_users) {
    if (n_users < TR_SAMPLE_FROM) return 0;
    return std::max<int64_t>((int64_t)1 << 16, n_users / 64) / TR_PASS_USERS * TR_PASS_USERS;
}

int grid_x_for(int64_t n_users) {
    const int64_t passes = (n_users + TR_PASS_USERS - 1) / TR_PASS_USERS;
    return (int)std::min<int64_t>(passes, TR_MAX_GRID_X);
}

template <int NT, int P>
int launch_scan(const TraceArgs& a, hipStream_t st) {
    const uint32_t lds = (uint32_t)a.nblk * 4u * NT * P * 1024u;          // >= the NT * 4 KiB the final merge needs
    if (lds > TR_MAX_LDS) return GSW_ERR_UNSUPPORTED;
    GSW_HIP(allow_dynamic_lds((const void*)gsw_trace_scan_kernel<NT, P>, lds));
    const int tiles_y = (a.B + NT * 16 - 1) / (NT * 16);
    hipLaunchKernelGGL((gsw_trace_scan_kernel<NT, P>), dim3(a.grid_x, tiles_y), dim3(TR_WG), lds, st, a);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

template <int P>
int launch_scan_planes(const TraceArgs& a, hipStream_t st) {
    // image tiles per workgroup: as many as the batch needs, NT P <= 4 accumulator sets, the fragments within the LDS
    int nt = (a.B > 32) ? 4 : (a.B > 16) ? 2 : 1;
    while (nt > 1 && (nt * P > 4 || (uint32_t)a.nblk * 4u * nt * P * 1024u > 64u * 1024u)) nt >>= 1;
    if (nt == 4) {
        if constexpr (P == 1) return launch_scan<4, 1>(a, st);
    }
    if (nt == 2) {
        if constexpr (P <= 2) return launch_scan<2, P>(a, st);
    }
    return launch_scan<1, P>(a, st);
}

}  // namespace

extern "C" {

size_t gsw_trace_workspace_bytes(int B, int64_t n_users, int k) {
    if (B < 1 || n_users < 1 || n_users > (int64_t)INT32_MAX || k < 1 || k > TR_LIST) return 0;
    const size_t b16 = (size_t)((B + 15) / 16 * 16);
    return b16 * sizeof(int64_t) /* floors */ + b16 * (size_t)grid_x_for(n_users) * (size_t)k * sizeof(int64_t);
}

int gsw_trace_topk(const uint32_t* counts_dev, int B, int msg_bits, int copies, int mode, const uint8_t* registry_dev, int64_t n_users, int k,
                   int32_t* idx_dev, int32_t* score_dev, void* workspace_dev, void* stream) {
    if (!counts_dev || !registry_dev || !idx_dev || !score_dev || !workspace_dev) return GSW_ERR_BAD_ARG;
    if (B < 1 || msg_bits < 8 || msg_bits > 2048 || (msg_bits & 7) || copies < 1 || k < 1 || k > TR_LIST) return GSW_ERR_BAD_ARG;
    if (n_users < 1 || n_users > (int64_t)INT32_MAX || (mode != GSW_TRACE_SOFT && mode != GSW_TRACE_HARD)) return GSW_ERR_BAD_ARG;
    if ((int64_t)msg_bits * copies >= ((int64_t)1 << 31)) return GSW_ERR_UNSUPPORTED;
    const int hard = mode == GSW_TRACE_HARD;
    const int planes = (hard || copies <= 127) ? 1 : (copies <= 16000) ? 2 : (copies <= 2000000) ? 3 : 0;
    if (!planes || B > 65535 * 16) return GSW_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    TraceArgs a;
    a.counts = counts_dev;
    a.registry = registry_dev;
    const size_t b16 = (size_t)((B + 15) / 16 * 16);
    int* floors = (int*)workspace_dev;
    a.partial = (int64_t*)workspace_dev + b16;
    a.floor = nullptr;
    a.floor_out = nullptr;
    a.idx = idx_dev;
    a.score = score_dev;
    a.B = B; a.M = msg_bits; a.V = copies; a.hard = hard; a.k = k;
    a.rowbytes = msg_bits / 8;
    a.nblk = (msg_bits + 255) / 256;
    a.U = n_users;
    a.passes = (n_users + TR_PASS_USERS - 1) / TR_PASS_USERS;
    a.grid_x = grid_x_for(n_users);
    a.aligned = (a.rowbytes % 8 == 0) && ((uintptr_t)registry_dev % 8 == 0);
    auto scan = [&](const TraceArgs& x) { return planes == 1 ? launch_scan_planes<1>(x, st) : planes == 2 ? launch_scan_planes<2>(x, st) : launch_scan_planes<3>(x, st); };
    if (const int64_t sample = sample_users(n_users)) {
        TraceArgs s = a;
        s.U = sample;
        s.passes = sample / TR_PASS_USERS;
        s.grid_x = grid_x_for(sample);
        int rc = scan(s);
        if (rc != GSW_OK) return rc;
        s.floor_out = floors;
        hipLaunchKernelGGL(gsw_trace_finish_kernel, dim3(B), dim3(64), 0, st, s);
        GSW_HIP(hipGetLastError());
        a.floor = floors;
    }
    int rc = scan(a);
    if (rc != GSW_OK) return rc;
    hipLaunchKernelGGL(gsw_trace_finish_kernel, dim3(B), dim3(64), 0, st, a);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

}  // extern "C"
