// gswm_align_soft.inc -- every candidate alignment of gsw_level_pack's rows in one launch (gfx950): the sign row AND its P level planes, the input of
// an alignment search ranked by reliability levels.
// Included in gswm_keyed.hip after gswm_align.inc: GSW_HIP and allow_dynamic_lds are that file's, AlignMap and align_map gswm_align.inc's.
// With GSW_LEVEL_ALIGN_PLAN_ONLY defined only the launch policy below is compiled: plain host C++ that needs gswm.h and gswm_record.h alone
// (tests/level_align_plan_cases.cpp sweeps it without a GPU).
//
//   signs      : [B, n/8], planes : [B, P, n/8] as gsw_level_pack writes them; n = C H W, one bit per element (l = 1), P in 1..4
//   out_signs  : [B, A, n/8], out_planes : [B, A, P, n/8]: row (b, a) of each is bit for bit gsw_rows_align's row at l = 1
//
// A level plane is an l = 1 row, so 1 + P launches of gsw_rows_align write the same bytes -- and compute the source position of every element 1 + P
// times; that index arithmetic, not memory, bounds gsw_rows_align.  Here a lane computes the source bit of each of a word's 32 elements ONCE
// (align_gather's incremental (x, y, c, i, j) walk) and gathers that bit from the sign row and from all P planes: 1 + P accumulators, one walk.
//
// Work split as gsw_rows_align_kernel: grid (alignment chunks, images), 256 lanes, the image's 1 + P rows staged in LDS once per workgroup at a stride of
// rowbytes rounded up to 16, then the chunk's alignments one after the other.  The words of all 1 + P output rows are cut at the SAME byte offsets, those
// of the sign row's first 4-byte boundary: a row that starts at another phase (rows of 15 bytes, output pointers of different alignment) gets the word as
// four byte stores.  The head and tail bytes (at most 6 per row) are assembled one byte offset per lane, for all 1 + P rows.
//
// LDS bound.  (1 + P) padded rows of up to 65 536 bytes together are staged (gsw_rows_align's bound: two workgroups share a CU's 160 KiB); beyond it
// the rows are read in place from global memory (SG).  The domain is the soft search's: n (1 + P) <= GSW_ROW_MAX_BITS, so SG rows total at most 128 KiB.
//
// level_align_decide is the whole launch policy and every refusal; the entry point only fills LevelAlignArgs from its plan.  All arithmetic is integer.
//
// Kernel
//   gsw_level_rows_align_kernel<L, P, SG> : L bits per element (1 here; 2 and 4 are gswm_align_soft_l.inc's), P level planes (1..4), SG: the source rows are
//                                           read from global memory

namespace {

constexpr int LA_LDS_MAX_BYTES = 65536;       // the 1 + P padded rows that are staged in LDS, together
constexpr int LA_CHUNK_MAX = 16;              // alignments per workgroup, at most
constexpr int64_t LA_TARGET_WGS = 2048;       // the chunk shrinks while the grid would have fewer workgroups than this (8 per CU)

struct LevelAlignPlan {
    int status;
    int sg;                   // 1: rows read from global memory
    int chunk;                // alignments per workgroup
    int grid_x, grid_y;       // (chunks, images)
    int rowbytes;
    int lstride;              // bytes between two rows of the image in LDS (0 with sg)
    uint32_t lds;
};

// the launch decision: pure, host only.  A refusal has its status and zeros everywhere else.
inline LevelAlignPlan level_align_decide(bool pointers_ok, int P, int B, int C, int H, int W, int A) {
    LevelAlignPlan p{};
    p.status = GSW_ERR_BAD_ARG;
    if (!pointers_ok || P < 1 || P > 4 || B < 1 || C < 1 || H < 1 || W < 1 || A < 1) return p;
    const int64_t ch = (int64_t)C * H;        // (C, H, W < 2^31 each: no product overflows before it is compared)
    p.status = GSW_ERR_UNSUPPORTED;
    if (ch > GSW_ROW_MAX_BITS || ch * W * (1 + P) > GSW_ROW_MAX_BITS || B > 65535) return p;     // (B: the grid's second dimension)
    const int64_t n = ch * W;
    if (n % 8 != 0) { p.status = GSW_ERR_RAGGED; return p; }
    p.rowbytes = (int)(n / 8);
    const int padded = (p.rowbytes + 15) / 16 * 16;
    p.sg = (1 + P) * padded > LA_LDS_MAX_BYTES;
    p.lstride = p.sg ? 0 : padded;
    p.lds = p.sg ? 0u : (uint32_t)((1 + P) * padded);
    const int64_t want = (int64_t)A * B / LA_TARGET_WGS;
    p.chunk = (int)(want < 1 ? 1 : want > LA_CHUNK_MAX ? LA_CHUNK_MAX : want);
    p.grid_x = (int)(((int64_t)A + p.chunk - 1) / p.chunk);
    p.grid_y = B;
    p.status = GSW_OK;
    return p;
}

}  // namespace

#ifndef GSW_LEVEL_ALIGN_PLAN_ONLY

namespace {

constexpr int LA_WG = 256;

struct LevelAlignArgs {
    const uint8_t* signs;     // [B, rowbytes]
    const uint8_t* planes;    // [B, P, rowbytes]
    const int32_t* aligns;    // [A, 3]
    uint8_t* out_signs;       // [B, A, rowbytes]
    uint8_t* out_planes;      // [B, A, P, rowbytes]
    int C, H, W, A, chunk, rowbytes, lstride;
};

// `count` elements of L bits from output element e0 on, MSB first in the low count * L bits of acc[r], for the R rows src[0 .. R): the source group of an
// element is computed once and read from every row (L in 1, 2, 4 divides 8: a group never straddles a byte)
template <int L, int R, typename Src>
__device__ __forceinline__ void level_align_gather(const Src (&src)[R], const AlignMap& m, int e0, int count, int H, int W, uint32_t (&acc)[R]) {
    const int hw = H * W;
    const int c = e0 / hw, r = e0 - c * hw;
    int y = r / W, x = r - y * W;
    int cb = c * hw + m.s0;
    int i = y + m.i0, j = x + m.j0;
    if (i >= H) i -= H;
    if (j >= W) j -= W;
#pragma unroll
    for (int q = 0; q < R; ++q) acc[q] = 0u;
#pragma unroll 8
    for (int k = 0; k < count; ++k) {
        const uint32_t pbit = (uint32_t)(cb + i * m.si + j * m.sj) * L;
        const uint32_t at = pbit >> 3, sh = (8u - L) - (pbit & 7u);
#pragma unroll
        for (int q = 0; q < R; ++q) acc[q] = (acc[q] << L) | (((uint32_t)src[q][at] >> sh) & ((1u << L) - 1u));
        ++x;
        if (++j == W) j = 0;
        if (x == W) {
            x = 0, j = m.j0;
            ++y;
            if (++i == H) i = 0;
            if (y == H) y = 0, i = m.i0, cb += hw;
        }
    }
}

// four bytes, the lowest address first, at any alignment
__device__ __forceinline__ void level_align_store_word(uint8_t* at, uint32_t v) {
    if (((uintptr_t)at & 3u) == 0) {
        *(uint32_t*)at = v;
    } else {
        at[0] = (uint8_t)v, at[1] = (uint8_t)(v >> 8), at[2] = (uint8_t)(v >> 16), at[3] = (uint8_t)(v >> 24);
    }
}

template <int L, int P, bool SG>
__global__ __launch_bounds__(LA_WG) void gsw_level_rows_align_kernel(LevelAlignArgs s) {
    extern __shared__ __attribute__((aligned(16))) uint8_t la_lds[];
    constexpr int R = 1 + P, EPW = 32 / L, EPB = 8 / L;             // elements per output word, per byte
    const int tid = threadIdx.x, b = blockIdx.y;
    const uint8_t* src[R];
    src[0] = s.signs + (int64_t)b * s.rowbytes;
#pragma unroll
    for (int q = 1; q < R; ++q) src[q] = s.planes + ((int64_t)b * P + (q - 1)) * s.rowbytes;

    if constexpr (!SG) {                                            // ---- stage the 1 + P rows
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const uint8_t* row = src[q];
            uint8_t* dst = la_lds + q * s.lstride;
            if (((uintptr_t)row & 3u) == 0) {
                const int nw = s.rowbytes >> 2;
                for (int w = tid; w < nw; w += LA_WG) ((uint32_t*)dst)[w] = ((const uint32_t*)row)[w];
                for (int j = 4 * nw + tid; j < s.rowbytes; j += LA_WG) dst[j] = row[j];
            } else {
                for (int j = tid; j < s.rowbytes; j += LA_WG) dst[j] = row[j];
            }
            src[q] = dst;
        }
        __syncthreads();
    }

    const int a0 = blockIdx.x * s.chunk;
    const int a1 = a0 + s.chunk < s.A ? a0 + s.chunk : s.A;
    for (int a = a0; a < a1; ++a) {
        const AlignMap m = align_map(s.aligns[3 * a], s.aligns[3 * a + 1], s.aligns[3 * a + 2], s.H, s.W);
        const int64_t ba = (int64_t)b * s.A + a;
        uint8_t* orow[R];
        orow[0] = s.out_signs + ba * s.rowbytes;
#pragma unroll
        for (int q = 1; q < R; ++q) orow[q] = s.out_planes + (ba * P + (q - 1)) * s.rowbytes;
        int head = (int)((4u - (uint32_t)((uintptr_t)orow[0] & 3u)) & 3u);   // bytes in front of the sign row's first 4-byte boundary
        if (head > s.rowbytes) head = s.rowbytes;
        const int nwords = (s.rowbytes - head) >> 2;
        const int edge = s.rowbytes - 4 * nwords;                   // head + tail bytes, at most 6
        for (int w = tid; w < nwords; w += LA_WG) {
            uint32_t acc[R];
#pragma unroll
            for (int q = 0; q < R; ++q) acc[q] = 0u;
            if (m.ok) level_align_gather<L, R>(src, m, (head + 4 * w) * EPB, EPW, s.H, s.W, acc);
#pragma unroll
            for (int q = 0; q < R; ++q) level_align_store_word(orow[q] + head + 4 * w, __builtin_bswap32(acc[q]));   // MSB first: the first element lands in the lowest address
        }
        if (tid < edge) {
            const int byte = tid < head ? tid : 4 * nwords + tid;   // (tid - head) bytes past head + 4 nwords
            uint32_t acc[R];
#pragma unroll
            for (int q = 0; q < R; ++q) acc[q] = 0u;
            if (m.ok) level_align_gather<L, R>(src, m, byte * EPB, EPB, s.H, s.W, acc);
#pragma unroll
            for (int q = 0; q < R; ++q) orow[q][byte] = (uint8_t)acc[q];
        }
    }
}

template <int L, int P>
int launch_level_rows_align(const LevelAlignArgs& s, const LevelAlignPlan& p, hipStream_t st) {
    void (*kernel)(LevelAlignArgs) = p.sg ? gsw_level_rows_align_kernel<L, P, true> : gsw_level_rows_align_kernel<L, P, false>;
    GSW_HIP(allow_dynamic_lds((const void*)kernel, p.lds));
    hipLaunchKernelGGL(kernel, dim3(p.grid_x, p.grid_y), dim3(LA_WG), p.lds, st, s);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

}  // namespace

extern "C" {

int gsw_level_rows_align(const uint8_t* signs_dev, const uint8_t* planes_dev, int P, int B, int C, int H, int W, const int32_t* aligns_dev, int A,
                         uint8_t* out_signs_dev, uint8_t* out_planes_dev, void* stream) {
    const bool pointers_ok = signs_dev && planes_dev && aligns_dev && out_signs_dev && out_planes_dev && ((uintptr_t)aligns_dev & 3u) == 0;
    const LevelAlignPlan p = level_align_decide(pointers_ok, P, B, C, H, W, A);
    if (p.status != GSW_OK) return p.status;
    const LevelAlignArgs s{signs_dev, planes_dev, aligns_dev, out_signs_dev, out_planes_dev, C, H, W, A, p.chunk, p.rowbytes, p.lstride};
    switch (P) {
        case 1: return launch_level_rows_align<1, 1>(s, p, (hipStream_t)stream);
        case 2: return launch_level_rows_align<1, 2>(s, p, (hipStream_t)stream);
        case 3: return launch_level_rows_align<1, 3>(s, p, (hipStream_t)stream);
        default: return launch_level_rows_align<1, 4>(s, p, (hipStream_t)stream);
    }
}

}  // extern "C"

#endif  // GSW_LEVEL_ALIGN_PLAN_ONLY
