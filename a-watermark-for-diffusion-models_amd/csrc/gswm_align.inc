// gswm_align.inc -- every candidate alignment of a packed quantised row in one launch (gfx950): the input of an alignment search.
// Included at the end of gswm_keyed.hip: GSW_HIP, allow_dynamic_lds and GSW_ROW_MAX_BITS are that file's.
//
//   in      : row b of gsw_quant_pack / gsw_sign_pack.  Element e = (c H + y) W + x owns bits [e l, e l + l), MSB first; byte j holds bits 8 j .. 8 j + 7
//   a       = (d, dy, dx): flip the last axis if d & 4, turn d & 3 quarter turns counterclockwise (torch.rot90), roll cyclically by (dy, dx)
//   out     : row (b, a) = the packed row of that transform of image b's [C, H, W] lattice: a permutation of l-bit groups, no arithmetic on values
//
// The inverse map is affine.  With i = (y - dy) mod H and j = (x - dx) mod W the source element of output element (c, y, x) is
//   c H W + s0 + i si + j sj          (s0, si, sj) from d alone: the quarter turns give (p, q) = (i, j), (j, W-1-i), (H-1-i, W-1-j), (H-1-j, i),
//                                     the flip replaces q by W-1-q, and the source is p W + q
// so one kernel serves all eight d.  An entry with d outside 0..7, or an odd d on a non-square lattice, has no such map: its row is written as zeros
// (the wrapper refuses such a list before it is uploaded; the entry point sees a device pointer and cannot).
//
// Work split.  Grid (alignment chunks, images), 256 lanes.  A workgroup stages its image's row in LDS once, then walks the `chunk` alignments of its chunk.  Per
// alignment every lane assembles whole 32-bit words of the output row, 32 / l elements each: (c, y, x) of the word's first element by two divisions, then x, y, c
// and i, j advance by increments with wrap -- no division per element.  The word is built MSB first and byte-swapped, so the stores are coalesced dwords; the
// bytes in front of the first 4-byte boundary of an output row and behind the last (rows of 15 or 425 bytes start at any address) are assembled one byte per lane.
//
// LDS bound.  Rows of up to 65 536 bytes (524 288 bits) are staged: two workgroups still share a CU's 160 KiB, and the kernel search's bound (523 264 bits + a
// keystream) is of the same size.  Longer rows (up to GSW_ROW_MAX_BITS) are read in place from global memory (SG), as the key search reads them.
//
// align_decide is the whole launch policy and every refusal; the entry point only fills AlignArgs from its plan.  All arithmetic is integer.
//
// Kernel
//   gsw_rows_align_kernel<L, SG> : L bits per element (1, 2, 4), SG: the source row is read from global memory

namespace {

constexpr int AL_WG = 256;
constexpr int AL_LDS_MAX_BYTES = 65536;       // the longest row that is staged in LDS
constexpr int AL_CHUNK_MAX = 16;              // alignments per workgroup, at most
constexpr int64_t AL_TARGET_WGS = 2048;       // the chunk shrinks while the grid would have fewer workgroups than this (8 per CU)

struct AlignPlan {
    int status;
    int sg;                   // 1: rows read from global memory
    int chunk;                // alignments per workgroup
    int grid_x, grid_y;       // (chunks, images)
    int rowbytes;
    uint32_t lds;
};

// the launch decision: pure, host only
inline AlignPlan align_decide(bool pointers_ok, int B, int C, int H, int W, int l, int A) {
    AlignPlan p{};
    p.status = GSW_ERR_BAD_ARG;
    if (!pointers_ok || B < 1 || C < 1 || H < 1 || W < 1 || A < 1 || (l != 1 && l != 2 && l != 4)) return p;
    const int64_t ch = (int64_t)C * H;        // (C, H, W < 2^31 each: no product overflows before it is compared)
    p.status = GSW_ERR_UNSUPPORTED;
    if (ch > GSW_ROW_MAX_BITS || ch * W * l > GSW_ROW_MAX_BITS || B > 65535) return p;     // (B: the grid's second dimension)
    const int64_t n_bits = ch * W * l;
    if (n_bits % 8 != 0) { p.status = GSW_ERR_RAGGED; return p; }
    p.rowbytes = (int)(n_bits / 8);
    p.sg = p.rowbytes > AL_LDS_MAX_BYTES;
    p.lds = p.sg ? 0u : (uint32_t)((p.rowbytes + 15) / 16 * 16);
    const int64_t want = (int64_t)A * B / AL_TARGET_WGS;
    p.chunk = (int)(want < 1 ? 1 : want > AL_CHUNK_MAX ? AL_CHUNK_MAX : want);
    p.grid_x = (A + p.chunk - 1) / p.chunk;
    p.grid_y = B;
    p.status = GSW_OK;
    return p;
}

struct AlignArgs {
    const uint8_t* rows;      // [B, rowbytes]
    const int32_t* aligns;    // [A, 3]
    uint8_t* out;             // [B, A, rowbytes]
    int C, H, W, A, chunk, rowbytes;
};

// the transform of one alignment as the kernel uses it (the same in every lane)
struct AlignMap {
    int s0, si, sj;           // source element of (c, i, j) = c H W + s0 + i si + j sj
    int i0, j0;               // i at y = 0, j at x = 0
    bool ok;
};

__device__ __forceinline__ AlignMap align_map(int d, int dy, int dx, int H, int W) {
    AlignMap m;
    m.ok = d >= 0 && d <= 7 && (!(d & 1) || H == W);
    int p0, pi, pj, q0, qi, qj;                                     // p = p0 + pi i + pj j (the row of the flipped lattice), q likewise (its column)
    switch (d & 3) {
        case 0: p0 = 0, pi = 1, pj = 0, q0 = 0, qi = 0, qj = 1; break;
        case 1: p0 = 0, pi = 0, pj = 1, q0 = W - 1, qi = -1, qj = 0; break;
        case 2: p0 = H - 1, pi = -1, pj = 0, q0 = W - 1, qi = 0, qj = -1; break;
        default: p0 = H - 1, pi = 0, pj = -1, q0 = 0, qi = 1, qj = 0; break;
    }
    if (d & 4) q0 = W - 1 - q0, qi = -qi, qj = -qj;
    m.s0 = p0 * W + q0;
    m.si = pi * W + qi;
    m.sj = pj * W + qj;
    int sy = dy % H, sx = dx % W;                                   // once per alignment
    if (sy < 0) sy += H;
    if (sx < 0) sx += W;
    m.i0 = sy ? H - sy : 0;
    m.j0 = sx ? W - sx : 0;
    return m;
}

// `count` elements from output element e0 on, MSB first in the low count * L bits; src: the packed source row (LDS or global memory)
template <int L, typename Src>
__device__ __forceinline__ uint32_t align_gather(Src src, const AlignMap& m, int e0, int count, int H, int W) {
    const int hw = H * W;
    const int c = e0 / hw, r = e0 - c * hw;
    int y = r / W, x = r - y * W;
    int cb = c * hw + m.s0;
    int i = y + m.i0, j = x + m.j0;
    if (i >= H) i -= H;
    if (j >= W) j -= W;
    uint32_t acc = 0u;
#pragma unroll 8
    for (int k = 0; k < count; ++k) {
        const uint32_t pbit = (uint32_t)(cb + i * m.si + j * m.sj) * L;
        acc = (acc << L) | (((uint32_t)src[pbit >> 3] >> (8 - L - (pbit & 7u))) & ((1u << L) - 1u));
        ++x;
        if (++j == W) j = 0;
        if (x == W) {
            x = 0, j = m.j0;
            ++y;
            if (++i == H) i = 0;
            if (y == H) y = 0, i = m.i0, cb += hw;
        }
    }
    return acc;
}

template <int L, bool SG>
__global__ __launch_bounds__(AL_WG) void gsw_rows_align_kernel(AlignArgs s) {
    extern __shared__ __attribute__((aligned(16))) uint8_t al_lds[];
    const int tid = threadIdx.x, b = blockIdx.y;
    const uint8_t* row = s.rows + (int64_t)b * s.rowbytes;
    constexpr int EPW = 32 / L, EPB = 8 / L;                        // elements per output word, per byte

    if constexpr (!SG) {                                            // ---- stage the row
        if (((uintptr_t)row & 3u) == 0) {
            const int nw = s.rowbytes >> 2;
            for (int w = tid; w < nw; w += AL_WG) ((uint32_t*)al_lds)[w] = ((const uint32_t*)row)[w];
            for (int j = 4 * nw + tid; j < s.rowbytes; j += AL_WG) al_lds[j] = row[j];
        } else {
            for (int j = tid; j < s.rowbytes; j += AL_WG) al_lds[j] = row[j];
        }
        __syncthreads();
    }

    const int a0 = blockIdx.x * s.chunk;
    const int a1 = a0 + s.chunk < s.A ? a0 + s.chunk : s.A;
    for (int a = a0; a < a1; ++a) {
        const AlignMap m = align_map(s.aligns[3 * a], s.aligns[3 * a + 1], s.aligns[3 * a + 2], s.H, s.W);
        uint8_t* orow = s.out + ((int64_t)b * s.A + a) * s.rowbytes;
        int head = (int)((4u - (uint32_t)((uintptr_t)orow & 3u)) & 3u);   // bytes in front of the row's first 4-byte boundary
        if (head > s.rowbytes) head = s.rowbytes;
        const int nwords = (s.rowbytes - head) >> 2;
        const int edge = s.rowbytes - 4 * nwords;                   // head + tail bytes, at most 6
        for (int w = tid; w < nwords; w += AL_WG) {
            uint32_t acc = 0u;
            if (m.ok) {
                if constexpr (SG) acc = align_gather<L>(row, m, (head + 4 * w) * EPB, EPW, s.H, s.W);
                else acc = align_gather<L>((const uint8_t*)al_lds, m, (head + 4 * w) * EPB, EPW, s.H, s.W);
            }
            *(uint32_t*)(orow + head + 4 * w) = __builtin_bswap32(acc);   // MSB first: the first element lands in the lowest address
        }
        if (tid < edge) {
            const int byte = tid < head ? tid : 4 * nwords + tid;   // (tid - head) bytes past head + 4 nwords
            uint32_t acc = 0u;
            if (m.ok) {
                if constexpr (SG) acc = align_gather<L>(row, m, byte * EPB, EPB, s.H, s.W);
                else acc = align_gather<L>((const uint8_t*)al_lds, m, byte * EPB, EPB, s.H, s.W);
            }
            orow[byte] = (uint8_t)acc;
        }
    }
}

template <int L>
int launch_rows_align(const AlignArgs& s, const AlignPlan& p, hipStream_t st) {
    void (*kernel)(AlignArgs) = p.sg ? gsw_rows_align_kernel<L, true> : gsw_rows_align_kernel<L, false>;
    GSW_HIP(allow_dynamic_lds((const void*)kernel, p.lds));
    hipLaunchKernelGGL(kernel, dim3(p.grid_x, p.grid_y), dim3(AL_WG), p.lds, st, s);
    GSW_HIP(hipGetLastError());
    return GSW_OK;
}

}  // namespace

extern "C" {

int gsw_rows_align(const uint8_t* rows_dev, int B, int C, int H, int W, int l, const int32_t* aligns_dev, int A, uint8_t* out_dev, void* stream) {
    const AlignPlan p = align_decide(rows_dev && aligns_dev && out_dev && ((uintptr_t)aligns_dev & 3u) == 0, B, C, H, W, l, A);
    if (p.status != GSW_OK) return p.status;
    const AlignArgs s{rows_dev, aligns_dev, out_dev, C, H, W, A, p.chunk, p.rowbytes};
    switch (l) {
        case 1: return launch_rows_align<1>(s, p, (hipStream_t)stream);
        case 2: return launch_rows_align<2>(s, p, (hipStream_t)stream);
        default: return launch_rows_align<4>(s, p, (hipStream_t)stream);
    }
}

}  // extern "C"
