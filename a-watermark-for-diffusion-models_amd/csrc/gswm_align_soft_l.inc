// gswm_align_soft_l.inc -- every candidate alignment of gsw_level_pack_l's rows in one launch (gfx950): the n l-bit row of a multi-bit window (l = 2, 4) AND
// its P level planes, the input of an alignment search ranked by reliability levels at l > 1.
// Included in gswm_keyed.hip after gswm_align_soft.inc: the kernel, LevelAlignPlan, LevelAlignArgs and launch_level_rows_align<L, P> are that file's.
// With GSW_LEVEL_ALIGN_PLAN_ONLY defined only the launch policy below is compiled (tests/level_align_l_plan_cases.cpp sweeps it without a GPU).
//
//   signs      : [B, n l / 8], planes : [B, P, n l / 8] as gsw_level_pack_l writes them; n = C H W, element e owns bits [e l, e l + l) of every row, MSB first
//   out_signs  : [B, A, n l / 8], out_planes : [B, A, P, n l / 8]: row (b, a) of each is bit for bit gsw_rows_align's row at that l
//
// A level plane at l > 1 is a packed row of l-bit groups like the quantised row itself: an alignment moves the l level bits of an element with its l window
// bits.  gsw_level_rows_align_kernel<L, P, SG> computes the source ELEMENT of an output element once (level_align_gather's incremental walk) and gathers its
// L-bit group from all 1 + P rows: a word of the output is 32 / L elements, so the walk is 1 / L as long per byte as at l = 1.  Staging, the SG fallback, head
// and tail bytes and the word stores at any output phase are the l = 1 kernel's; only the row length (n l / 8 bytes) differs.
//
// level_align_l_decide is level_align_decide with n l bits per row: the domain is n l (1 + P) <= GSW_ROW_MAX_BITS, the soft searches' at n_bits = n l.
// l = 1 decides what level_align_decide decides and launches the same kernel.

namespace {

// the launch decision: pure, host only.  A refusal has its status and zeros everywhere else.
inline LevelAlignPlan level_align_l_decide(bool pointers_ok, int l, int P, int B, int C, int H, int W, int A) {
    LevelAlignPlan p{};
    p.status = GSW_ERR_BAD_ARG;
    if (!pointers_ok || (l != 1 && l != 2 && l != 4) || P < 1 || P > 4 || B < 1 || C < 1 || H < 1 || W < 1 || A < 1) return p;
    const int64_t ch = (int64_t)C * H;        // (C, H, W < 2^31 each: no product overflows before it is compared)
    p.status = GSW_ERR_UNSUPPORTED;
    if (ch > GSW_ROW_MAX_BITS || ch * W * l * (1 + P) > GSW_ROW_MAX_BITS || B > 65535) return p;     // (B: the grid's second dimension)
    const int64_t n_bits = ch * W * l;
    if (n_bits % 8 != 0) { p.status = GSW_ERR_RAGGED; return p; }
    p.rowbytes = (int)(n_bits / 8);
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

template <int L>
int launch_level_rows_align_l(int P, const LevelAlignArgs& s, const LevelAlignPlan& p, hipStream_t st) {
    switch (P) {
        case 1: return launch_level_rows_align<L, 1>(s, p, st);
        case 2: return launch_level_rows_align<L, 2>(s, p, st);
        case 3: return launch_level_rows_align<L, 3>(s, p, st);
        default: return launch_level_rows_align<L, 4>(s, p, st);
    }
}

}  // namespace

extern "C" {

int gsw_level_rows_align_l(const uint8_t* signs_dev, const uint8_t* planes_dev, int P, int l, int B, int C, int H, int W, const int32_t* aligns_dev, int A,
                           uint8_t* out_signs_dev, uint8_t* out_planes_dev, void* stream) {
    const bool pointers_ok = signs_dev && planes_dev && aligns_dev && out_signs_dev && out_planes_dev && ((uintptr_t)aligns_dev & 3u) == 0;
    const LevelAlignPlan p = level_align_l_decide(pointers_ok, l, P, B, C, H, W, A);
    if (p.status != GSW_OK) return p.status;
    const LevelAlignArgs s{signs_dev, planes_dev, aligns_dev, out_signs_dev, out_planes_dev, C, H, W, A, p.chunk, p.rowbytes, p.lstride};
    switch (l) {
        case 1: return launch_level_rows_align_l<1>(P, s, p, (hipStream_t)stream);
        case 2: return launch_level_rows_align_l<2>(P, s, p, (hipStream_t)stream);
        default: return launch_level_rows_align_l<4>(P, s, p, (hipStream_t)stream);
    }
}

}  // extern "C"

#endif  // GSW_LEVEL_ALIGN_PLAN_ONLY
