// gswm_counts_align_soft_l.inc -- the level-weighted vote of every candidate alignment of gsw_level_pack_l's rows (l = 2, 4) under ONE key, in one launch
// (gfx950): the operand of a registry search over (record, alignment) pairs ranked by reliability levels at l > 1.  Included at the end of gswm_keyed.hip
// after gswm_counts_align_soft.inc: the kernel, LevelCountsAlignArgs and launch_level_counts_align<L, P> are that file's; the policy is
// level_counts_align_l_decide (gswm_counts_align_soft_l_plan.h).
//
//   score[b, a, t] = bias + sum over p = t (mod M) of level_p (2 d_p - 1)          p over the n l cipher positions of the image
//   wsum [b, a, t] =        sum over p = t (mod M) of level_p                      (optional: a null pointer skips it)
//
// d_p = (bit p of gsw_rows_align's row (b, a) of the quantised row at that l) ^ (keystream bit p), level_p = sum_k 2^k (bit p of the aligned plane k):
// gsw_extract_soft_l's score and wsum of the aligned image under the table the rows were packed with.
//
// gsw_level_counts_align_kernel<L, P, WORDS> gathers the L-bit group of an element from all 1 + P rows after one index walk; once a lane holds the aligned
// 32-bit words (or bytes) of the rows the counting is that of l = 1: the vertical counters on the word path, the int32 accumulators on the byte path and the
// reduction region do not know how many bits an element owns.  Only the gather and the row length (n l) differ.

namespace {

template <int L>
int launch_level_counts_align_l(int P, const LevelCountsAlignArgs& s, const LevelCountsAlignPlan& p, hipStream_t st) {
    switch (P) {
        case 1: return launch_level_counts_align<L, 1>(s, p, st);
        case 2: return launch_level_counts_align<L, 2>(s, p, st);
        case 3: return launch_level_counts_align<L, 3>(s, p, st);
        default: return launch_level_counts_align<L, 4>(s, p, st);
    }
}

}  // namespace

extern "C" {

int gsw_level_counts_align_l(const uint8_t* signs_dev, const uint8_t* planes_dev, int P, int l, int B, int C, int H, int W, const int32_t* aligns_dev, int A,
                             const uint8_t key[32], const uint8_t nonce16[16], int msg_bits, int bias, int32_t* score_dev, int32_t* wsum_dev, void* stream) {
    const bool pointers_ok = signs_dev && planes_dev && aligns_dev && key && nonce16 && score_dev && ((uintptr_t)aligns_dev & 3u) == 0 &&
                             ((uintptr_t)score_dev & 3u) == 0 && ((uintptr_t)wsum_dev & 3u) == 0;
    const LevelCountsAlignPlan p = level_counts_align_l_decide(pointers_ok, l, P, B, C, H, W, A, msg_bits, bias);
    if (p.status != GSW_OK) return p.status;
    const auto le = [](const uint8_t* q) { return (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24); };
    const LevelCountsAlignArgs s{signs_dev, planes_dev, aligns_dev, score_dev, wsum_dev,
                                 le(key), le(key + 4), le(key + 8), le(key + 12), le(key + 16), le(key + 20), le(key + 24), le(key + 28),
                                 le(nonce16), le(nonce16 + 4), le(nonce16 + 8), le(nonce16 + 12),
                                 C, H, W, A, p.chunk, p.rowbytes, p.lstride, p.nblk, msg_bits, p.lanes, p.groups, p.cplanes, bias,
                                 p.off_ks, p.off_red, p.off_red_n};
    switch (l) {
        case 1: return launch_level_counts_align_l<1>(P, s, p, (hipStream_t)stream);
        case 2: return launch_level_counts_align_l<2>(P, s, p, (hipStream_t)stream);
        default: return launch_level_counts_align_l<4>(P, s, p, (hipStream_t)stream);
    }
}

}  // extern "C"
