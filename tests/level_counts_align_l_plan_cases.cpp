// level_counts_align_l_plan_cases.cpp -- walks a grid of inputs of level_counts_align_l_decide (csrc/gswm_counts_align_soft_l_plan.h) and prints every input whose
// decision breaks an invariant of a launch that no kernel checks or, at l = 1, differs from level_counts_align_decide's, then every refusal case whose status or
// (all-zero) decision is not the expected one.  The invariants are those of tests/level_counts_align_plan_cases.cpp with the row of Nb = n l bits in place of n.
// Host code only: tests/test_align_soft_l_host.py builds it with the library's compiler; built with -fsanitize=address,undefined it is the sanitizer run of the policy.
//   level_counts_align_l_plan_cases    stdout: one line per broken input; stderr: "<inputs> inputs, <broken> broken, <classes seen>"
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include <stddef.h>
#include <stdint.h>

#include "gswm.h"
#include "gswm_counts_align_soft_l_plan.h"

static const uint32_t CAP = 131072u;    // the cap restated: 128 KiB, within a CU's 160 KiB

// the LDS bytes restated from the layout: 1 + P rows padded to 16, the keystream in 64-byte blocks, two uint16 per position and counting lane
static __int128 lds_bytes(__int128 n, int P, int M) {                 // n: the bits of a row
    const __int128 rowbytes = n / 8;
    const int words = M % 32 == 0, units = words ? M / 32 : M / 8, lanes = 256 / units * units;
    return (1 + P) * ((rowbytes + 15) / 16 * 16) + 64 * ((rowbytes + 63) / 64) + 2 * (__int128)lanes * (words ? 64 : 16);
}

// the status restated: BAD_ARG, then RAGGED, then UNSUPPORTED (128-bit products: nothing overflows)
static int expected_status(bool ptr, int l, int P, int B, int C, int H, int W, int A, int M, int32_t bias) {
    if (l != 1 && l != 2 && l != 4) return GSW_ERR_BAD_ARG;
    if (!ptr || B < 1 || C < 1 || H < 1 || W < 1 || A < 1 || P < 1 || P > 4) return GSW_ERR_BAD_ARG;
    if (M < 8 || M > 2048 || M % 8) return GSW_ERR_BAD_ARG;
    const __int128 n = (__int128)C * H * W * l;
    if (n % 8 != 0 || n % M != 0) return GSW_ERR_RAGGED;
    if (n * (1 + P) > 1048576 || B > 65535) return GSW_ERR_UNSUPPORTED;
    if (lds_bytes(n, P, M) > CAP) return GSW_ERR_UNSUPPORTED;
    const __int128 mag = bias < 0 ? -(__int128)bias : (__int128)bias;
    if (mag + 15 * (n / M) > 2147483647) return GSW_ERR_UNSUPPORTED;
    return GSW_OK;
}

static std::string broken(int l, int P, int B, int C, int H, int W, int A, int M, int32_t bias, const LevelCountsAlignPlan& p) {
    std::string bad;
    auto need = [&](bool ok, const char* name) { if (!ok) bad += std::string(bad.empty() ? "" : ",") + name; };
    const int64_t n = (int64_t)C * H * W * l;                           // the bits of a row
    need(p.rowbytes * 8ll == n && p.copies * (int64_t)M == n, "row");
    need(p.nblk * 64 >= p.rowbytes && (p.nblk - 1) * 64 < p.rowbytes, "nblk");
    // LDS: [1 + P rows | keystream | X' | N'], disjoint, 16-byte aligned, within the cap and within a CU's 160 KiB
    need(p.lstride % 16 == 0 && p.lstride >= p.rowbytes && p.lstride < p.rowbytes + 16, "lstride");
    need(p.off_ks % 16 == 0 && p.off_ks >= (uint32_t)(1 + P) * (uint32_t)p.lstride, "row_region");
    need(p.off_red % 16 == 0 && p.off_red >= p.off_ks + 64u * (uint32_t)p.nblk, "ks_region");
    const uint32_t lane_bytes = p.words ? 64u : 16u;                    // 32 or 8 uint16 per lane and kind
    need(p.off_red_n % 16 == 0 && p.off_red_n >= p.off_red + (uint32_t)p.lanes * lane_bytes, "x_region");
    need(p.lds >= p.off_red_n + (uint32_t)p.lanes * lane_bytes && p.lds <= LCA_LDS_CAP && LCA_LDS_CAP <= CAP && p.lds <= 160u * 1024u, "lds");
    need((__int128)p.lds == lds_bytes(n, P, M), "lds_restated");
    // the lanes: a multiple of the message units, so that a lane's unit never changes; a column of the reduction region holds groups x M uint16
    need(p.words == (M % 32 == 0) && p.units == (p.words ? M / 32 : M / 8), "units");
    need(p.lanes >= 1 && p.lanes <= LCA_WG && p.lanes % p.units == 0 && p.lanes + p.units > LCA_WG && p.groups * p.units == p.lanes, "lanes");
    need((int64_t)p.groups * M * 2 == (int64_t)p.lanes * lane_bytes, "red_read");
    // the widths: a lane's largest count fits its live counter planes, 15 times it fits the uint16 it leaves in LDS (and half a dword in registers), the column
    // sums reach at most 15 V, which with the bias fits the int32 that is stored
    const int64_t row_units = p.words ? n / 32 : n / 8;
    need((int64_t)p.lane_max * p.lanes >= row_units && (int64_t)(p.lane_max - 1) * p.lanes < row_units, "lane_max");
    need(p.words ? (p.cplanes >= 1 && p.cplanes <= LCA_PLANES && p.lane_max < (1 << p.cplanes) && p.lane_max >= (1 << (p.cplanes - 1))) : p.cplanes == 0, "cplanes");
    need(p.lane_max <= (p.words ? 127 : 4369), "counter_width");
    need(15ll * p.lane_max <= 65535, "lds_width");
    need((int64_t)p.lane_max * p.groups >= p.copies, "copies");
    need((bias < 0 ? -(int64_t)bias : (int64_t)bias) + 15ll * p.copies <= 2147483647ll, "int32");
    // the grid covers every (image, alignment) exactly once
    need(p.chunk >= 1 && p.chunk <= 16, "chunk");
    need(p.grid_x >= 1 && (int64_t)p.grid_x * p.chunk >= A && (int64_t)(p.grid_x - 1) * p.chunk < A, "grid_x");
    need(p.grid_y == B && p.grid_y <= 65535, "grid_y");
    need(p.chunk == 1 || (int64_t)A * B / p.chunk >= 2048, "chunk_keeps_the_grid");
    if (l == 1) {
        const LevelCountsAlignPlan q = level_counts_align_decide(true, P, B, C, H, W, A, M, bias);
        need(std::memcmp(&p, &q, sizeof p) == 0, "l1_is_level_counts_align_decide");
    }
    return bad;
}

static bool decided_nothing(const LevelCountsAlignPlan& p) {
    return !p.words && !p.chunk && !p.grid_x && !p.grid_y && !p.rowbytes && !p.lstride && !p.nblk && !p.units && !p.lanes && !p.groups && !p.lane_max && !p.cplanes &&
           !p.copies && !p.off_ks && !p.off_red && !p.off_red_n && !p.lds;
}

int main() {
    const int ls[] = {0, 1, 2, 3, 4};
    const int Bs[] = {0, 1, 3, 70, 4096, 65535, 65536};
    const int As[] = {0, 1, 8, 17, 648, 2048, 2049, 65535, 2147483647};
    const int Ms[] = {0, 4, 8, 12, 16, 24, 32, 40, 64, 96, 200, 256, 264, 1024, 2048, 2056};
    const int Ps[] = {0, 1, 2, 3, 4, 5};
    const int32_t biases[] = {0, 61440, -7, 2147483647, (int32_t)(-2147483647 - 1), 2147483647 - 15 * 64, 2147483647 - 15 * 64 + 1};
    std::vector<std::vector<int>> shapes = {{1, 8, 8}, {3, 5, 8}, {4, 5, 8}, {4, 16, 16}, {2, 6, 6}, {8, 17, 25}, {4, 64, 64}, {4, 128, 128}, {1, 3, 3}, {1, 1, 2}, {1, 1, 3},
                                            {4, 32, 32}, {4, 256, 256}, {4, 128, 132}, {4, 128, 256}, {4, 64, 128}, {4, 128, 66}, {1, 8, 65536}, {1, 1, 524288}, {1, 1, 131072},
                                            {1, 1, 209712}, {1, 1, 104860}, {1, 1, 52430}, {2147483647, 2147483647, 2147483647}, {0, 8, 8}, {4, -1, 8}};
    long long n = 0, bad = 0;
    std::set<std::string> seen;
    for (int l : ls)
    for (const auto& s : shapes)
        for (int P : Ps)
            for (int M : Ms)
                for (int32_t bias : biases)
                    for (int B : Bs)
                        for (int A : As) {
                            const LevelCountsAlignPlan p = level_counts_align_l_decide(true, l, P, B, s[0], s[1], s[2], A, M, bias);
                            ++n;
                            const int want = expected_status(true, l, P, B, s[0], s[1], s[2], A, M, bias);
                            if (p.status != want || (want != GSW_OK && !decided_nothing(p))) {
                                printf("status\tl=%d\tP=%d\tB=%d\tshape=%d,%d,%d\tA=%d\tM=%d\tbias=%d\tstatus=%d\twant=%d\n", l, P, B, s[0], s[1], s[2], A, M, (int)bias, p.status, want);
                                ++bad;
                                continue;
                            }
                            if (want != GSW_OK) { seen.insert(want == GSW_ERR_BAD_ARG ? "bad_arg" : want == GSW_ERR_RAGGED ? "ragged" : "unsupported"); continue; }
                            seen.insert(std::string(p.words ? "words" : "bytes") + "@l" + std::to_string(l));
                            seen.insert("chunk" + std::to_string(p.chunk));
                            if (p.words) seen.insert("cplanes" + std::to_string(p.cplanes));
                            if (p.lds == LCA_LDS_CAP) seen.insert("lds_at_cap");
                            if (p.lanes < LCA_WG) seen.insert("idle_lanes");
                            if (s[0] == 4 && s[1] == 64 && s[2] == 64 && l == 4 && P == 4 && M == 256) seen.insert(p.lds == 80u * 1024u ? "4x64x64_l4_p4_80KiB" : "4x64x64_l4_p4_WRONG");
                            const std::string b = broken(l, P, B, s[0], s[1], s[2], A, M, bias, p);
                            if (!b.empty()) { printf("%s\tl=%d\tP=%d\tB=%d\tshape=%d,%d,%d\tA=%d\tM=%d\tbias=%d\tlds=%u\tchunk=%d\n", b.c_str(), l, P, B, s[0], s[1], s[2], A, M, (int)bias, p.lds, p.chunk); ++bad; }
                        }
    // ---- every refusal precedes a launch, in the stated order when an input breaks several
    struct Case { const char* name; bool ptr; int l, P, B, C, H, W, A, M; int32_t bias; int status; };
    const Case cases[] = {
        {"pointers", false, 2, 4, 3, 4, 8, 8, 5, 64, 0, GSW_ERR_BAD_ARG},
        {"l_zero", true, 0, 4, 3, 4, 8, 8, 5, 64, 0, GSW_ERR_BAD_ARG},
        {"l_three", true, 3, 4, 3, 4, 8, 8, 5, 64, 0, GSW_ERR_BAD_ARG},
        {"b_zero", true, 2, 4, 0, 4, 8, 8, 5, 64, 0, GSW_ERR_BAD_ARG},
        {"w_zero", true, 4, 4, 3, 4, 8, 0, 5, 64, 0, GSW_ERR_BAD_ARG},
        {"a_zero", true, 4, 4, 3, 4, 8, 8, 0, 64, 0, GSW_ERR_BAD_ARG},
        {"p_five", true, 2, 5, 3, 4, 8, 8, 5, 64, 0, GSW_ERR_BAD_ARG},
        {"m_twelve", true, 2, 4, 3, 4, 8, 8, 5, 12, 0, GSW_ERR_BAD_ARG},
        {"m_2056", true, 4, 4, 3, 4, 64, 64, 5, 2056, 0, GSW_ERR_BAD_ARG},
        {"ragged_bytes_l2", true, 2, 4, 3, 1, 1, 3, 5, 8, 0, GSW_ERR_RAGGED},
        {"ragged_message_l2", true, 2, 4, 3, 4, 8, 8, 5, 24, 0, GSW_ERR_RAGGED},
        {"ok/message_tiles_at_l4_only", true, 4, 4, 3, 4, 5, 8, 5, 40, 0, GSW_OK},            // 640 cipher bits: 16 copies of 40 on the byte path
        {"ragged_message_l2_128", true, 2, 4, 3, 4, 5, 8, 5, 128, 0, GSW_ERR_RAGGED},         // 320 cipher bits at l = 2 ...
        {"ok/message_l4_128", true, 4, 4, 3, 4, 5, 8, 5, 128, 0, GSW_OK},                      // ... 640 at l = 4
        {"past_domain_l4", true, 4, 4, 3, 4, 128, 128, 5, 256, 0, GSW_ERR_UNSUPPORTED},
        {"past_domain_l2", true, 2, 2, 3, 4, 256, 256, 5, 256, 0, GSW_ERR_UNSUPPORTED},
        {"past_lds_cap_l4", true, 4, 1, 3, 4, 128, 132, 5, 256, 0, GSW_ERR_UNSUPPORTED},
        {"ok/at_lds_cap_l4_p1", true, 4, 1, 3, 4, 128, 128, 5, 256, 0, GSW_OK},                // a row of 524 288 bits: 128 KiB exactly
        {"ok/at_lds_cap_l2_p4", true, 2, 4, 3, 4, 128, 128, 5, 256, 0, GSW_OK},                // a row of 131 072 bits at P = 4: the cap exactly
        {"ok/4x64x64_l4_p4", true, 4, 4, 3, 4, 64, 64, 5, 256, 15 * 256, GSW_OK},
        {"huge_product", true, 4, 4, 3, 2147483647, 2147483647, 2147483647, 5, 8, 0, GSW_ERR_RAGGED},
        {"huge_even_product", true, 2, 4, 3, 2147483646, 2147483644, 2147483640, 5, 8, 0, GSW_ERR_UNSUPPORTED},
        {"b_65536", true, 2, 4, 65536, 4, 8, 8, 5, 64, 0, GSW_ERR_UNSUPPORTED},
        {"bias_past_int32_l4", true, 4, 4, 3, 4, 32, 32, 5, 64, 2147483647 - 15 * 256 + 1, GSW_ERR_UNSUPPORTED},
        {"ok/bias_at_int32_l4", true, 4, 4, 3, 4, 32, 32, 5, 64, 2147483647 - 15 * 256, GSW_OK},
        {"bias_int32_min", true, 2, 4, 3, 4, 32, 32, 5, 64, (int32_t)(-2147483647 - 1), GSW_ERR_UNSUPPORTED},
        {"order/bad_l_before_ragged", true, 3, 4, 3, 1, 1, 3, 5, 8, 0, GSW_ERR_BAD_ARG},
        {"order/bad_message_before_ragged", true, 2, 4, 3, 1, 1, 3, 5, 12, 0, GSW_ERR_BAD_ARG},
        {"order/ragged_before_unsupported", true, 4, 4, 65536, 4, 512, 512, 5, 24, 0, GSW_ERR_RAGGED},
        {"ok/longest_message_l2", true, 2, 4, 3, 4, 64, 64, 8, 2048, 0, GSW_OK},
    };
    for (const Case& c : cases) {
        const LevelCountsAlignPlan p = level_counts_align_l_decide(c.ptr, c.l, c.P, c.B, c.C, c.H, c.W, c.A, c.M, c.bias);
        ++n;
        if (p.status != c.status || (c.status != GSW_OK && !decided_nothing(p)) ||
            (c.status == GSW_OK && !broken(c.l, c.P, c.B, c.C, c.H, c.W, c.A, c.M, c.bias, p).empty())) {
            printf("refusal\t%s\tstatus=%d\n", c.name, p.status);
            ++bad;
        }
    }
    std::string classes;
    for (const auto& s : seen) classes += " " + s;
    fprintf(stderr, "%lld inputs, %lld broken,%s\n", n, bad, classes.c_str());
    return 0;
}
