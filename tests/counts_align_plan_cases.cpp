// counts_align_plan_cases.cpp -- walks a grid of inputs of counts_align_decide (csrc/gswm_counts_align_plan.h) and prints every input whose decision breaks an
// invariant of a launch that no kernel checks, then every refusal case whose status or (all-zero) decision is not the expected one.  Host code only:
// tests/test_trace_align_host.py builds it with the library's compiler; built with -fsanitize=address,undefined it is the sanitizer run of the policy.
//   counts_align_plan_cases            stdout: one line per broken input; stderr: "<inputs> inputs, <broken> broken, <classes seen>"
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include <stddef.h>
#include <stdint.h>

#include "gswm.h"
#include "gswm_counts_align_plan.h"

// the status restated: BAD_ARG, then RAGGED, then UNSUPPORTED (128-bit products: nothing overflows)
static int expected_status(bool ptr, int B, int C, int H, int W, int l, int A, int M) {
    if (!ptr || B < 1 || C < 1 || H < 1 || W < 1 || A < 1 || (l != 1 && l != 2 && l != 4)) return GSW_ERR_BAD_ARG;
    if (M < 8 || M > 2048 || M % 8) return GSW_ERR_BAD_ARG;
    const __int128 n = (__int128)C * H * W * l;
    if (n % 8 != 0 || n % M != 0) return GSW_ERR_RAGGED;
    if (n > 524288 || B > 65535) return GSW_ERR_UNSUPPORTED;
    return GSW_OK;
}

static std::string broken(int B, int C, int H, int W, int l, int A, int M, const CountsAlignPlan& p) {
    std::string bad;
    auto need = [&](bool ok, const char* name) { if (!ok) bad += std::string(bad.empty() ? "" : ",") + name; };
    const int64_t n = (int64_t)C * H * W * l;
    need(p.rowbytes * 8ll == n && p.copies * (int64_t)M == n, "row");
    need(p.nblk * 64 >= p.rowbytes && (p.nblk - 1) * 64 < p.rowbytes, "nblk");
    // LDS: [row | keystream | reduction], disjoint, 16-byte aligned, within the cap and within a CU's 160 KiB
    need(p.off_ks % 16 == 0 && p.off_ks >= (uint32_t)p.rowbytes, "row_region");
    need(p.off_red % 16 == 0 && p.off_red >= p.off_ks + 64u * (uint32_t)p.nblk, "ks_region");
    need(p.lds == p.off_red + CA_RED_BYTES && p.lds <= CA_LDS_CAP && p.lds <= 160u * 1024u, "lds");
    // the lanes: a multiple of the message units, so that a lane's unit never changes; the reduction region holds every lane's counters
    need(p.words == (M % 32 == 0) && p.units == (p.words ? M / 32 : M / 8), "units");
    need(p.lanes >= 1 && p.lanes <= CA_WG && p.lanes % p.units == 0 && p.lanes + p.units > CA_WG && p.groups * p.units == p.lanes, "lanes");
    need((uint32_t)p.lanes * (p.words ? 32u : 16u) <= CA_RED_BYTES, "red_region");
    need((int64_t)p.groups * M * (p.words ? 1 : 2) <= (int64_t)CA_RED_BYTES, "red_read");
    // the counters: a lane's largest count fits its width, the groups together reach V, which fits the int32 that is stored
    const int64_t row_units = p.words ? n / 32 : n / 8;
    need((int64_t)p.lane_max * p.lanes >= row_units && (int64_t)(p.lane_max - 1) * p.lanes < row_units, "lane_max");
    need(p.lane_max <= (p.words ? (1 << CA_PLANES) - 1 : 65535), "counter_width");
    need(p.words ? p.lane_max <= 255 : p.lane_max <= 65535, "lds_width");
    need((int64_t)p.lane_max * p.groups >= p.copies && p.copies <= 2147483647ll, "copies");
    // the grid covers every (image, alignment) exactly once
    need(p.chunk >= 1 && p.chunk <= 16, "chunk");
    need(p.grid_x >= 1 && (int64_t)p.grid_x * p.chunk >= A && (int64_t)(p.grid_x - 1) * p.chunk < A, "grid_x");
    need(p.grid_y == B && p.grid_y <= 65535, "grid_y");
    need(p.chunk == 1 || (int64_t)A * B / p.chunk >= 2048, "chunk_keeps_the_grid");
    return bad;
}

static bool decided_nothing(const CountsAlignPlan& p) {
    return !p.words && !p.chunk && !p.grid_x && !p.grid_y && !p.rowbytes && !p.nblk && !p.units && !p.lanes && !p.groups && !p.lane_max && !p.copies && !p.off_ks &&
           !p.off_red && !p.lds;
}

int main() {
    const int Bs[] = {0, 1, 2, 3, 17, 70, 300, 4096, 65535, 65536};
    const int As[] = {0, 1, 3, 8, 12, 16, 17, 120, 200, 648, 2047, 2048, 2049, 65535, 1000003, 2147483647};
    const int Ms[] = {0, 4, 8, 12, 16, 24, 32, 40, 64, 96, 128, 200, 256, 264, 1024, 2040, 2048, 2056};
    const int ls[] = {1, 2, 3, 4};
    std::vector<std::vector<int>> shapes = {{1, 8, 8}, {3, 5, 8}, {4, 16, 16}, {2, 6, 6}, {4, 17, 25}, {4, 12, 12}, {4, 64, 64}, {4, 128, 128}, {1, 3, 3}, {1, 1, 8},
                                            {4, 32, 32}, {4, 256, 512}, {4, 256, 513}, {4, 512, 512}, {1, 8, 65536}, {1, 8, 65537}, {1, 1, 524288}, {1, 1, 524296},
                                            {1, 255, 2056}, {2147483647, 2147483647, 2147483647}, {0, 8, 8}, {4, -1, 8}};
    long long n = 0, bad = 0;
    std::set<std::string> seen;
    for (const auto& s : shapes)
        for (int l : ls)
            for (int M : Ms)
                for (int B : Bs)
                    for (int A : As) {
                        const CountsAlignPlan p = counts_align_decide(true, B, s[0], s[1], s[2], l, A, M);
                        ++n;
                        const int want = expected_status(true, B, s[0], s[1], s[2], l, A, M);
                        if (p.status != want || (want != GSW_OK && !decided_nothing(p))) {
                            printf("status\tB=%d\tshape=%d,%d,%d\tl=%d\tA=%d\tM=%d\tstatus=%d\twant=%d\n", B, s[0], s[1], s[2], l, A, M, p.status, want);
                            ++bad;
                            continue;
                        }
                        if (want != GSW_OK) { seen.insert(want == GSW_ERR_BAD_ARG ? "bad_arg" : want == GSW_ERR_RAGGED ? "ragged" : "unsupported"); continue; }
                        seen.insert(p.words ? "words" : "bytes");
                        seen.insert("chunk" + std::to_string(p.chunk));
                        if (p.lds > 128u * 1024u) seen.insert("lds>128K");
                        if (p.lanes < CA_WG) seen.insert("idle_lanes");
                        const std::string b = broken(B, s[0], s[1], s[2], l, A, M, p);
                        if (!b.empty()) { printf("%s\tB=%d\tshape=%d,%d,%d\tl=%d\tA=%d\tM=%d\tlds=%u\tchunk=%d\n", b.c_str(), B, s[0], s[1], s[2], l, A, M, p.lds, p.chunk); ++bad; }
                    }
    // ---- every refusal precedes a launch, in the stated order when an input breaks several
    struct Case { const char* name; bool ptr; int B, C, H, W, l, A, M; int status; };
    const Case cases[] = {
        {"pointers", false, 3, 4, 8, 8, 1, 5, 64, GSW_ERR_BAD_ARG},
        {"b_zero", true, 0, 4, 8, 8, 1, 5, 64, GSW_ERR_BAD_ARG},
        {"c_zero", true, 3, 0, 8, 8, 1, 5, 64, GSW_ERR_BAD_ARG},
        {"h_negative", true, 3, 4, -1, 8, 1, 5, 64, GSW_ERR_BAD_ARG},
        {"w_zero", true, 3, 4, 8, 0, 1, 5, 64, GSW_ERR_BAD_ARG},
        {"a_zero", true, 3, 4, 8, 8, 1, 0, 64, GSW_ERR_BAD_ARG},
        {"l_three", true, 3, 4, 8, 8, 3, 5, 64, GSW_ERR_BAD_ARG},
        {"m_zero", true, 3, 4, 8, 8, 1, 5, 0, GSW_ERR_BAD_ARG},
        {"m_twelve", true, 3, 4, 8, 8, 1, 5, 12, GSW_ERR_BAD_ARG},
        {"m_2056", true, 3, 4, 64, 64, 1, 5, 2056, GSW_ERR_BAD_ARG},
        {"ragged_bytes", true, 3, 1, 3, 3, 1, 5, 8, GSW_ERR_RAGGED},
        {"ragged_message", true, 3, 4, 8, 8, 1, 5, 24, GSW_ERR_RAGGED},
        {"past_domain", true, 3, 4, 512, 512, 1, 5, 256, GSW_ERR_UNSUPPORTED},
        {"one_past_domain", true, 3, 1, 1, 524296, 1, 5, 8, GSW_ERR_UNSUPPORTED},
        {"huge_product", true, 3, 2147483647, 2147483647, 2147483647, 1, 5, 8, GSW_ERR_RAGGED},
        {"huge_even_product", true, 3, 2147483646, 2147483644, 2147483640, 4, 5, 8, GSW_ERR_UNSUPPORTED},
        {"b_65536", true, 65536, 4, 8, 8, 1, 5, 64, GSW_ERR_UNSUPPORTED},
        {"order/bad_arg_before_ragged", true, 3, 1, 3, 3, 3, 5, 8, GSW_ERR_BAD_ARG},
        {"order/bad_message_before_ragged", true, 3, 1, 3, 3, 1, 5, 12, GSW_ERR_BAD_ARG},
        {"order/ragged_before_unsupported", true, 65536, 4, 512, 512, 1, 5, 24, GSW_ERR_RAGGED},
        {"ok/at_domain", true, 3, 4, 256, 512, 1, 5, 256, GSW_OK},
        {"ok/b_65535", true, 65535, 4, 8, 8, 1, 5, 64, GSW_OK},
        {"ok/v_2048", true, 2, 4, 64, 64, 1, 8, 8, GSW_OK},
        {"ok/longest_message", true, 3, 4, 64, 64, 4, 8, 2048, GSW_OK},
    };
    for (const Case& c : cases) {
        const CountsAlignPlan p = counts_align_decide(c.ptr, c.B, c.C, c.H, c.W, c.l, c.A, c.M);
        ++n;
        if (p.status != c.status || (c.status != GSW_OK && !decided_nothing(p)) || (c.status == GSW_OK && !broken(c.B, c.C, c.H, c.W, c.l, c.A, c.M, p).empty())) {
            printf("refusal\t%s\tstatus=%d\n", c.name, p.status);
            ++bad;
        }
    }
    std::string classes;
    for (const auto& s : seen) classes += " " + s;
    fprintf(stderr, "%lld inputs, %lld broken,%s\n", n, bad, classes.c_str());
    return 0;
}
