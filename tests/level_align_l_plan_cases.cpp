// level_align_l_plan_cases.cpp -- walks a grid of inputs of level_align_l_decide (csrc/gswm_align_soft_l.inc, compiled here without its entry point) and prints
// every input whose status is not the restated one, whose decision breaks an invariant of a launch that no kernel checks, or whose l = 1 decision differs from
// level_align_decide's; then every refusal case whose status or (all-zero) decision is not the expected one.  Host code only: tests/test_align_soft_l_host.py builds
// it with the library's compiler; built with -fsanitize=address,undefined it is the sanitizer run of the policy.
//   level_align_l_plan_cases          stdout: one line per broken input; stderr: "<inputs> inputs, <broken> broken, <classes seen>"
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include <stddef.h>
#include <stdint.h>

#include "gswm.h"
#include "gswm_record.h"   // GSW_ROW_MAX_BITS
#define GSW_LEVEL_ALIGN_PLAN_ONLY
#include "gswm_align_soft.inc"
#include "gswm_align_soft_l.inc"

// the status restated: BAD_ARG, then UNSUPPORTED, then RAGGED (128-bit products: nothing overflows)
static int expected_status(bool ptr, int l, int P, int B, int C, int H, int W, int A) {
    if (!ptr || (l != 1 && l != 2 && l != 4) || P < 1 || P > 4 || B < 1 || C < 1 || H < 1 || W < 1 || A < 1) return GSW_ERR_BAD_ARG;
    const __int128 nb = (__int128)C * H * W * l;
    if (nb * (1 + P) > 1048576 || B > 65535) return GSW_ERR_UNSUPPORTED;
    return nb % 8 ? GSW_ERR_RAGGED : GSW_OK;
}

static std::string broken(int l, int P, int B, int C, int H, int W, int A, const LevelAlignPlan& p) {
    std::string bad;
    auto need = [&](bool ok, const char* name) { if (!ok) bad += std::string(bad.empty() ? "" : ",") + name; };
    const int64_t nb = (int64_t)C * H * W * l;
    need(p.rowbytes * 8ll == nb, "row");                                   // the gather reads bytes below rowbytes of 1 + P rows, the stores end at rowbytes
    need(p.lds <= 65536u, "lds<=65536");
    if (p.sg) {
        need(p.lds == 0 && p.lstride == 0, "sg");
        need((int64_t)(1 + P) * ((p.rowbytes + 15) / 16 * 16) > 65536, "sg_needed");
        need((int64_t)(1 + P) * p.rowbytes <= 131072, "sg_rows<=128KiB");
    } else {
        need(p.lstride % 16 == 0 && p.lstride >= p.rowbytes && p.lstride < p.rowbytes + 16, "lstride");
        need((int64_t)p.lds == (int64_t)(1 + P) * p.lstride, "rows<=lds");
    }
    need(p.chunk >= 1 && p.chunk <= 16, "chunk");
    need(p.grid_x >= 1 && (int64_t)p.grid_x * p.chunk >= A && (int64_t)(p.grid_x - 1) * p.chunk < A, "grid_x");
    need(p.grid_y == B && p.grid_y <= 65535, "grid_y");
    need(p.chunk == 1 || (int64_t)A * B / p.chunk >= 2048, "chunk_keeps_the_grid");
    if (l == 1) {
        const LevelAlignPlan q = level_align_decide(true, P, B, C, H, W, A);
        need(std::memcmp(&p, &q, sizeof p) == 0, "l1_is_level_align_decide");
    }
    return bad;
}

static bool decided_nothing(const LevelAlignPlan& p) {
    return p.sg == 0 && p.chunk == 0 && p.grid_x == 0 && p.grid_y == 0 && p.rowbytes == 0 && p.lstride == 0 && p.lds == 0;
}

int main() {
    const int Bs[] = {0, 1, 2, 3, 17, 300, 4096, 65535, 65536};
    const int As[] = {0, 1, 3, 8, 16, 17, 200, 648, 2047, 2048, 2049, 65535, 1000003, 2147483647};
    const int ls[] = {0, 1, 2, 3, 4, 8};
    long long n = 0, bad = 0;
    std::set<std::string> seen;
    for (int l : ls)
        for (int P = 0; P <= 5; ++P) {
            const int w = (l == 2 || l == 4) ? l : 1, planes = P >= 1 && P <= 4 ? P : 1;
            // lattices: tiny and ragged ones, odd rows, rows of an even number of bytes that is no multiple of 4 (l = 2), both sides of the LDS bound of this
            // (l, P), the top of the domain of this (l, P) and past it
            std::vector<std::vector<int>> shapes = {{1, 1, 1}, {1, 1, 2}, {1, 1, 3}, {1, 1, 4}, {1, 3, 8}, {3, 5, 8}, {1, 8, 8}, {4, 6, 10}, {4, 16, 16}, {4, 32, 32}, {4, 64, 64},
                                                    {4, 128, 128}, {4, 128, 256}, {4, 256, 256}, {2147483647, 2147483647, 2147483647}, {2147483646, 2147483644, 2147483640},
                                                    {0, 8, 8}, {4, -1, 8}};
            const int edge = 65536 / (1 + planes) * 8 / w;                 // elements per row at the LDS bound
            for (int d = -40; d <= 40; d += 4) shapes.push_back({1, 1, edge + d});
            const int top = (int)(GSW_ROW_MAX_BITS / (1 + planes) / w);    // elements per row at the top of the domain
            for (int d = -16; d <= 8; d += 2) shapes.push_back({1, 1, top + d});
            for (const auto& s : shapes)
                for (int B : Bs)
                    for (int A : As) {
                        const LevelAlignPlan p = level_align_l_decide(true, l, P, B, s[0], s[1], s[2], A);
                        ++n;
                        const int want = expected_status(true, l, P, B, s[0], s[1], s[2], A);
                        if (p.status != want || (want != GSW_OK && !decided_nothing(p))) {
                            printf("status\tl=%d\tP=%d\tB=%d\tshape=%d,%d,%d\tA=%d\tstatus=%d\twant=%d\n", l, P, B, s[0], s[1], s[2], A, p.status, want);
                            ++bad;
                            continue;
                        }
                        if (want != GSW_OK) { seen.insert(want == GSW_ERR_BAD_ARG ? "bad_arg" : want == GSW_ERR_RAGGED ? "ragged" : "unsupported"); continue; }
                        seen.insert(std::string(p.sg ? "sg" : "lds") + "@l" + std::to_string(l));
                        seen.insert("chunk" + std::to_string(p.chunk));
                        if (l == 2 && p.rowbytes % 4 == 2) seen.insert("l2_rows_at_phase_2");
                        if (s[0] == 4 && s[1] == 128 && s[2] == 128 && l == 4 && P == 2) seen.insert(p.sg && p.rowbytes * 3 == 98304 ? "4x128x128_l4_p2_sg" : "4x128x128_l4_p2_WRONG");
                        const std::string b = broken(l, P, B, s[0], s[1], s[2], A, p);
                        if (!b.empty()) { printf("%s\tl=%d\tP=%d\tB=%d\tshape=%d,%d,%d\tA=%d\tlds=%u\tchunk=%d\n", b.c_str(), l, P, B, s[0], s[1], s[2], A, p.lds, p.chunk); ++bad; }
                    }
        }
    // ---- every refusal precedes a launch: the status, and a decision of zeros (no grid, no LDS)
    struct Case { const char* name; bool ptr; int l, P, B, C, H, W, A; int status; };
    const Case cases[] = {
        {"pointers", false, 2, 2, 3, 4, 8, 8, 5, GSW_ERR_BAD_ARG},
        {"l_zero", true, 0, 2, 3, 4, 8, 8, 5, GSW_ERR_BAD_ARG},
        {"l_three", true, 3, 2, 3, 4, 8, 8, 5, GSW_ERR_BAD_ARG},
        {"l_eight", true, 8, 2, 3, 4, 8, 8, 5, GSW_ERR_BAD_ARG},
        {"p_zero", true, 2, 0, 3, 4, 8, 8, 5, GSW_ERR_BAD_ARG},
        {"p_five", true, 4, 5, 3, 4, 8, 8, 5, GSW_ERR_BAD_ARG},
        {"b_zero", true, 2, 2, 0, 4, 8, 8, 5, GSW_ERR_BAD_ARG},
        {"c_zero", true, 2, 2, 3, 0, 8, 8, 5, GSW_ERR_BAD_ARG},
        {"h_negative", true, 2, 2, 3, 4, -1, 8, 5, GSW_ERR_BAD_ARG},
        {"w_zero", true, 2, 2, 3, 4, 8, 0, 5, GSW_ERR_BAD_ARG},
        {"a_zero", true, 2, 2, 3, 4, 8, 8, 0, GSW_ERR_BAD_ARG},
        {"ragged_l2", true, 2, 2, 3, 1, 1, 3, 5, GSW_ERR_RAGGED},
        {"ragged_l4", true, 4, 2, 3, 1, 1, 1, 5, GSW_ERR_RAGGED},
        {"ok/whole_byte_l4", true, 4, 2, 3, 1, 1, 2, 5, GSW_OK},
        {"ok/4x128x128_l4_p2", true, 4, 2, 1, 4, 128, 128, 3, GSW_OK},
        {"ok/at_domain_l4_p3", true, 4, 3, 1, 4, 128, 128, 3, GSW_OK},
        {"past_domain_l4_p4", true, 4, 4, 1, 4, 128, 128, 3, GSW_ERR_UNSUPPORTED},
        {"ok/at_domain_l2_p1", true, 2, 1, 3, 4, 256, 256, 5, GSW_OK},
        {"past_domain_l2_p2", true, 2, 2, 3, 4, 256, 256, 5, GSW_ERR_UNSUPPORTED},
        {"huge_product", true, 4, 1, 3, 2147483647, 2147483647, 2147483647, 5, GSW_ERR_UNSUPPORTED},
        {"b_65536", true, 2, 2, 65536, 4, 8, 8, 5, GSW_ERR_UNSUPPORTED},
        {"order/bad_arg_before_ragged", true, 3, 2, 3, 1, 1, 3, 5, GSW_ERR_BAD_ARG},
        {"order/unsupported_before_ragged", true, 2, 2, 65536, 1, 1, 3, 5, GSW_ERR_UNSUPPORTED},
        {"ok/b_65535", true, 2, 2, 65535, 4, 8, 8, 5, GSW_OK},
    };
    for (const Case& c : cases) {
        const LevelAlignPlan p = level_align_l_decide(c.ptr, c.l, c.P, c.B, c.C, c.H, c.W, c.A);
        ++n;
        if (p.status != c.status || (c.status != GSW_OK && !decided_nothing(p)) || (c.status == GSW_OK && !broken(c.l, c.P, c.B, c.C, c.H, c.W, c.A, p).empty())) {
            printf("refusal\t%s\tstatus=%d\n", c.name, p.status);
            ++bad;
        }
    }
    std::string classes;
    for (const auto& s : seen) classes += " " + s;
    fprintf(stderr, "%lld inputs, %lld broken,%s\n", n, bad, classes.c_str());
    return 0;
}
