// level_align_plan_cases.cpp -- walks a grid of inputs of level_align_decide (csrc/gswm_align_soft.inc, compiled here without its kernel) and prints every
// input whose decision breaks an invariant of a launch that no kernel checks, then every refusal case whose status or (all-zero) decision is not the expected
// one.  Host code only: tests/test_level_align_plan_host.py builds it with the library's compiler; built with -fsanitize=address,undefined it is the sanitizer
// run of the policy.
//   level_align_plan_cases            stdout: one line per broken input; stderr: "<inputs> inputs, <broken> broken, <classes seen>"
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include <stddef.h>
#include <stdint.h>

#include "gswm.h"
#include "gswm_record.h"   // GSW_ROW_MAX_BITS
#define GSW_LEVEL_ALIGN_PLAN_ONLY
#include "gswm_align_soft.inc"

static std::string broken(int P, int B, int C, int H, int W, int A, const LevelAlignPlan& p) {
    std::string bad;
    auto need = [&](bool ok, const char* name) { if (!ok) bad += std::string(bad.empty() ? "" : ",") + name; };
    const int64_t n = (int64_t)C * H * W;
    need(p.rowbytes * 8ll == n, "row");
    need(p.lds <= 65536u, "lds<=65536");
    if (p.sg) {
        need(p.lds == 0 && p.lstride == 0, "sg");
        need((int64_t)(1 + P) * ((p.rowbytes + 15) / 16 * 16) > 65536, "sg_needed");
    } else {
        need(p.lstride % 16 == 0 && p.lstride >= p.rowbytes && p.lstride < p.rowbytes + 16, "lstride");
        need((int64_t)p.lds == (int64_t)(1 + P) * p.lstride, "rows<=lds");
    }
    need(p.chunk >= 1 && p.chunk <= 16, "chunk");
    need(p.grid_x >= 1 && (int64_t)p.grid_x * p.chunk >= A && (int64_t)(p.grid_x - 1) * p.chunk < A, "grid_x");
    need(p.grid_y == B && p.grid_y <= 65535, "grid_y");
    need(p.chunk == 1 || (int64_t)A * B / p.chunk >= 2048, "chunk_keeps_the_grid");
    return bad;
}

int main() {
    const int Bs[] = {1, 2, 3, 17, 34, 300, 4096, 65535};
    const int As[] = {1, 2, 3, 8, 15, 16, 17, 72, 120, 200, 648, 2047, 2048, 2049, 65535, 1000003, 2147483647};
    long long n = 0, bad = 0;
    bool seen_sg[2] = {false, false};
    std::set<int> chunks;
    for (int P = 1; P <= 4; ++P) {
        // lattices: tiny ones, odd rows, both sides of the LDS bound of this P (padded and not), the top of the domain of this P and one past it
        std::vector<std::vector<int>> shapes = {{1, 2, 4}, {3, 5, 8}, {1, 8, 9}, {4, 8, 8}, {4, 32, 32}, {4, 64, 64}, {1, 1, 8}, {1, 8, 1}, {8, 1, 1}};
        const int edge = 65536 / (1 + P);                                  // bytes per row at the bound
        for (int d = -33; d <= 33; ++d) shapes.push_back({1, 8, edge + d});
        const int top = (int)(GSW_ROW_MAX_BITS / (1 + P) / 8);             // bytes per row at the top of the domain
        for (int d = -2; d <= 0; ++d) shapes.push_back({1, 8, top + d});
        shapes.push_back({4, 256, 1048576 / (1 + P) / 1024});
        for (const auto& s : shapes)
            for (int B : Bs)
                for (int A : As) {
                    const LevelAlignPlan p = level_align_decide(true, P, B, s[0], s[1], s[2], A);
                    ++n;
                    if (p.status != GSW_OK) { printf("refused\tP=%d\tB=%d\tshape=%d,%d,%d\tA=%d\tstatus=%d\n", P, B, s[0], s[1], s[2], A, p.status); ++bad; continue; }
                    seen_sg[p.sg] = true;
                    chunks.insert(p.chunk);
                    const std::string b = broken(P, B, s[0], s[1], s[2], A, p);
                    if (!b.empty()) { printf("%s\tP=%d\tB=%d\tshape=%d,%d,%d\tA=%d\tlds=%u\tchunk=%d\n", b.c_str(), P, B, s[0], s[1], s[2], A, p.lds, p.chunk); ++bad; }
                }
    }
    // ---- every refusal precedes a launch: the status, and a decision of zeros (no grid, no LDS)
    struct Case { const char* name; bool ptr; int P, B, C, H, W, A; int status; };
    const Case cases[] = {
        {"pointers", false, 2, 3, 4, 8, 8, 5, GSW_ERR_BAD_ARG},
        {"p_zero", true, 0, 3, 4, 8, 8, 5, GSW_ERR_BAD_ARG},
        {"p_five", true, 5, 3, 4, 8, 8, 5, GSW_ERR_BAD_ARG},
        {"b_zero", true, 2, 0, 4, 8, 8, 5, GSW_ERR_BAD_ARG},
        {"c_zero", true, 2, 3, 0, 8, 8, 5, GSW_ERR_BAD_ARG},
        {"h_negative", true, 2, 3, 4, -1, 8, 5, GSW_ERR_BAD_ARG},
        {"w_zero", true, 2, 3, 4, 8, 0, 5, GSW_ERR_BAD_ARG},
        {"a_zero", true, 2, 3, 4, 8, 8, 0, GSW_ERR_BAD_ARG},
        {"a_negative", true, 2, 3, 4, 8, 8, -2, GSW_ERR_BAD_ARG},
        {"ragged", true, 2, 3, 1, 3, 3, 5, GSW_ERR_RAGGED},
        {"past_domain_p1", true, 1, 3, 4, 512, 257, 5, GSW_ERR_UNSUPPORTED},
        {"past_domain_p4", true, 4, 3, 4, 256, 205, 5, GSW_ERR_UNSUPPORTED},
        {"huge_product", true, 1, 3, 2147483647, 2147483647, 2147483647, 5, GSW_ERR_UNSUPPORTED},
        {"b_65536", true, 2, 65536, 4, 8, 8, 5, GSW_ERR_UNSUPPORTED},
        {"order/bad_arg_before_ragged", true, 5, 3, 1, 3, 3, 5, GSW_ERR_BAD_ARG},
        {"order/unsupported_before_ragged", true, 2, 65536, 1, 3, 3, 5, GSW_ERR_UNSUPPORTED},
        {"ok/at_domain_p1", true, 1, 3, 4, 512, 256, 5, GSW_OK},
        {"ok/at_domain_p3", true, 3, 3, 4, 256, 256, 5, GSW_OK},
        {"ok/b_65535", true, 2, 65535, 4, 8, 8, 5, GSW_OK},
    };
    for (const Case& c : cases) {
        const LevelAlignPlan p = level_align_decide(c.ptr, c.P, c.B, c.C, c.H, c.W, c.A);
        ++n;
        const bool decided_nothing = p.sg == 0 && p.chunk == 0 && p.grid_x == 0 && p.grid_y == 0 && p.rowbytes == 0 && p.lstride == 0 && p.lds == 0;
        if (p.status != c.status || (c.status != GSW_OK && !decided_nothing) || (c.status == GSW_OK && !broken(c.P, c.B, c.C, c.H, c.W, c.A, p).empty())) {
            printf("refusal\t%s\tstatus=%d\n", c.name, p.status);
            ++bad;
        }
    }
    std::string seen;
    for (int c : chunks) seen += " chunk" + std::to_string(c);
    fprintf(stderr, "%lld inputs, %lld broken,%s%s%s\n", n, bad, seen_sg[0] ? " lds" : "", seen_sg[1] ? " sg" : "", seen.c_str());
    return 0;
}
