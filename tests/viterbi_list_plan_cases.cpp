// viterbi_list_plan_cases.cpp -- walks a grid of inputs of viterbi_list_decide (csrc/gswm_viterbi_list_plan.h) and prints every input whose decision breaks
// an invariant of a launch that no kernel checks, then every refusal case whose status or (all-zero) decision is not the expected one.  Host code only:
// tests/test_viterbi_list_plan_host.py builds it with the library's compiler; built with -fsanitize=address,undefined it is the sanitizer run of the policy.
//   viterbi_list_plan_cases      stdout: one line per broken input; stderr: "<inputs> inputs, <broken> broken, <classes seen>"
#include <cstdio>
#include <set>
#include <string>

#include <stddef.h>
#include <stdint.h>

#include "gswm.h"
#include "gswm_viterbi_list_plan.h"

static const uint32_t CU_LDS = 163840u;  // the bound restated: one wave's slice within the 160 KiB of a compute unit
static const uint32_t WG_LDS = 81920u;   // workgroups of several waves: half of it

static int64_t gcd64(int64_t a, int64_t b) {
    while (b) { const int64_t t = a % b; a = b; b = t; }
    return a;
}

static bool list_ok(int L) { return L == 1 || L == 2 || L == 4 || L == 8; }

// the slice restated from the README's formula, M (5 + 1/16 + 9 L / 2) + 256 L: 16 x that is M (81 + 72 L) + 4096 L, exactly
static int64_t slice(int64_t M, int L) {
    const int64_t x16 = M * (81 + 72 * (int64_t)L) + 4096 * (int64_t)L;
    return (x16 / 16 + 15) / 16 * 16;     // (M is a multiple of 16: x16 / 16 is exact)
}

// the status restated: BAD_ARG, then UNSUPPORTED
static int expected(bool ptr, int B, int64_t M, int64_t stride, int L) {
    if (!ptr || B < 1 || M < 64 || M % 16 || stride < M || !list_ok(L)) return GSW_ERR_BAD_ARG;
    if (slice(M, L) > (int64_t)CU_LDS) return GSW_ERR_UNSUPPORTED;
    return GSW_OK;
}

static bool decided_nothing(const ViterbiListPlan& p) {
    return !p.M && !p.T && !p.I && !p.info_bytes && !p.payload_bytes && !p.S && !p.Sinv && !p.L && !p.full_from && !p.waves && !p.wg && !p.grid && !p.wave_lds &&
           !p.lds;
}

static std::string broken(const ViterbiListQuery& q, const ViterbiListPlan& p) {
    std::string bad;
    auto need = [&](bool ok, const char* name) { if (!ok) bad += std::string(bad.empty() ? "" : ",") + name; };
    need(p.M == q.M && p.T * 2 == p.M && p.I == p.T - 6 && p.L == q.L, "sizes");
    need(p.info_bytes * 8 == p.T && p.info_bytes * 8 - 6 == p.I, "info_bytes");
    need(p.payload_bytes == (p.I - 16) / 8 && p.payload_bytes >= 1 && p.payload_bytes + 3 == p.info_bytes, "payload");
    int r = 0;
    while ((int64_t)(r + 1) * (r + 1) <= p.M) ++r;
    need((p.S & 1) && p.S >= (r | 1) && gcd64(p.S, p.M) == 1, "step");
    bool smallest = true;
    for (int s = r | 1; s < p.S; s += 2) smallest = smallest && gcd64(s, p.M) != 1;
    need(smallest, "step_is_smallest");
    need(p.Sinv >= 1 && p.Sinv < p.M && (int64_t)p.S * p.Sinv % p.M == 1, "inverse");
    need((int64_t)(p.M - 1) * p.Sinv < (1ll << 31) && (int64_t)(p.M - 1) * p.S < (1ll << 31), "index_products_fit_uint32");
    // every list is full from step 6 + log2 L on, and the mask-free steps exist: (1 << (full_from - 6)) == L, full_from <= I
    need(p.full_from >= 6 && (1 << (p.full_from - 6)) == p.L && p.full_from <= p.I, "full_from");
    // LDS: a wave's slice holds its six rows in the kernel's order, every row of 16-byte accesses starts 16-byte aligned, the workgroup's slices fit
    const int64_t rows = 4ll * p.M + 256ll * p.L + (int64_t)p.T * 8 * p.L + (int64_t)p.L * p.T + p.M + p.info_bytes;
    need((int64_t)p.wave_lds >= rows && p.wave_lds % 16 == 0 && (int64_t)p.wave_lds == slice(p.M, p.L), "wave_lds");
    need((4ll * p.M) % 16 == 0 && (4ll * p.M + 256ll * p.L) % 16 == 0, "rows_aligned");
    need(p.lds == (uint32_t)p.waves * p.wave_lds && p.lds <= CU_LDS && (p.waves == 1 || p.lds <= WG_LDS), "lds");
    need(p.waves == 1 || p.waves == 2 || p.waves == 4, "waves");
    need(p.wg == 64 * p.waves && p.wg <= 256, "wg");
    need(p.waves == 1 || p.waves / 2 < q.B, "waves_are_filled");
    need(p.waves == 4 || (uint32_t)(2 * p.waves) * p.wave_lds > WG_LDS || p.waves >= q.B, "waves_are_most");
    need(p.grid >= 1 && (int64_t)p.grid * p.waves >= q.B && (int64_t)(p.grid - 1) * p.waves < q.B, "grid");
    return bad;
}

int main() {
    long long n = 0, bad = 0;
    std::set<std::string> seen;
    const int Bs[] = {-1, 0, 1, 2, 3, 4, 5, 64, 70, 257, 16384, 2147483647};
    const int Ls[] = {0, 1, 2, 3, 4, 8, 16};
    int64_t largest[9] = {0};
    for (int64_t M = -16; M <= 8192 + 64; ++M)
        for (int L : Ls)
            for (int B : Bs)
                for (int64_t pad : {(int64_t)-1, (int64_t)0, (int64_t)16, (int64_t)1 << 33})
                    for (int ptr = 0; ptr < 2; ++ptr) {
                        if (M % 16 && (B > 3 || pad > 16)) continue;       // lengths off the grid: refused whatever else, a thinner sample
                        ViterbiListQuery q{};
                        q.pointers_ok = ptr; q.B = B; q.L = L; q.M = M; q.stride = M + pad;
                        const ViterbiListPlan p = viterbi_list_decide(q);
                        ++n;
                        const int want = expected(ptr, B, M, M + pad, L);
                        if (p.status != want || (want != GSW_OK && !decided_nothing(p))) {
                            printf("status\tM=%lld\tL=%d\tB=%d\tstride=%lld\tptr=%d\tstatus=%d\twant=%d\n", (long long)M, L, B, (long long)(M + pad), ptr, p.status, want);
                            ++bad;
                            continue;
                        }
                        if (want != GSW_OK) { seen.insert(want == GSW_ERR_BAD_ARG ? "bad_arg" : "unsupported"); continue; }
                        seen.insert("waves" + std::to_string(p.waves));
                        seen.insert("L" + std::to_string(p.L));
                        if (M > largest[L]) largest[L] = M;
                        if ((uint32_t)p.waves * 2 * p.wave_lds > WG_LDS && p.waves < 4 && B > p.waves) seen.insert("waves_cut_by_lds");
                        if (p.waves < 4 && (uint32_t)4 * p.wave_lds <= WG_LDS) seen.insert("waves_cut_by_batch");
                        if (p.waves == 1 && p.lds > WG_LDS) seen.insert("lone_wave_above_half");
                        const std::string b = broken(q, p);
                        if (!b.empty()) { printf("%s\tM=%lld\tL=%d\tB=%d\n", b.c_str(), (long long)M, L, B); ++bad; }
                    }
    // every multiple of 16 in 64 .. 2048 is served at every L; within the sweep L = 1, 2 and 4 reach its end and L = 8 stops at its bound
    for (int L : {1, 2, 4, 8})
        for (int64_t M = 64; M <= 2048; M += 16) {
            ViterbiListQuery q{};
            q.pointers_ok = true; q.B = 1; q.L = L; q.M = M; q.stride = M;
            ++n;
            if (viterbi_list_decide(q).status != GSW_OK) { printf("must_serve\tM=%lld\tL=%d\n", (long long)M, L); ++bad; }
        }
    // ---- the bound of each L, the known answers and every refusal, in the stated order when an input breaks several
    struct Case { const char* name; bool ptr; int B, L; int64_t M, stride; int status, S, payload, waves; };
    const Case cases[] = {
        {"pointers", false, 1, 4, 256, 256, GSW_ERR_BAD_ARG, 0, 0, 0},
        {"b_zero", true, 0, 4, 256, 256, GSW_ERR_BAD_ARG, 0, 0, 0},
        {"m_48", true, 1, 4, 48, 48, GSW_ERR_BAD_ARG, 0, 0, 0},
        {"m_not_16", true, 1, 4, 264, 264, GSW_ERR_BAD_ARG, 0, 0, 0},
        {"stride_short", true, 1, 4, 256, 255, GSW_ERR_BAD_ARG, 0, 0, 0},
        {"l_0", true, 1, 0, 256, 256, GSW_ERR_BAD_ARG, 0, 0, 0},
        {"l_3", true, 1, 3, 256, 256, GSW_ERR_BAD_ARG, 0, 0, 0},
        {"l_16", true, 1, 16, 256, 256, GSW_ERR_BAD_ARG, 0, 0, 0},
        {"l_negative", true, 1, -8, 256, 256, GSW_ERR_BAD_ARG, 0, 0, 0},
        {"bound/l1", true, 1, 1, 17104, 17104, GSW_OK, 131, 1066, 1},
        {"bound/l1_next", true, 1, 1, 17120, 17120, GSW_ERR_UNSUPPORTED, 0, 0, 0},
        {"bound/l2", true, 1, 2, 11600, 11600, GSW_OK, 107, 722, 1},
        {"bound/l2_next", true, 1, 2, 11616, 11616, GSW_ERR_UNSUPPORTED, 0, 0, 0},
        {"bound/l4", true, 1, 4, 7056, 7056, GSW_OK, 85, 438, 1},
        {"bound/l4_next", true, 1, 4, 7072, 7072, GSW_ERR_UNSUPPORTED, 0, 0, 0},
        {"bound/l8", true, 3, 8, 3936, 3936, GSW_OK, 65, 243, 1},
        {"bound/l8_next", true, 1, 8, 3952, 3952, GSW_ERR_UNSUPPORTED, 0, 0, 0},
        {"huge_m", true, 1, 1, (int64_t)1 << 31, (int64_t)1 << 31, GSW_ERR_UNSUPPORTED, 0, 0, 0},
        {"order/bad_arg_before_unsupported", true, 0, 8, 3952, 3952, GSW_ERR_BAD_ARG, 0, 0, 0},
        {"order/list_size_before_unsupported", true, 1, 16, 3952, 3952, GSW_ERR_BAD_ARG, 0, 0, 0},
        {"order/stride_before_unsupported", true, 1, 8, 3952, 100, GSW_ERR_BAD_ARG, 0, 0, 0},
        {"ok/m_64", true, 1, 8, 64, 64, GSW_OK, 9, 1, 1},
        {"ok/m_256_l8", true, 70, 8, 256, 272, GSW_OK, 17, 13, 4},
        {"ok/m_2048_l1", true, 3, 1, 2048, 2048, GSW_OK, 45, 125, 4},
        {"ok/m_2048_l4", true, 70, 4, 2048, 2048, GSW_OK, 45, 125, 1},
        {"ok/m_2048_l2", true, 70, 2, 2048, 2048, GSW_OK, 45, 125, 2},
        {"ok/two_images", true, 2, 2, 256, 256, GSW_OK, 17, 13, 2},
    };
    for (const Case& c : cases) {
        ViterbiListQuery q{};
        q.pointers_ok = c.ptr; q.B = c.B; q.L = c.L; q.M = c.M; q.stride = c.stride;
        const ViterbiListPlan p = viterbi_list_decide(q);
        ++n;
        const bool ok = p.status == c.status && p.status == expected(c.ptr, c.B, c.M, c.stride, c.L) &&
                        (c.status != GSW_OK ? decided_nothing(p) : broken(q, p).empty() && p.S == c.S && p.payload_bytes == c.payload && p.waves == c.waves);
        if (!ok) {
            printf("case\t%s\tstatus=%d\tS=%d\tpayload=%d\twaves=%d\n", c.name, p.status, p.S, p.payload_bytes, p.waves);
            ++bad;
        }
    }
    std::string classes;
    for (const auto& s : seen) classes += " " + s;
    fprintf(stderr, "%lld inputs, %lld broken,%s largest1=%lld largest8=%lld\n", n, bad, classes.c_str(), (long long)largest[1], (long long)largest[8]);
    return 0;
}
