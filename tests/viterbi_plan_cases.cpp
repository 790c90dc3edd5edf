// viterbi_plan_cases.cpp -- walks a grid of inputs of viterbi_decide (csrc/gswm_viterbi_plan.h) and prints every input whose decision breaks an invariant of a
// launch that no kernel checks, then every refusal case whose status or (all-zero) decision is not the expected one.  Host code only:
// tests/test_viterbi_plan_host.py builds it with the library's compiler; built with -fsanitize=address,undefined it is the sanitizer run of the policy.
//   viterbi_plan_cases      stdout: one line per broken input; stderr: "<inputs> inputs, <broken> broken, <classes seen>"
#include <cstdio>
#include <set>
#include <string>

#include <stddef.h>
#include <stdint.h>

#include "gswm.h"
#include "gswm_viterbi_plan.h"

static const uint32_t CAP = 98304u;     // the workgroup's rows restated: 96 KiB, within a CU's 160 KiB

static int64_t gcd64(int64_t a, int64_t b) {
    while (b) { const int64_t t = a % b; a = b; b = t; }
    return a;
}

// the status restated: BAD_ARG, then UNSUPPORTED
static int expected(bool ptr, int B, int64_t M, int64_t stride) {
    if (!ptr || B < 1 || M < 64 || M % 16 || stride < M) return GSW_ERR_BAD_ARG;
    if (M > 8192) return GSW_ERR_UNSUPPORTED;
    return GSW_OK;
}

static bool decided_nothing(const ViterbiPlan& p) {
    return !p.M && !p.T && !p.I && !p.info_bytes && !p.payload_bytes && !p.S && !p.Sinv && !p.waves && !p.wg && !p.grid && !p.wave_lds && !p.lds;
}

static std::string broken(const ViterbiQuery& q, const ViterbiPlan& p) {
    std::string bad;
    auto need = [&](bool ok, const char* name) { if (!ok) bad += std::string(bad.empty() ? "" : ",") + name; };
    need(p.M == q.M && p.T * 2 == p.M && p.I == p.T - 6, "sizes");
    need(p.info_bytes * 8 == p.T && p.info_bytes * 8 - 6 == p.I, "info_bytes");               // the tail fills the last byte
    need(p.payload_bytes == (p.I - 16) / 8 && p.payload_bytes >= 1 && p.payload_bytes + 3 == p.info_bytes, "payload");
    // the interleaver: odd, coprime to M, the smallest such from isqrt(M) | 1 on, and Sinv its inverse
    int r = 0;
    while ((int64_t)(r + 1) * (r + 1) <= p.M) ++r;
    need((p.S & 1) && p.S >= (r | 1) && gcd64(p.S, p.M) == 1, "step");
    bool smallest = true;
    for (int s = r | 1; s < p.S; s += 2) smallest = smallest && gcd64(s, p.M) != 1;
    need(smallest, "step_is_smallest");
    need(p.Sinv >= 1 && p.Sinv < p.M && (int64_t)p.S * p.Sinv % p.M == 1, "inverse");
    need((int64_t)(p.M - 1) * p.Sinv < (1ll << 31) && (int64_t)(p.M - 1) * p.S < (1ll << 31), "index_products_fit_uint32");
    // LDS: a wave's slice holds its five rows, slices are 16-byte aligned, the workgroup's fit the cap
    need(p.wave_lds >= (uint32_t)(4 * p.M + 8 * p.T + p.T + p.M + p.info_bytes) && p.wave_lds % 16 == 0, "wave_lds");
    need(p.lds == (uint32_t)p.waves * p.wave_lds && p.lds <= CAP, "lds");
    need(p.waves == 1 || p.waves == 2 || p.waves == 4, "waves");
    need(p.wg == 64 * p.waves && p.wg <= 256, "wg");
    need(p.waves == 1 || p.waves / 2 < q.B, "waves_are_filled");                             // 2 waves need 2 images, 4 need 3
    need(p.waves == 4 || (uint32_t)(2 * p.waves) * p.wave_lds > CAP || p.waves >= q.B, "waves_are_most");   // the next larger workgroup would not fit or not fill
    need(p.grid >= 1 && (int64_t)p.grid * p.waves >= q.B && (int64_t)(p.grid - 1) * p.waves < q.B, "grid");   // every image once
    return bad;
}

int main() {
    long long n = 0, bad = 0;
    std::set<std::string> seen;
    const int Bs[] = {-1, 0, 1, 2, 3, 4, 5, 64, 70, 257, 16384, 2147483647};
    for (int64_t M = -16; M <= 8192 + 64; ++M)
        for (int B : Bs)
            for (int64_t pad : {(int64_t)-1, (int64_t)0, (int64_t)16, (int64_t)1 << 33})
                for (int ptr = 0; ptr < 2; ++ptr) {
                    ViterbiQuery q{};
                    q.pointers_ok = ptr; q.B = B; q.M = M; q.stride = M + pad;
                    const ViterbiPlan p = viterbi_decide(q);
                    ++n;
                    const int want = expected(ptr, B, M, M + pad);
                    if (p.status != want || (want != GSW_OK && !decided_nothing(p))) {
                        printf("status\tM=%lld\tB=%d\tstride=%lld\tptr=%d\tstatus=%d\twant=%d\n", (long long)M, B, (long long)(M + pad), ptr, p.status, want);
                        ++bad;
                        continue;
                    }
                    if (want != GSW_OK) { seen.insert(want == GSW_ERR_BAD_ARG ? "bad_arg" : "unsupported"); continue; }
                    seen.insert("waves" + std::to_string(p.waves));
                    int root = 0;
                    while ((int64_t)(root + 1) * (root + 1) <= p.M) ++root;
                    if (p.S != (root | 1)) seen.insert("step_moved_on");
                    if ((uint32_t)p.waves * 2 * p.wave_lds > CAP && p.waves < 4 && B > p.waves) seen.insert("waves_cut_by_lds");
                    if (p.waves < 4 && (uint32_t)4 * p.wave_lds <= CAP) seen.insert("waves_cut_by_batch");
                    const std::string b = broken(q, p);
                    if (!b.empty()) { printf("%s\tM=%lld\tB=%d\n", b.c_str(), (long long)M, B); ++bad; }
                }
    // ---- the known answers and every refusal, in the stated order when an input breaks several
    struct Case { const char* name; bool ptr; int B; int64_t M, stride; int status, S, payload, waves; };
    const Case cases[] = {
        {"pointers", false, 1, 256, 256, GSW_ERR_BAD_ARG, 0, 0, 0},
        {"b_zero", true, 0, 256, 256, GSW_ERR_BAD_ARG, 0, 0, 0},
        {"m_48", true, 1, 48, 48, GSW_ERR_BAD_ARG, 0, 0, 0},
        {"m_not_16", true, 1, 264, 264, GSW_ERR_BAD_ARG, 0, 0, 0},
        {"stride_short", true, 1, 256, 255, GSW_ERR_BAD_ARG, 0, 0, 0},
        {"m_8208", true, 1, 8208, 8208, GSW_ERR_UNSUPPORTED, 0, 0, 0},
        {"order/bad_arg_before_unsupported", true, 0, 8208, 8208, GSW_ERR_BAD_ARG, 0, 0, 0},
        {"order/stride_before_unsupported", true, 1, 8208, 100, GSW_ERR_BAD_ARG, 0, 0, 0},
        {"ok/m_64", true, 1, 64, 64, GSW_OK, 9, 1, 1},
        {"ok/m_256", true, 70, 256, 272, GSW_OK, 17, 13, 4},
        {"ok/m_2048", true, 3, 2048, 2048, GSW_OK, 45, 125, 4},
        {"ok/m_4096", true, 257, 4096, 4096, GSW_OK, 65, 253, 2},
        {"ok/m_8192", true, 257, 8192, 8192, GSW_OK, 91, 509, 1},
        {"ok/two_images", true, 2, 256, 256, GSW_OK, 17, 13, 2},
    };
    for (const Case& c : cases) {
        ViterbiQuery q{};
        q.pointers_ok = c.ptr; q.B = c.B; q.M = c.M; q.stride = c.stride;
        const ViterbiPlan p = viterbi_decide(q);
        ++n;
        const bool ok = p.status == c.status && (c.status != GSW_OK ? decided_nothing(p)
                                                                     : broken(q, p).empty() && p.S == c.S && p.payload_bytes == c.payload && p.waves == c.waves);
        if (!ok) {
            printf("case\t%s\tstatus=%d\tS=%d\tpayload=%d\twaves=%d\n", c.name, p.status, p.S, p.payload_bytes, p.waves);
            ++bad;
        }
    }
    std::string classes;
    for (const auto& s : seen) classes += " " + s;
    fprintf(stderr, "%lld inputs, %lld broken,%s\n", n, bad, classes.c_str());
    return 0;
}
