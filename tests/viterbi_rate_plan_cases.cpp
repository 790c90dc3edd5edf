// viterbi_rate_plan_cases.cpp -- walks a grid of inputs of viterbi_rate_decide (csrc/gswm_viterbi_rate_plan.h) and prints every input whose decision breaks
// an invariant of a launch that no kernel checks, every rate-0 decision that differs from viterbi_decide's or viterbi_list_decide's in any field, then every
// refusal case whose status or (all-zero) decision is not the expected one.  Host code only: tests/test_viterbi_rate_plan_host.py builds it with the
// library's compiler, plain and with -fsanitize=address,undefined (the sanitizer run of the policy).
//   viterbi_rate_plan_cases      stdout: one line per broken input; stderr: "<inputs> inputs, <broken> broken, <classes seen>"
#include <cstdio>
#include <set>
#include <string>

#include <stddef.h>
#include <stdint.h>

#include "gswm.h"
#include "gswm_viterbi_plan.h"
#include "gswm_viterbi_list_plan.h"
#include "gswm_viterbi_rate_plan.h"

static const int64_t CU_LDS = 163840;    // one wave's list slice within the 160 KiB of a compute unit
static const int64_t WG_LDS = 81920;     // list workgroups of several waves: half of it
static const int64_t PLAIN_LDS = 98304;  // the plain read's workgroup: 96 KiB

static int64_t gcd64(int64_t a, int64_t b) {
    while (b) { const int64_t t = a % b; a = b; b = t; }
    return a;
}

static bool list_ok(int L) { return L == 1 || L == 2 || L == 4 || L == 8; }

// N(t) restated by brute force: walk the pattern table of the issue, step by step
static int64_t kept_brute(int rate, int64_t t) {
    static const int keep[3][3] = {{2, 0, 0}, {2, 1, 0}, {2, 1, 1}};
    int64_t n = 0;
    for (int64_t i = 0; i < t; ++i) n += keep[rate][i % (rate + 1)];
    return n;
}

// N(t) restated in the issue's closed forms
static int64_t kept_closed(int rate, int64_t t) {
    static const int64_t rest[3] = {0, 2, 3};
    return rate == 0 ? 2 * t : rate == 1 ? 3 * (t / 2) + 2 * (t % 2) : 4 * (t / 3) + rest[t % 3];
}

// T restated: the largest multiple of 8 with N(T) <= M, by search from above
static int64_t steps(int rate, int64_t M) {
    int64_t T = M / 8 * 8;
    while (kept_closed(rate, T) > M) T -= 8;
    return T;
}

static int64_t slice(int64_t M, int64_t T, bool list, int L) {
    const int64_t raw = list ? 4 * M + 256 * (int64_t)L + 9 * T * L + M + T / 8 : 4 * M + 8 * T + T + M + T / 8;
    return (raw + 15) / 16 * 16;
}

// the status restated: BAD_ARG, then UNSUPPORTED
static int expected(bool ptr, bool list, int B, int64_t M, int64_t stride, int L, int rate) {
    if (!ptr || B < 1 || M < 64 || M % 16 || stride < M || (list && !list_ok(L)) || rate < 0 || rate > 2) return GSW_ERR_BAD_ARG;
    if (list ? (M > CU_LDS || slice(M, steps(rate, M), true, L) > CU_LDS) : M > 8192) return GSW_ERR_UNSUPPORTED;
    return GSW_OK;
}

static bool decided_nothing(const ViterbiRatePlan& p) {
    return !p.M && !p.T && !p.I && !p.N && !p.info_bytes && !p.payload_bytes && !p.S && !p.Sinv && !p.rate && !p.L && !p.full_from && !p.waves && !p.wg &&
           !p.grid && !p.wave_lds && !p.lds;
}

static std::string broken(const ViterbiRateQuery& q, const ViterbiRatePlan& p) {
    std::string bad;
    auto need = [&](bool ok, const char* name) { if (!ok) bad += std::string(bad.empty() ? "" : ",") + name; };
    const int L = q.list ? q.L : 1;
    need(p.M == q.M && p.rate == q.rate && p.L == L, "echo");
    need(p.T == steps(q.rate, q.M) && p.T % 8 == 0 && p.T >= 32 && p.I == p.T - 6, "steps");
    need(p.N == kept_closed(q.rate, p.T) && p.N <= p.M && kept_closed(q.rate, p.T + 8) > p.M && p.N >= p.T, "kept");
    need(p.info_bytes * 8 == p.T && p.payload_bytes == p.info_bytes - 3 && p.payload_bytes >= 1 && p.I - 16 - 8 * p.payload_bytes == 2, "info_word");
    int r = 0;
    while ((int64_t)(r + 1) * (r + 1) <= p.M) ++r;
    need((p.S & 1) && p.S >= (r | 1) && gcd64(p.S, p.M) == 1, "step");
    bool smallest = true;
    for (int s = r | 1; s < p.S; s += 2) smallest = smallest && gcd64(s, p.M) != 1;
    need(smallest, "step_is_smallest");
    need(p.Sinv >= 1 && p.Sinv < p.M && (int64_t)p.S * p.Sinv % p.M == 1, "inverse");
    need((int64_t)(p.M - 1) * p.Sinv < (1ll << 31) && (int64_t)(p.M - 1) * p.S < (1ll << 31), "index_products_fit_uint32");
    need(p.full_from >= 6 && (1 << (p.full_from - 6)) == p.L && p.full_from <= p.I, "full_from");
    // the last vote any step reads lies below N; a whole period inside the info steps never reads past it
    const int P = q.rate + 1;
    need(kept_closed(q.rate, (int64_t)p.I / P * P) <= p.N, "periods_read_below_n");
    // LDS: the slice holds its rows in the kernels' order, rows of wide accesses start 16-byte aligned
    const int64_t rows = q.list ? 4ll * p.M + 256ll * L + (int64_t)p.T * 8 * L + (int64_t)L * p.T + p.M + p.info_bytes
                                : 4ll * p.M + 8ll * p.T + p.T + p.M + p.info_bytes;
    need((int64_t)p.wave_lds >= rows && p.wave_lds % 16 == 0 && (int64_t)p.wave_lds == slice(p.M, p.T, q.list, L), "wave_lds");
    need((4ll * p.M) % 16 == 0 && (4ll * p.M + 256ll * L) % 16 == 0, "rows_aligned");
    const int64_t wg_lds = q.list ? WG_LDS : PLAIN_LDS;
    need(p.lds == (uint32_t)p.waves * p.wave_lds && (int64_t)p.lds <= (q.list ? CU_LDS : PLAIN_LDS) && (p.waves == 1 || (int64_t)p.lds <= wg_lds), "lds");
    need(p.waves == 1 || p.waves == 2 || p.waves == 4, "waves");
    need(p.wg == 64 * p.waves && p.wg <= 256, "wg");
    need(p.waves == 1 || p.waves / 2 < q.B, "waves_are_filled");
    need(p.waves == 4 || (int64_t)(2 * p.waves) * p.wave_lds > wg_lds || p.waves >= q.B, "waves_are_most");
    need(p.grid >= 1 && (int64_t)p.grid * p.waves >= q.B && (int64_t)(p.grid - 1) * p.waves < q.B, "grid");
    return bad;
}

// rate 0: the plan equals the older plan of the same entry point, field for field (refusals included)
static bool equals_older(const ViterbiRateQuery& q, const ViterbiRatePlan& p) {
    if (q.list) {
        ViterbiListQuery o{};
        o.pointers_ok = q.pointers_ok; o.B = q.B; o.L = q.L; o.M = q.M; o.stride = q.stride;
        const ViterbiListPlan w = viterbi_list_decide(o);
        if (w.status != GSW_OK) return p.status == w.status;
        return p.status == w.status && p.M == w.M && p.T == w.T && p.I == w.I && p.N == w.M && p.info_bytes == w.info_bytes && p.payload_bytes == w.payload_bytes &&
               p.S == w.S && p.Sinv == w.Sinv && p.L == w.L && p.full_from == w.full_from && p.waves == w.waves && p.wg == w.wg && p.grid == w.grid &&
               p.wave_lds == w.wave_lds && p.lds == w.lds;
    }
    ViterbiQuery o{};
    o.pointers_ok = q.pointers_ok; o.B = q.B; o.M = q.M; o.stride = q.stride;
    const ViterbiPlan w = viterbi_decide(o);
    if (w.status != GSW_OK) return p.status == w.status;
    return p.status == w.status && p.M == w.M && p.T == w.T && p.I == w.I && p.N == w.M && p.info_bytes == w.info_bytes && p.payload_bytes == w.payload_bytes &&
           p.S == w.S && p.Sinv == w.Sinv && p.L == 1 && p.full_from == 6 && p.waves == w.waves && p.wg == w.wg && p.grid == w.grid && p.wave_lds == w.wave_lds &&
           p.lds == w.lds;
}

int main() {
    long long n = 0, bad = 0;
    std::set<std::string> seen;
    // N(t): the plan's function, the closed forms and the brute-force count agree
    for (int rate = 0; rate < 3; ++rate)
        for (int64_t t = 0; t <= 4200; ++t) {
            ++n;
            if (viterbi_rate_kept_bits(rate, t) != kept_brute(rate, t) || kept_closed(rate, t) != kept_brute(rate, t)) {
                printf("kept_bits\trate=%d\tt=%lld\n", rate, (long long)t);
                ++bad;
            }
        }
    const int Bs[] = {-1, 0, 1, 2, 3, 4, 5, 64, 257, 16384, 2147483647};
    const int Ls[] = {0, 1, 2, 3, 4, 8, 16};
    const int rates[] = {-1, 0, 1, 2, 3};
    int64_t largest[2][3][9] = {};
    for (int64_t M = -16; M <= 8192 + 64; ++M)
        for (int rate : rates)
            for (int list = 0; list < 2; ++list)
                for (int L : Ls)
                    for (int B : Bs)
                        for (int64_t pad : {(int64_t)-1, (int64_t)0, (int64_t)16, (int64_t)1 << 33})
                            for (int ptr = 0; ptr < 2; ++ptr) {
                                if (M % 16 && (B > 3 || pad > 16 || B < 0)) continue;  // lengths off the grid: refused whatever else, a thinner sample
                                if (!list && L != 0 && L != 3) continue;               // the plain read does not read L: two values show it
                                ViterbiRateQuery q{};
                                q.pointers_ok = ptr; q.list = list; q.B = B; q.L = L; q.rate = rate; q.M = M; q.stride = M + pad;
                                const ViterbiRatePlan p = viterbi_rate_decide(q);
                                ++n;
                                const int want = expected(ptr, list, B, M, M + pad, L, rate);
                                if (p.status != want || (want != GSW_OK && !decided_nothing(p))) {
                                    printf("status\tM=%lld\trate=%d\tlist=%d\tL=%d\tB=%d\tstride=%lld\tptr=%d\tstatus=%d\twant=%d\n", (long long)M, rate, list, L, B,
                                           (long long)(M + pad), ptr, p.status, want);
                                    ++bad;
                                    continue;
                                }
                                if (rate == 0 && !equals_older(q, p)) {
                                    printf("rate0_differs\tM=%lld\tlist=%d\tL=%d\tB=%d\tstride=%lld\tptr=%d\n", (long long)M, list, L, B, (long long)(M + pad), ptr);
                                    ++bad;
                                }
                                if (want != GSW_OK) { seen.insert(want == GSW_ERR_BAD_ARG ? "bad_arg" : list ? "unsupported_list" : "unsupported_plain"); continue; }
                                seen.insert("waves" + std::to_string(p.waves));
                                seen.insert("rate" + std::to_string(p.rate));
                                seen.insert(list ? "L" + std::to_string(p.L) : "plain");
                                if (M > largest[list][rate][p.L]) largest[list][rate][p.L] = M;
                                if (p.M - p.N > 0) seen.insert("spare");
                                if (p.I % (rate + 1)) seen.insert("tail_inside_a_period");
                                if (p.full_from % (rate + 1)) seen.insert("entry_inside_a_period");
                                if (!list && p.lds > 96u * 1024u - 2048u) seen.insert("plain_lds_near_the_limit");
                                if (list && p.waves == 1 && (int64_t)p.lds > WG_LDS) seen.insert("lone_wave_above_half");
                                const std::string b = broken(q, p);
                                if (!b.empty()) { printf("%s\tM=%lld\trate=%d\tlist=%d\tL=%d\tB=%d\n", b.c_str(), (long long)M, rate, list, L, B); ++bad; }
                            }
    // every multiple of 16 in 64 .. 2048 is served at every L and every rate; the plain read serves every M up to 8192 at every rate
    for (int rate = 0; rate < 3; ++rate) {
        for (int L : {1, 2, 4, 8})
            for (int64_t M = 64; M <= 2048; M += 16) {
                ViterbiRateQuery q{};
                q.pointers_ok = true; q.list = true; q.B = 1; q.L = L; q.rate = rate; q.M = M; q.stride = M;
                ++n;
                if (viterbi_rate_decide(q).status != GSW_OK) { printf("must_serve\tM=%lld\trate=%d\tL=%d\n", (long long)M, rate, L); ++bad; }
            }
        for (int64_t M = 64; M <= 8192; M += 16) {
            ViterbiRateQuery q{};
            q.pointers_ok = true; q.list = false; q.B = 1; q.rate = rate; q.M = M; q.stride = M;
            ++n;
            if (viterbi_rate_decide(q).status != GSW_OK) { printf("must_serve_plain\tM=%lld\trate=%d\n", (long long)M, rate); ++bad; }
        }
    }
    // ---- the issue's worked sizes, the bound of each (rate, L), and every refusal, in the stated order when an input breaks several
    struct Case { const char* name; bool ptr, list; int B, L, rate; int64_t M, stride; int status, T, N, payload, waves; uint32_t wave_lds; };
    const Case cases[] = {
        {"size/64_conv23", true, false, 1, 0, 1, 64, 64, GSW_OK, 40, 60, 2, 1, 0},
        {"size/64_conv34", true, false, 1, 0, 2, 64, 64, GSW_OK, 48, 64, 3, 1, 0},
        {"size/80_conv34", true, false, 1, 0, 2, 80, 80, GSW_OK, 56, 75, 4, 1, 0},
        {"size/256_conv23", true, false, 70, 0, 1, 256, 272, GSW_OK, 168, 252, 18, 4, 0},
        {"size/256_conv34", true, true, 70, 4, 2, 256, 256, GSW_OK, 192, 256, 21, 4, 0},
        {"size/2048_conv23", true, true, 1, 8, 1, 2048, 2048, GSW_OK, 1360, 2040, 167, 1, 0},
        {"size/2048_conv34", true, false, 70, 0, 2, 2048, 2048, GSW_OK, 1536, 2048, 189, 4, 0},
        {"size/8192_conv23", true, false, 70, 0, 1, 8192, 8192, GSW_OK, 5456, 8184, 679, 1, 0},
        {"size/8192_conv34", true, false, 70, 0, 2, 8192, 8192, GSW_OK, 6144, 8192, 765, 1, 97024},
        {"size/8192_conv", true, false, 70, 0, 0, 8192, 8192, GSW_OK, 4096, 8192, 509, 1, 0},
        {"bound/conv23_l1", true, true, 1, 1, 1, 14752, 14752, GSW_OK, 9832, 14748, 1226, 1, 0},
        {"bound/conv23_l1_next", true, true, 1, 1, 1, 14768, 14768, GSW_ERR_UNSUPPORTED, 0, 0, 0, 0, 0},
        {"bound/conv23_l2", true, true, 1, 2, 1, 9552, 9552, GSW_OK, 6368, 9552, 793, 1, 0},
        {"bound/conv23_l2_next", true, true, 1, 2, 1, 9568, 9568, GSW_ERR_UNSUPPORTED, 0, 0, 0, 0, 0},
        {"bound/conv23_l4", true, true, 1, 4, 1, 5600, 5600, GSW_OK, 3728, 5592, 463, 1, 0},
        {"bound/conv23_l4_next", true, true, 1, 4, 1, 5616, 5616, GSW_ERR_UNSUPPORTED, 0, 0, 0, 0, 0},
        {"bound/conv23_l8", true, true, 3, 8, 1, 3040, 3040, GSW_OK, 2024, 3036, 250, 1, 0},
        {"bound/conv23_l8_next", true, true, 1, 8, 1, 3056, 3056, GSW_ERR_UNSUPPORTED, 0, 0, 0, 0, 0},
        {"bound/conv34_l1", true, true, 1, 1, 2, 13808, 13808, GSW_OK, 10352, 13803, 1291, 1, 0},
        {"bound/conv34_l1_next", true, true, 1, 1, 2, 13824, 13824, GSW_ERR_UNSUPPORTED, 0, 0, 0, 0, 0},
        {"bound/conv34_l2", true, true, 1, 2, 2, 8784, 8784, GSW_OK, 6584, 8779, 820, 1, 0},
        {"bound/conv34_l2_next", true, true, 1, 2, 2, 8800, 8800, GSW_ERR_UNSUPPORTED, 0, 0, 0, 0, 0},
        {"bound/conv34_l4", true, true, 1, 4, 2, 5072, 5072, GSW_OK, 3800, 5067, 472, 1, 0},
        {"bound/conv34_l4_next", true, true, 1, 4, 2, 5088, 5088, GSW_ERR_UNSUPPORTED, 0, 0, 0, 0, 0},
        {"bound/conv34_l8", true, true, 3, 8, 2, 2736, 2736, GSW_OK, 2048, 2731, 253, 1, 0},
        {"bound/conv34_l8_next", true, true, 1, 8, 2, 2752, 2752, GSW_ERR_UNSUPPORTED, 0, 0, 0, 0, 0},
        {"bound/conv_l1", true, true, 1, 1, 0, 17104, 17104, GSW_OK, 8552, 17104, 1066, 1, 0},
        {"bound/conv_l1_next", true, true, 1, 1, 0, 17120, 17120, GSW_ERR_UNSUPPORTED, 0, 0, 0, 0, 0},
        {"bound/plain_next", true, false, 1, 0, 2, 8208, 8208, GSW_ERR_UNSUPPORTED, 0, 0, 0, 0, 0},
        {"huge_m", true, true, 1, 1, 2, (int64_t)1 << 31, (int64_t)1 << 31, GSW_ERR_UNSUPPORTED, 0, 0, 0, 0, 0},
        {"huge_m_plain", true, false, 1, 1, 1, (int64_t)1 << 40, (int64_t)1 << 40, GSW_ERR_UNSUPPORTED, 0, 0, 0, 0, 0},
        {"pointers", false, false, 1, 0, 1, 256, 256, GSW_ERR_BAD_ARG, 0, 0, 0, 0, 0},
        {"b_zero", true, true, 0, 4, 1, 256, 256, GSW_ERR_BAD_ARG, 0, 0, 0, 0, 0},
        {"m_48", true, false, 1, 0, 2, 48, 48, GSW_ERR_BAD_ARG, 0, 0, 0, 0, 0},
        {"m_not_16", true, true, 1, 4, 2, 264, 264, GSW_ERR_BAD_ARG, 0, 0, 0, 0, 0},
        {"stride_short", true, false, 1, 0, 1, 256, 255, GSW_ERR_BAD_ARG, 0, 0, 0, 0, 0},
        {"l_3", true, true, 1, 3, 1, 256, 256, GSW_ERR_BAD_ARG, 0, 0, 0, 0, 0},
        {"rate_3", true, false, 1, 0, 3, 256, 256, GSW_ERR_BAD_ARG, 0, 0, 0, 0, 0},
        {"rate_negative", true, true, 1, 4, -1, 256, 256, GSW_ERR_BAD_ARG, 0, 0, 0, 0, 0},
        {"order/rate_before_unsupported", true, false, 1, 0, 3, 8208, 8208, GSW_ERR_BAD_ARG, 0, 0, 0, 0, 0},
        {"order/rate_before_unsupported_list", true, true, 1, 8, 5, 3056, 3056, GSW_ERR_BAD_ARG, 0, 0, 0, 0, 0},
        {"order/list_size_before_unsupported", true, true, 1, 16, 1, 3056, 3056, GSW_ERR_BAD_ARG, 0, 0, 0, 0, 0},
        {"order/stride_before_unsupported", true, true, 1, 8, 2, 2752, 100, GSW_ERR_BAD_ARG, 0, 0, 0, 0, 0},
        {"order/batch_before_unsupported", true, false, 0, 0, 2, 8208, 8208, GSW_ERR_BAD_ARG, 0, 0, 0, 0, 0},
    };
    for (const Case& c : cases) {
        ViterbiRateQuery q{};
        q.pointers_ok = c.ptr; q.list = c.list; q.B = c.B; q.L = c.L; q.rate = c.rate; q.M = c.M; q.stride = c.stride;
        const ViterbiRatePlan p = viterbi_rate_decide(q);
        ++n;
        const bool ok = p.status == c.status && p.status == expected(c.ptr, c.list, c.B, c.M, c.stride, c.L, c.rate) &&
                        (c.status != GSW_OK ? decided_nothing(p)
                                            : broken(q, p).empty() && p.T == c.T && p.N == c.N && p.payload_bytes == c.payload && p.waves == c.waves &&
                                                  (!c.wave_lds || p.wave_lds == c.wave_lds));
        if (!ok) {
            printf("case\t%s\tstatus=%d\tT=%d\tN=%d\tpayload=%d\twaves=%d\twave_lds=%u\n", c.name, p.status, p.T, p.N, p.payload_bytes, p.waves, p.wave_lds);
            ++bad;
        }
    }
    std::string classes;
    for (const auto& s : seen) classes += " " + s;
    fprintf(stderr, "%lld inputs, %lld broken,%s", n, bad, classes.c_str());
    for (int rate = 0; rate < 3; ++rate) fprintf(stderr, " plain%d=%lld list%d_8=%lld", rate, (long long)largest[0][rate][1], rate, (long long)largest[1][rate][8]);
    fprintf(stderr, "\n");
    return 0;
}
