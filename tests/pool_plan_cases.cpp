// pool_plan_cases.cpp -- walks a grid of inputs of pool_decide (csrc/gswm_pool_plan.h) for both of its kinds and prints every input whose decision breaks an
// invariant of a launch that no kernel checks, then every refusal case whose status or (all-zero) decision is not the expected one.  Host code only:
// tests/test_trace_pool_host.py builds it with the library's compiler; built with -fsanitize=address,undefined it is the sanitizer run of the policy.
//   pool_plan_cases      stdout: one line per broken input; stderr: "<inputs> inputs, <broken> broken, <classes seen>"
#include <cstdio>
#include <set>
#include <string>

#include <stddef.h>
#include <stdint.h>

#include "gswm.h"
#include "gswm_pool_plan.h"

static const uint32_t CAP = 131072u;    // the tile restated: 128 KiB, within a CU's 160 KiB

static int bit_length(__int128 v) {
    int q = 0;
    for (; v > 0; v >>= 1) ++q;
    return q;
}

// the status of pooling restated: BAD_ARG, then UNSUPPORTED (128-bit products: nothing overflows)
static int expected_rows(bool ptr, int P, int B, int G, int max_set, int Q, int64_t n) {
    if (!ptr || G < 1 || n < 1 || Q < 1) return GSW_ERR_BAD_ARG;
    if (P < 0 || P > 4 || B < 1 || G > B || max_set < 1 || max_set > B || n % 8) return GSW_ERR_BAD_ARG;
    const int need = bit_length((__int128)(P ? (1 << P) - 1 : 1) * max_set);
    if (need <= 10 && Q < need) return GSW_ERR_BAD_ARG;
    if (Q > 10 || need > 10) return GSW_ERR_UNSUPPORTED;
    if ((__int128)n * (1 + Q) > 1048576 || (__int128)n * ((1 << Q) - 1) >= ((__int128)1 << 31)) return GSW_ERR_UNSUPPORTED;
    return GSW_OK;
}

// ... of the search: BAD_ARG, then RAGGED, then UNSUPPORTED
static int expected_search(bool ptr, bool rec, bool rec16, int G, int Q, int64_t n, int64_t stride, int mb, int64_t U, int k) {
    if (!ptr || G < 1 || n < 1 || Q < 1) return GSW_ERR_BAD_ARG;
    if (k < 1 || k > 8 || U > 2147483647ll) return GSW_ERR_BAD_ARG;
    if (!rec || U < 1 || mb < 1 || mb > GSW_MSG_INLINE_MAX || stride < 48 + mb || stride % 16 || !rec16) return GSW_ERR_BAD_ARG;
    if (n % (8 * (int64_t)mb)) return GSW_ERR_RAGGED;
    if (Q > 10) return GSW_ERR_UNSUPPORTED;
    if ((__int128)n * (1 + Q) > 1048576 || (__int128)n * ((1 << Q) - 1) >= ((__int128)1 << 31)) return GSW_ERR_UNSUPPORTED;
    if (G > 65535) return GSW_ERR_UNSUPPORTED;
    if ((__int128)(1 + Q) * ((n / 8 + 63) / 64) * 64 > CAP) return GSW_ERR_UNSUPPORTED;
    return GSW_OK;
}

static bool decided_nothing(const PoolPlan& p) {
    return !p.Q && !p.T && !p.msg4 && !p.rowbytes && !p.rowwords && !p.nblk && !p.rows_aligned && !p.grid_x && !p.grid_y && !p.wg && !p.lds && !p.ws_bytes;
}

static std::string broken_rows(const PoolQuery& q, const PoolPlan& p) {
    std::string bad;
    auto need = [&](bool ok, const char* name) { if (!ok) bad += std::string(bad.empty() ? "" : ",") + name; };
    need(p.Q == q.Q && p.Q >= 1 && p.Q <= 10, "q");
    need(((int64_t)(q.P ? (1 << q.P) - 1 : 1)) * q.max_set < (1ll << p.Q), "planes_hold_the_sets");
    need(p.rowbytes * 8ll == q.n_bits && p.rowwords * 4 >= p.rowbytes && (p.rowwords - 1) * 4 < p.rowbytes, "row");
    need(!p.rows_aligned || (q.rows_aligned && p.rowbytes % 4 == 0), "aligned");
    need(p.grid_x == q.G && p.grid_y == 1, "one_workgroup_per_set");                     // the grid covers every set exactly once
    need(p.wg >= 64 && p.wg <= 512 && (p.wg & (p.wg - 1)) == 0 && (p.wg == 64 || p.wg / 2 < p.rowwords), "wg");
    need(p.lds == 0 && p.ws_bytes == 0 && p.T == 0 && p.nblk == 0, "search_fields");
    need(q.n_bits * ((1ll << p.Q) - 1) < (1ll << 31), "int32");                          // wsum and every score
    return bad;
}

static std::string broken_search(const PoolQuery& q, const PoolPlan& p) {
    std::string bad;
    auto need = [&](bool ok, const char* name) { if (!ok) bad += std::string(bad.empty() ? "" : ",") + name; };
    need(p.Q == q.Q && p.Q >= 1 && p.Q <= 10, "q");
    need(p.rowbytes * 8ll == q.n_bits, "row");
    need(p.nblk * 64 >= p.rowbytes && (p.nblk - 1) * 64 < p.rowbytes, "nblk");
    need(!p.rows_aligned || (q.rows_aligned && p.rowbytes % 4 == 0), "aligned");
    need(p.msg4 == (q.msg_bytes % 4 == 0), "msg4");
    need(p.T == 1 || p.T == 4 || p.T == 16, "tile");
    const uint64_t staged = (uint64_t)p.T * (1 + p.Q) * p.nblk * 64;
    need(staged <= CAP && POOL_TILE_LDS <= CAP, "rows_fit_the_tile");
    need(p.lds >= staged && p.lds >= (uint32_t)(8 * p.T * 8 * 8) && p.lds <= CAP, "lds");
    need(p.T == 1 || q.G > p.T / 4, "tile_is_filled");                                   // a tile of 4 needs 2 sets, one of 16 needs 5
    need(p.T == 16 || q.G <= (p.T == 1 ? 1 : 4) || (uint64_t)(p.T * 4) * (1 + p.Q) * p.nblk * 64 > CAP, "tile_is_largest");
    need(p.grid_y >= 1 && (int64_t)p.grid_y * p.T >= q.G && (int64_t)(p.grid_y - 1) * p.T < q.G && p.grid_y <= 65535, "grid_y");   // every set once
    need(p.grid_x >= 1 && p.grid_x <= 512 && p.grid_x <= q.n_records, "grid_x");        // record ranges u0 = U x / grid_x: none empty, all covered
    need(p.wg == 512, "wg");
    need(p.ws_bytes == (size_t)q.G * (size_t)p.grid_x * (size_t)q.k * 8 && p.ws_bytes == search_workspace_bytes(SEARCH_SIGN, q.G, q.n_records, q.k), "workspace");
    need(q.n_bits * ((1ll << p.Q) - 1) < (1ll << 31), "int32");
    return bad;
}

int main() {
    long long n = 0, bad = 0;
    std::set<std::string> seen;
    auto status_name = [](int s) { return s == GSW_ERR_BAD_ARG ? "bad_arg" : s == GSW_ERR_RAGGED ? "ragged" : "unsupported"; };
    const int64_t bits[] = {0, 7, 8, 12, 120, 256, 504, 512, 1920, 4096, 16384, 65536, 95320, 95328, 131072, 349520, 524288, 524296, 1048576, 2097152, 1ll << 40};
    // ---- pooling
    const int Bs[] = {0, 1, 2, 3, 5, 68, 69, 146, 147, 1023, 1024, 4096, 100000};
    const int sets[] = {0, 1, 2, 3, 5, 68, 69, 146, 147, 341, 342, 1023, 1024, 5000};
    for (int64_t nb : bits)
        for (int P = -1; P <= 5; ++P)
            for (int B : Bs)
                for (int G : {0, 1, 2, 3, 17, 4096, 100000})
                    for (int ms : sets)
                        for (int Q = 0; Q <= 11; ++Q)
                            for (int al = 0; al < 2; ++al) {
                                PoolQuery q{};
                                q.kind = POOL_ROWS; q.pointers_ok = true; q.rows_aligned = al; q.P = P; q.B = B; q.G = G; q.max_set = ms; q.Q = Q; q.n_bits = nb;
                                const PoolPlan p = pool_decide(q);
                                ++n;
                                const int want = expected_rows(true, P, B, G, ms, Q, nb);
                                if (p.status != want || (want != GSW_OK && !decided_nothing(p))) {
                                    printf("status\trows\tn=%lld\tP=%d\tB=%d\tG=%d\tmax_set=%d\tQ=%d\tstatus=%d\twant=%d\n", (long long)nb, P, B, G, ms, Q, p.status, want);
                                    ++bad;
                                    continue;
                                }
                                if (want != GSW_OK) { seen.insert(std::string("rows_") + status_name(want)); continue; }
                                seen.insert("rows_wg" + std::to_string(p.wg));
                                seen.insert("rows_q" + std::to_string(p.Q));
                                if (p.rows_aligned) seen.insert("rows_dwords"); else seen.insert("rows_bytes");
                                const std::string b = broken_rows(q, p);
                                if (!b.empty()) { printf("%s\trows\tn=%lld\tP=%d\tB=%d\tG=%d\tmax_set=%d\tQ=%d\n", b.c_str(), (long long)nb, P, B, G, ms, Q); ++bad; }
                            }
    // ---- the search
    for (int64_t nb : bits)
        for (int Q = 0; Q <= 11; ++Q)
            for (int G : {0, 1, 2, 4, 5, 16, 17, 300, 65535, 65536})
                for (int mb : {0, 1, 3, 4, 5, 8, 32, 256, 257})
                    for (int64_t U : {(int64_t)0, (int64_t)1, (int64_t)5, (int64_t)37, (int64_t)1000, (int64_t)4096, (int64_t)4097, (int64_t)1 << 20, (int64_t)2147483647, (int64_t)1 << 31})
                        for (int k : {0, 1, 3, 8, 9})
                            for (int64_t stride : {(int64_t)0, (int64_t)48, (int64_t)64, (int64_t)72, (int64_t)80, (int64_t)304, (int64_t)320})
                                for (int al = 0; al < 2; ++al) {
                                    PoolQuery q{};
                                    q.kind = POOL_SEARCH; q.pointers_ok = true; q.rows_aligned = al; q.records_present = true; q.records_aligned = true;
                                    q.G = G; q.Q = Q; q.n_bits = nb; q.record_stride = stride; q.n_records = U; q.msg_bytes = mb; q.k = k;
                                    const PoolPlan p = pool_decide(q);
                                    ++n;
                                    const int want = expected_search(true, true, true, G, Q, nb, stride, mb, U, k);
                                    if (p.status != want || (want != GSW_OK && !decided_nothing(p))) {
                                        printf("status\tsearch\tn=%lld\tQ=%d\tG=%d\tmb=%d\tU=%lld\tk=%d\tstride=%lld\tstatus=%d\twant=%d\n", (long long)nb, Q, G, mb, (long long)U, k,
                                               (long long)stride, p.status, want);
                                        ++bad;
                                        continue;
                                    }
                                    if (want != GSW_OK) { seen.insert(std::string("search_") + status_name(want)); continue; }
                                    seen.insert("search_t" + std::to_string(p.T));
                                    seen.insert("search_q" + std::to_string(p.Q));
                                    seen.insert(p.msg4 ? "search_msg4" : "search_msg_bytes");
                                    if (p.lds == CAP) seen.insert("search_lds_at_cap");
                                    if (G > 4 && p.T < 16) seen.insert("search_tile_cut_by_lds");
                                    const std::string b = broken_search(q, p);
                                    if (!b.empty()) { printf("%s\tsearch\tn=%lld\tQ=%d\tG=%d\tmb=%d\tU=%lld\tk=%d\n", b.c_str(), (long long)nb, Q, G, mb, (long long)U, k); ++bad; }
                                }
    // ---- every refusal precedes a launch, in the stated order when an input breaks several
    struct RowsCase { const char* name; bool ptr; int P, B, G, ms, Q; int64_t n; int status; };
    const RowsCase rows[] = {
        {"pointers", false, 0, 3, 1, 3, 2, 64, GSW_ERR_BAD_ARG},
        {"p_negative", true, -1, 3, 1, 3, 2, 64, GSW_ERR_BAD_ARG},
        {"p_five", true, 5, 3, 1, 3, 7, 64, GSW_ERR_BAD_ARG},
        {"b_zero", true, 0, 0, 1, 1, 1, 64, GSW_ERR_BAD_ARG},
        {"g_zero", true, 0, 3, 0, 3, 2, 64, GSW_ERR_BAD_ARG},
        {"more_sets_than_images", true, 0, 3, 4, 1, 1, 64, GSW_ERR_BAD_ARG},
        {"set_larger_than_batch", true, 0, 3, 1, 4, 3, 64, GSW_ERR_BAD_ARG},
        {"bits_not_bytes", true, 0, 3, 1, 3, 2, 60, GSW_ERR_BAD_ARG},
        {"q_zero", true, 0, 3, 1, 3, 0, 64, GSW_ERR_BAD_ARG},
        {"q_below_the_sets", true, 4, 5, 1, 5, 6, 64, GSW_ERR_BAD_ARG},                  // 15 x 5 = 75 needs 7 planes
        {"ok/q_holds_the_sets", true, 4, 5, 1, 5, 7, 64, GSW_OK},
        {"ok/q_above_the_sets", true, 4, 5, 1, 5, 10, 64, GSW_OK},
        {"69_images_at_15_levels", true, 4, 69, 1, 69, 10, 256, GSW_ERR_UNSUPPORTED},
        {"69_images_at_15_levels_q11", true, 4, 69, 1, 69, 11, 256, GSW_ERR_UNSUPPORTED},
        {"ok/68_images_at_15_levels", true, 4, 68, 1, 68, 10, 256, GSW_OK},
        {"1024_images", true, 0, 1024, 1, 1024, 10, 64, GSW_ERR_UNSUPPORTED},
        {"ok/1023_images", true, 0, 1023, 1, 1023, 10, 64, GSW_OK},
        {"q_eleven", true, 0, 3, 1, 3, 11, 64, GSW_ERR_UNSUPPORTED},
        {"past_domain", true, 0, 1, 1, 1, 1, 524296, GSW_ERR_UNSUPPORTED},
        {"ok/top_of_domain", true, 0, 1, 1, 1, 1, 524288, GSW_OK},
        {"past_domain_q10", true, 4, 68, 1, 68, 10, 95328, GSW_ERR_UNSUPPORTED},
        {"ok/top_of_domain_q10", true, 4, 68, 1, 68, 10, 95320, GSW_OK},
        {"order/bad_arg_before_unsupported", true, 5, 2000, 1, 2000, 11, 2097152, GSW_ERR_BAD_ARG},
    };
    for (const RowsCase& c : rows) {
        PoolQuery q{};
        q.kind = POOL_ROWS; q.pointers_ok = c.ptr; q.rows_aligned = true; q.P = c.P; q.B = c.B; q.G = c.G; q.max_set = c.ms; q.Q = c.Q; q.n_bits = c.n;
        const PoolPlan p = pool_decide(q);
        ++n;
        if (p.status != c.status || (c.status != GSW_OK && !decided_nothing(p)) || (c.status == GSW_OK && !broken_rows(q, p).empty())) {
            printf("refusal\trows\t%s\tstatus=%d\n", c.name, p.status);
            ++bad;
        }
    }
    struct SearchCase { const char* name; bool ptr, rec, rec16; int G, Q; int64_t n, stride; int mb; int64_t U; int k; int status; };
    const SearchCase search[] = {
        {"pointers", false, true, true, 3, 5, 256, 80, 32, 10, 1, GSW_ERR_BAD_ARG},
        {"records_null", true, false, true, 3, 5, 256, 80, 32, 10, 1, GSW_ERR_BAD_ARG},
        {"records_misaligned", true, true, false, 3, 5, 256, 80, 32, 10, 1, GSW_ERR_BAD_ARG},
        {"g_zero", true, true, true, 0, 5, 256, 80, 32, 10, 1, GSW_ERR_BAD_ARG},
        {"q_zero", true, true, true, 3, 0, 256, 80, 32, 10, 1, GSW_ERR_BAD_ARG},
        {"k_nine", true, true, true, 3, 5, 256, 80, 32, 10, 9, GSW_ERR_BAD_ARG},
        {"no_records", true, true, true, 3, 5, 256, 80, 32, 0, 1, GSW_ERR_BAD_ARG},
        {"stride_short", true, true, true, 3, 5, 256, 64, 32, 10, 1, GSW_ERR_BAD_ARG},
        {"stride_odd", true, true, true, 3, 5, 256, 88, 32, 10, 1, GSW_ERR_BAD_ARG},
        {"ragged", true, true, true, 3, 5, 264, 80, 32, 10, 1, GSW_ERR_RAGGED},
        {"q_eleven", true, true, true, 3, 11, 256, 80, 32, 10, 1, GSW_ERR_UNSUPPORTED},
        {"past_domain", true, true, true, 3, 10, 95488, 80, 32, 10, 1, GSW_ERR_UNSUPPORTED},
        {"past_int32", true, true, true, 3, 1, 1ll << 31, 80, 32, 10, 1, GSW_ERR_UNSUPPORTED},
        {"g_65536", true, true, true, 65536, 5, 256, 80, 32, 10, 1, GSW_ERR_UNSUPPORTED},
        {"padded_rows_past_the_tile", true, true, true, 1, 10, 95320, 64, 5, 10, 1, GSW_ERR_UNSUPPORTED},   // 11915 bytes pad to 11968: 11 rows are 131 648 bytes
        {"order/bad_arg_before_ragged", true, true, true, 3, 0, 264, 80, 32, 10, 1, GSW_ERR_BAD_ARG},
        {"order/ragged_before_unsupported", true, true, true, 65536, 11, 264, 80, 32, 10, 1, GSW_ERR_RAGGED},
        {"ok/q10_one_set", true, true, true, 1, 10, 16384, 80, 32, 1 << 20, 8, GSW_OK},
        {"ok/q10_4x64x64_tile4", true, true, true, 5, 10, 16384, 80, 32, 1000, 1, GSW_OK},
        {"ok/top_of_domain", true, true, true, 1, 1, 524288, 80, 32, 5, 1, GSW_OK},
        {"ok/g_65535", true, true, true, 65535, 1, 256, 80, 32, 5, 1, GSW_OK},
    };
    for (const SearchCase& c : search) {
        PoolQuery q{};
        q.kind = POOL_SEARCH; q.pointers_ok = c.ptr; q.rows_aligned = true; q.records_present = c.rec; q.records_aligned = c.rec16;
        q.G = c.G; q.Q = c.Q; q.n_bits = c.n; q.record_stride = c.stride; q.n_records = c.U; q.msg_bytes = c.mb; q.k = c.k;
        const PoolPlan p = pool_decide(q);
        ++n;
        if (p.status != c.status || (c.status != GSW_OK && !decided_nothing(p)) || (c.status == GSW_OK && !broken_search(q, p).empty())) {
            printf("refusal\tsearch\t%s\tstatus=%d\n", c.name, p.status);
            ++bad;
        }
    }
    std::string classes;
    for (const auto& s : seen) classes += " " + s;
    fprintf(stderr, "%lld inputs, %lld broken,%s\n", n, bad, classes.c_str());
    return 0;
}
