// key_search_soft_plan_cases.cpp -- walks a grid of inputs of key_soft_decide (csrc/gswm_keysearch_soft_plan.h) and prints every input whose decision breaks an
// invariant of a launch that no kernel checks, then every refusal case whose status or (all-zero) decision is not the expected one.  Host code only:
// tests/test_key_search_soft_plan_host.py builds it with the library's compiler; built with -fsanitize=address,undefined it is the sanitizer run of the policy.
//   key_search_soft_plan_cases            stdout: one line per broken input; stderr: "<inputs> inputs, <broken> broken, <classes seen>"
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "gswm_keysearch_soft_plan.h"

static KeySoftQuery query(int B, int P, int64_t n_bits, int msg_bytes, int64_t stride, int64_t n_keys, int k, bool rows_aligned = true) {
    return KeySoftQuery{B, P, n_bits, stride, n_keys, msg_bytes, k, rows_aligned, rows_aligned, true, false, false, false, false};
}

// the kernels gswm_keysearch_soft.inc instantiates: (cp, P, sg)
static bool instantiated(int cp, int P, bool sg) {
    if (cp == 0) return true;                                              // the bit-by-bit path takes P at run time
    if (cp == 4) return !sg;
    if (cp == 18) return P == 4;
    return cp == 8 || cp == 12 || cp == 16;
}

static std::string broken(const KeySoftQuery& q, const KeySoftPlan& p) {
    std::string bad;
    auto need = [&](bool ok, const char* name) { if (!ok) bad += std::string(bad.empty() ? "" : ",") + name; };
    const int64_t rowwords = (int64_t)p.nblk * 16, amax = (int64_t)((1 << q.P) - 1) * p.copies;
    const int64_t W = q.msg_bytes / 4;
    need(p.lds <= 131072u, "lds<=131072");
    need(p.lds >= (uint32_t)(KS_WG / p.G) * SEARCH_LIST * 8u, "lds>=tail");
    need(p.T == 1 || p.T == 4 || p.T == 16 || p.T == 64, "T");
    need((int64_t)p.grid_y * p.T >= q.B && p.grid_y >= 1 && p.grid_y <= 65535, "grid_y");
    need(p.grid_x >= 1 && p.grid_x <= search_grid_cap(SEARCH_KEY, q.n_keys), "grid_x");
    need(p.ws_bytes == (size_t)q.B * (size_t)search_grid_cap(SEARCH_KEY, q.n_keys) * (size_t)q.k * 8u, "ws");
    need((size_t)q.B * (size_t)p.grid_x * (size_t)q.k * 8u <= p.ws_bytes, "grid<=ws");
    need(p.rowbytes * 8ll == q.n_bits && p.nblk == (p.rowbytes + 63) / 64, "row");
    need(p.wg == KS_WG && p.G >= 1 && p.G <= 64 && (p.G & (p.G - 1)) == 0, "G");
    need(p.kpi >= 1, "kpi>=1");
    need((int64_t)p.G * p.T * p.kpi <= KS_WG, "G*T*kpi<=256");
    need((int64_t)p.copies * 8 * q.msg_bytes == q.n_bits, "copies");
    need(instantiated(p.cp, q.P, p.sg), "instantiated");
    if (p.cp > 0) {
        need(q.msg_bytes % 4 == 0 && (!p.sg || p.rows_aligned) && p.cp >= q.P && amax < (1ll << p.cp), "cp");
        need(p.nb >= 1 && p.nb <= p.cp && (amax >> p.nb) == 0 && (amax >> (p.nb - 1)) != 0, "nb");
        need(p.w_off % 4 == 0 && (int64_t)p.w_off + (int64_t)p.T * p.nb * W * 4 <= (int64_t)p.lds, "W_t<=lds");
    } else {
        need(p.nb == 0, "nb");
    }
    need(p.ks_off % 4 == 0 && (int64_t)p.ks_off + (int64_t)p.kpi * rowwords * 4 <= (int64_t)p.w_off && p.w_off <= p.lds, "keystreams<=W_t");
    if (p.sg) {
        need(p.T == 1 && p.ks_off == 0, "sg");
    } else {
        need(p.istride >= (1 + q.P) * rowwords && (int64_t)p.T * p.istride * 4 <= (int64_t)p.ks_off, "rows<=keystreams");
    }
    return bad;
}

int main() {
    const int Bs[] = {1, 2, 3, 4, 5, 16, 17, 64, 65, 4096, 65535};
    const int mbs[] = {1, 3, 4, 5, 8, 12, 16, 31, 32, 64, 100, 128, 255, 256};
    const int64_t Ks[] = {1, 2, 3, 7, 64, 255, 256, 257, 512, 513, 4097, 1000003, 2147483647};
    long long n = 0, bad = 0;
    std::set<int> classes;
    bool seen_sg[2] = {false, false};
    for (int P = 1; P <= 4; ++P)
        for (int mb : mbs) {
            // copies: small ones, the boundaries of every counter class of this P, the tile and SG edges of this message length (both sides), the domain's edge
            std::vector<int64_t> copies = {1, 2, 3, 4, 5, 17, 64, 256};
            for (int64_t top : {16, 256, 4096, 65536})
                for (int64_t d = -1; d <= 1; ++d) copies.push_back((top + ((1 << P) - 2)) / ((1 << P) - 1) + d);
            for (int64_t edge : {1024, 4096, 16384, 65536, 131072})
                for (int64_t div : {1 + P, 2 + P, 3 + P})
                    for (int64_t d = -2; d <= 2; ++d) copies.push_back(edge / div / mb + d);
            for (int64_t c : copies) {
                if (c < 1) continue;
                const int64_t n_bits = c * 8 * mb;
                for (int B : Bs)
                    for (int64_t K : Ks)
                        for (int k : {1, 8})
                            for (bool aligned : {true, false}) {
                                const KeySoftQuery q = query(B, P, n_bits, mb, 48, K, k, aligned);
                                const KeySoftPlan p = key_soft_decide(q);
                                ++n;
                                if (p.status != GSW_OK) {
                                    if (p.status != GSW_ERR_UNSUPPORTED || n_bits * (1 + P) <= GSW_ROW_MAX_BITS) { printf("refused\tP=%d\tB=%d\tn_bits=%lld\tmsg_bytes=%d\n", P, B, (long long)n_bits, mb); ++bad; }
                                    continue;
                                }
                                classes.insert(p.cp);
                                seen_sg[p.sg] = true;
                                const std::string b = broken(q, p);
                                if (!b.empty()) { printf("%s\tP=%d\tB=%d\tn_bits=%lld\tmsg_bytes=%d\tn_keys=%lld\tk=%d\taligned=%d\tlds=%u\n", b.c_str(), P, B, (long long)n_bits, mb, (long long)K, k, (int)aligned, p.lds); ++bad; }
                            }
            }
        }
    // ---- every refusal precedes a launch: the status, and a decision of zeros (no grid, no LDS, no workspace)
    struct Refusal { const char* name; KeySoftQuery q; int status; };
    auto with = [](KeySoftQuery q, auto change) { change(q); return q; };
    const KeySoftQuery ok = query(3, 2, 4096, 8, 48, 10, 2);
    const Refusal refusals[] = {
        {"signs_null", with(ok, [](KeySoftQuery& q) { q.signs_null = true; }), GSW_ERR_BAD_ARG},
        {"planes_null", with(ok, [](KeySoftQuery& q) { q.planes_null = true; }), GSW_ERR_BAD_ARG},
        {"keys_null", with(ok, [](KeySoftQuery& q) { q.keys_null = true; }), GSW_ERR_BAD_ARG},
        {"outputs_null", with(ok, [](KeySoftQuery& q) { q.outputs_null = true; }), GSW_ERR_BAD_ARG},
        {"b_zero", with(ok, [](KeySoftQuery& q) { q.B = 0; }), GSW_ERR_BAD_ARG},
        {"k_zero", with(ok, [](KeySoftQuery& q) { q.k = 0; }), GSW_ERR_BAD_ARG},
        {"k_nine", with(ok, [](KeySoftQuery& q) { q.k = 9; }), GSW_ERR_BAD_ARG},
        {"n_bits_zero", with(ok, [](KeySoftQuery& q) { q.n_bits = 0; }), GSW_ERR_BAD_ARG},
        {"keys_zero", with(ok, [](KeySoftQuery& q) { q.n_keys = 0; }), GSW_ERR_BAD_ARG},
        {"keys_2p31", with(ok, [](KeySoftQuery& q) { q.n_keys = 2147483648ll; }), GSW_ERR_BAD_ARG},
        {"p_zero", with(ok, [](KeySoftQuery& q) { q.P = 0; }), GSW_ERR_BAD_ARG},
        {"p_five", with(ok, [](KeySoftQuery& q) { q.P = 5; }), GSW_ERR_BAD_ARG},
        {"msg_bytes_zero", with(ok, [](KeySoftQuery& q) { q.msg_bytes = 0; }), GSW_ERR_BAD_ARG},
        {"msg_bytes_257", with(ok, [](KeySoftQuery& q) { q.msg_bytes = 257; }), GSW_ERR_BAD_ARG},
        {"stride_short", with(ok, [](KeySoftQuery& q) { q.key_stride = 32; }), GSW_ERR_BAD_ARG},
        {"stride_not_16", with(ok, [](KeySoftQuery& q) { q.key_stride = 56; }), GSW_ERR_BAD_ARG},
        {"keys_misaligned", with(ok, [](KeySoftQuery& q) { q.keys_aligned = false; }), GSW_ERR_BAD_ARG},
        {"ragged", with(ok, [](KeySoftQuery& q) { q.n_bits = 4104; }), GSW_ERR_RAGGED},
        {"past_domain", with(ok, [](KeySoftQuery& q) { q.n_bits = 349568; }), GSW_ERR_UNSUPPORTED},
        {"b_65536", with(ok, [](KeySoftQuery& q) { q.B = 65536; }), GSW_ERR_UNSUPPORTED},
        {"order/bad_arg_before_ragged", with(ok, [](KeySoftQuery& q) { q.n_bits = 4104; q.k = 9; }), GSW_ERR_BAD_ARG},
        {"order/ragged_before_unsupported", with(ok, [](KeySoftQuery& q) { q.n_bits = 2097160; }), GSW_ERR_RAGGED},
        {"ok/rows_misaligned", with(ok, [](KeySoftQuery& q) { q.signs_aligned = false; }), GSW_OK},
        {"ok/at_domain", with(ok, [](KeySoftQuery& q) { q.n_bits = 349504; }), GSW_OK},
    };
    for (const Refusal& r : refusals) {
        const KeySoftPlan p = key_soft_decide(r.q);
        ++n;
        const bool decided_nothing = p.T == 0 && p.cp == 0 && p.nb == 0 && !p.sg && p.G == 0 && p.kpi == 0 && p.istride == 0 && p.copies == 0 && p.rowbytes == 0 && p.nblk == 0 &&
                                     p.rows_aligned == 0 && p.grid_x == 0 && p.grid_y == 0 && p.wg == 0 && p.ks_off == 0 && p.w_off == 0 && p.lds == 0 && p.ws_bytes == 0;
        if (p.status != r.status || (r.status != GSW_OK && !decided_nothing) || (r.status == GSW_OK && !broken(r.q, p).empty())) { printf("refusal\t%s\tstatus=%d\n", r.name, p.status); ++bad; }
    }
    std::string seen;
    for (int c : classes) seen += " cp" + std::to_string(c);
    fprintf(stderr, "%lld inputs, %lld broken,%s%s%s\n", n, bad, seen.c_str(), seen_sg[0] ? " lds" : "", seen_sg[1] ? " sg" : "");
    return 0;
}
