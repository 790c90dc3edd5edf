// robust_plan_cases.cpp -- walks a grid of inputs of robust_decide (csrc/gswm_robust_plan.h) and prints every input whose decision breaks an invariant of a
// launch that no kernel checks, every refusal whose status or (all-zero) decision is not the expected one, and every value at which robust_isqrt is not the
// exact floor square root.  Host code only: tests/test_robust_plan_host.py builds it with the library's compiler; built with -fsanitize=address,undefined it is
// the sanitizer run of the policy.
//   robust_plan_cases            stdout: one line per broken input; stderr: "<inputs> inputs, <broken> broken, <classes seen>"
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "gswm_robust_plan.h"

static RobustQuery query(int P, int B, int C, int h, int w, int l, int tile, int msg_bits, int iters, int sign_rounds) {
    return RobustQuery{P, B, C, h, w, l, tile, msg_bits, iters, sign_rounds, true, true, true, false, false, false, false};
}

static std::string broken(const RobustQuery& q, const RobustPlan& p) {
    std::string bad;
    auto need = [&](bool ok, const char* name) { if (!ok) bad += std::string(bad.empty() ? "" : ",") + name; };
    const int64_t nb = (int64_t)q.C * q.h * q.w * q.l;
    const int64_t lmax = q.P > 0 ? (1 << q.P) - 1 : 1, n_t = (int64_t)q.C * q.tile * q.tile * q.l;
    need(p.lds <= 131072u, "lds<=131072");
    need((1 << p.log2l) == q.l && (1 << p.log2t) == q.tile, "log2");
    need(p.tw == q.w / q.tile && p.tiles == (q.h / q.tile) * (q.w / q.tile) && p.tiles >= 1, "tiles");
    need(p.n_t == n_t && p.lmax == lmax, "n_t");
    need(p.rowbytes * 8ll == nb && p.rowbytes % 8 == 0 && p.nblk == (p.rowbytes + 63) / 64, "row");
    need(p.msg_bytes * 8 == q.msg_bits && (int64_t)p.copies * q.msg_bits == nb, "copies");
    need(p.log2s >= 0 && p.log2s <= 3 && (1 << p.log2s) <= p.copies && ((64 >> p.log2s) % 8) == 0, "log2s");
    need(p.grid == q.B && p.wg == RB_WG, "grid");
    need(p.level_rounds == (q.P > 0 && q.iters >= q.sign_rounds ? 1 : 0), "level_rounds");
    // the regions are disjoint and in order: row | planes | wgt | wtot | wsq | msg | end
    const int64_t tile_bytes = 4ll * p.tiles, shared = p.level_rounds ? tile_bytes : 0;
    need((int64_t)p.planes_off == 64ll * p.nblk && (int64_t)p.planes_off >= p.rowbytes, "row|planes");
    need((int64_t)p.wgt_off == (int64_t)p.planes_off + (int64_t)q.P * p.rowbytes, "planes|wgt");
    need((int64_t)p.wtot_off == (int64_t)p.wgt_off + tile_bytes, "wgt|wtot");
    need((int64_t)p.wsq_off == (int64_t)p.wtot_off + shared, "wtot|wsq");
    need((int64_t)p.msg_off == (int64_t)p.wsq_off + shared, "wsq|msg");
    need((int64_t)p.lds >= (int64_t)p.msg_off + p.msg_bytes && (int64_t)p.lds < (int64_t)p.msg_off + p.msg_bytes + 4, "msg|end");
    need(p.planes_off % 4 == 0 && p.wgt_off % 4 == 0 && p.wtot_off % 4 == 0 && p.wsq_off % 4 == 0 && p.msg_off % 4 == 0 && p.lds % 4 == 0, "aligned");
    // the int32 bound really holds: the largest weight, vote, score and sum of squares, computed in 64 bits
    const int64_t wmax = lmax * n_t, vote = lmax * wmax, score = (int64_t)p.copies * vote, wsq = lmax * lmax * n_t;
    need(wmax <= INT32_MAX && vote <= INT32_MAX && score <= INT32_MAX && wsq <= INT32_MAX && 2 * wmax <= INT32_MAX, "int32");
    need(nb * (1 + q.P) <= GSW_ROW_MAX_BITS, "domain");
    return bad;
}

static bool decided_nothing(const RobustPlan& p) {
    return p.log2l == 0 && p.log2t == 0 && p.tw == 0 && p.tiles == 0 && p.n_t == 0 && p.lmax == 0 && p.rowbytes == 0 && p.nblk == 0 && p.msg_bytes == 0 && p.copies == 0 &&
           p.log2s == 0 && p.level_rounds == 0 && p.grid == 0 && p.wg == 0 && p.planes_off == 0 && p.wgt_off == 0 && p.wtot_off == 0 && p.wsq_off == 0 && p.msg_off == 0 &&
           p.lds == 0;
}

static long long check_isqrt(uint32_t v, long long& n) {
    const uint64_t r = robust_isqrt(v);
    ++n;
    if (r * r <= (uint64_t)v && (uint64_t)v < (r + 1) * (r + 1)) return 0;
    printf("isqrt\tv=%u\tr=%llu\n", v, (unsigned long long)r);
    return 1;
}

int main() {
    long long n = 0, bad = 0;
    std::set<std::string> seen;
    // what the refusal of an input must be, restated: the order is BAD_ARG (none in the grid), UNSUPPORTED (lattice), RAGGED, UNSUPPORTED (rounds)
    const int Cs[] = {1, 3, 4, 16, 64, 320, 4096}, hs[] = {8, 16, 24, 32, 64, 96, 128, 256, 512, 1024}, ls[] = {1, 2, 4}, tiles[] = {8, 16, 32};
    const int Ms[] = {8, 24, 32, 64, 128, 256, 1024, 2048, 4096, 65536, 1048576};
    for (int P = 0; P <= 4; ++P)
        for (int C : Cs)
            for (int h : hs)
                for (int w : {h, 8, 3 * h / 2})
                    for (int l : ls)
                        for (int tile : tiles)
                            for (int M : Ms)
                                for (int iters : {0, 1, 8})
                                    for (int W : {0, 1})
                                        for (int B : {1, 3, 65536}) {
                                            const RobustQuery q = query(P, B, C, h, w, l, tile, M, iters, W);
                                            const RobustPlan p = robust_decide(q);
                                            ++n;
                                            const int64_t nb = (int64_t)C * h * w * l, lmax = P > 0 ? (1 << P) - 1 : 1, n_t = (int64_t)C * tile * tile * l;
                                            int want = GSW_OK;
                                            const char* why = "ok";
                                            if (h % tile || w % tile) { want = GSW_ERR_UNSUPPORTED; why = "lattice"; }
                                            else if (nb > GSW_ROW_MAX_BITS) { want = GSW_ERR_UNSUPPORTED; why = "row"; }
                                            else if (nb % M) { want = GSW_ERR_RAGGED; why = "ragged"; }
                                            else if (nb * (1 + P) > GSW_ROW_MAX_BITS) { want = GSW_ERR_UNSUPPORTED; why = "planes"; }
                                            else if ((nb / M) * lmax * lmax * n_t > (int64_t)INT32_MAX) { want = GSW_ERR_UNSUPPORTED; why = "int32"; }
                                            else {
                                                const int64_t rowbytes = nb / 8, tl = (int64_t)(h / tile) * (w / tile);
                                                const int64_t lds = (rowbytes + 63) / 64 * 64 + P * rowbytes + 4 * tl * ((P > 0 && iters >= W) ? 3 : 1) + (M / 8 + 3) / 4 * 4;
                                                if (lds > 131072) { want = GSW_ERR_UNSUPPORTED; why = "lds"; }
                                            }
                                            seen.insert(why);
                                            if (p.status != want) { printf("status\t%s\twant=%d\tgot=%d\tP=%d C=%d h=%d w=%d l=%d tile=%d M=%d I=%d W=%d\n", why, want, p.status, P, C, h, w, l, tile, M, iters, W); ++bad; continue; }
                                            if (p.status != GSW_OK) {
                                                if (!decided_nothing(p)) { printf("refusal decides\t%s\tP=%d C=%d h=%d w=%d l=%d tile=%d M=%d\n", why, P, C, h, w, l, tile, M); ++bad; }
                                                continue;
                                            }
                                            seen.insert("s" + std::to_string(p.log2s));
                                            const std::string b = broken(q, p);
                                            if (!b.empty()) { printf("%s\tP=%d C=%d h=%d w=%d l=%d tile=%d M=%d I=%d W=%d lds=%u\n", b.c_str(), P, C, h, w, l, tile, M, iters, W, p.lds); ++bad; }
                                        }
    // ---- every refusal precedes a launch: the status, and a decision of zeros
    struct Refusal { const char* name; RobustQuery q; int status; };
    auto with = [](RobustQuery q, auto change) { change(q); return q; };
    const RobustQuery ok = query(4, 3, 4, 64, 64, 1, 8, 256, 2, 1);
    const Refusal refusals[] = {
        {"signs_null", with(ok, [](RobustQuery& q) { q.signs_null = true; }), GSW_ERR_BAD_ARG},
        {"keys_null", with(ok, [](RobustQuery& q) { q.keys_null = true; }), GSW_ERR_BAD_ARG},
        {"outputs_null", with(ok, [](RobustQuery& q) { q.outputs_null = true; }), GSW_ERR_BAD_ARG},
        {"planes_null", with(ok, [](RobustQuery& q) { q.planes_null = true; }), GSW_ERR_BAD_ARG},
        {"planes_misaligned", with(ok, [](RobustQuery& q) { q.planes_aligned = false; }), GSW_ERR_BAD_ARG},
        {"signs_misaligned", with(ok, [](RobustQuery& q) { q.signs_aligned = false; }), GSW_ERR_BAD_ARG},
        {"keys_misaligned", with(ok, [](RobustQuery& q) { q.keys_aligned = false; }), GSW_ERR_BAD_ARG},
        {"p_minus", with(ok, [](RobustQuery& q) { q.P = -1; }), GSW_ERR_BAD_ARG},
        {"p_five", with(ok, [](RobustQuery& q) { q.P = 5; }), GSW_ERR_BAD_ARG},
        {"iters_minus", with(ok, [](RobustQuery& q) { q.iters = -1; }), GSW_ERR_BAD_ARG},
        {"iters_nine", with(ok, [](RobustQuery& q) { q.iters = 9; }), GSW_ERR_BAD_ARG},
        {"w_two", with(ok, [](RobustQuery& q) { q.sign_rounds = 2; }), GSW_ERR_BAD_ARG},
        {"w_minus", with(ok, [](RobustQuery& q) { q.sign_rounds = -1; }), GSW_ERR_BAD_ARG},
        {"b_zero", with(ok, [](RobustQuery& q) { q.B = 0; }), GSW_ERR_BAD_ARG},
        {"c_zero", with(ok, [](RobustQuery& q) { q.C = 0; }), GSW_ERR_BAD_ARG},
        {"h_zero", with(ok, [](RobustQuery& q) { q.h = 0; }), GSW_ERR_BAD_ARG},
        {"w_zero", with(ok, [](RobustQuery& q) { q.w = 0; }), GSW_ERR_BAD_ARG},
        {"m_zero", with(ok, [](RobustQuery& q) { q.msg_bits = 0; }), GSW_ERR_BAD_ARG},
        {"l_three", with(ok, [](RobustQuery& q) { q.l = 3; }), GSW_ERR_BAD_ARG},
        {"tile_four", with(ok, [](RobustQuery& q) { q.tile = 4; }), GSW_ERR_UNSUPPORTED},
        {"tile_64", with(ok, [](RobustQuery& q) { q.tile = 64; }), GSW_ERR_UNSUPPORTED},
        {"h_not_tiles", with(ok, [](RobustQuery& q) { q.h = 72; q.tile = 16; }), GSW_ERR_UNSUPPORTED},
        {"m_not_bytes", with(ok, [](RobustQuery& q) { q.msg_bits = 4; }), GSW_ERR_UNSUPPORTED},
        {"row_past_domain", with(ok, [](RobustQuery& q) { q.P = 0; q.C = 16; q.h = 512; q.w = 256; }), GSW_ERR_UNSUPPORTED},
        {"ragged", with(ok, [](RobustQuery& q) { q.msg_bits = 24; }), GSW_ERR_RAGGED},
        {"planes_past_domain", with(ok, [](RobustQuery& q) { q.C = 16; q.h = 128; q.w = 128; }), GSW_ERR_UNSUPPORTED},          // 262144 x 5
        {"int32", with(ok, [](RobustQuery& q) { q.C = 16; q.h = 64; q.w = 64; q.tile = 32; q.msg_bits = 8; }), GSW_ERR_UNSUPPORTED},   // 8192 x 225 x 16384
        {"lds", with(ok, [](RobustQuery& q) { q.P = 0; q.C = 1; q.h = 1024; q.w = 1024; q.msg_bits = 8192; }), GSW_ERR_UNSUPPORTED}, // 128 KiB of row + 64 KiB of weights
        {"order/bad_arg_before_unsupported", with(ok, [](RobustQuery& q) { q.tile = 4; q.iters = 9; }), GSW_ERR_BAD_ARG},
        {"order/lattice_before_ragged", with(ok, [](RobustQuery& q) { q.tile = 4; q.msg_bits = 24; }), GSW_ERR_UNSUPPORTED},
        {"order/ragged_before_planes", with(ok, [](RobustQuery& q) { q.C = 16; q.h = 128; q.w = 128; q.msg_bits = 24; }), GSW_ERR_RAGGED},
        {"ok/no_planes_pointer_without_planes", with(ok, [](RobustQuery& q) { q.P = 0; q.planes_null = true; q.planes_aligned = false; }), GSW_OK},
        {"ok/at_int32", with(ok, [](RobustQuery& q) { q.C = 1; q.h = 32; q.w = 32; q.tile = 32; q.msg_bits = 8; q.l = 4; }), GSW_OK},     // 512 x 225 x 4096 < 2^31
        {"ok/near_domain", with(ok, [](RobustQuery& q) { q.C = 3; q.h = 256; q.w = 256; q.tile = 32; }), GSW_OK},                       // 196608 x 5 = 983040 <= 2^20, 123 680 bytes of LDS
    };
    for (const Refusal& r : refusals) {
        const RobustPlan p = robust_decide(r.q);
        ++n;
        if (p.status != r.status || (r.status != GSW_OK && !decided_nothing(p)) || (r.status == GSW_OK && !broken(r.q, p).empty())) {
            printf("refusal\t%s\tstatus=%d\t%s\n", r.name, p.status, r.status == GSW_OK && p.status == GSW_OK ? broken(r.q, p).c_str() : "");
            ++bad;
        }
    }
    // ---- robust_isqrt is the exact floor square root
    long long roots = 0;
    for (uint32_t v = 0; v <= (1u << 24); ++v) bad += check_isqrt(v, roots);
    for (uint32_t v : {15u * 15u * 16384u - 1u, 15u * 15u * 16384u, 15u * 15u * 16384u + 1u, 0x7FFFFFFEu, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu}) bad += check_isqrt(v, roots);
    for (uint64_t r = 4096; r <= 65535; ++r) {                       // perfect squares past 2^24 and their neighbours
        const uint64_t s = r * r;
        bad += check_isqrt((uint32_t)(s - 1), roots);
        bad += check_isqrt((uint32_t)s, roots);
        if (s + 1 <= 0xFFFFFFFFull) bad += check_isqrt((uint32_t)(s + 1), roots);
    }
    std::string classes;
    for (const std::string& s : seen) classes += " " + s;
    fprintf(stderr, "%lld inputs, %lld broken, %lld roots,%s\n", n, bad, roots, classes.c_str());
    return 0;
}
