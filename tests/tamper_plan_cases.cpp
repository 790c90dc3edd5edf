// tamper_plan_cases.cpp -- walks a grid of inputs of the three decisions of csrc/gswm_tamper_plan.h (tile_decide for the map and for the vote, robust_decide)
// and prints every input whose decision breaks an invariant of a launch that no kernel checks, every refusal whose status or (all-zero) decision is not the
// expected one, and every value at which robust_isqrt is not the exact floor square root.  Host code only: tests/test_tamper_plan_host.py builds it with the
// library's compiler; built with -fsanitize=address,undefined it is the sanitizer run of the policy.
//   tamper_plan_cases            stdout: one line per broken input; stderr: "<inputs> inputs, <broken> broken, <roots> roots, <classes seen>"
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "gswm_tamper_plan.h"

static RobustQuery query(int P, int B, int C, int h, int w, int l, int tile, int msg_bits, int iters, int sign_rounds) {
    return RobustQuery{P, B, C, h, w, l, tile, msg_bits, iters, sign_rounds, true, true, true, false, false, false, false};
}

static TileQuery tile_query(int B, int C, int h, int w, int l, int tile, int msg_bits) {
    return TileQuery{B, C, h, w, l, tile, msg_bits, false, true, false, false, true, true};
}

// the geometry is the lattice's: appends what is not to `bad`
static void geometry(std::string& bad, const TileGeom& g, int C, int h, int w, int l, int tile, int msg_bits) {
    auto need = [&](bool ok, const char* name) { if (!ok) bad += std::string(bad.empty() ? "" : ",") + name; };
    const int64_t nb = (int64_t)C * h * w * l;
    need(g.C == C && g.h == h && g.w == w && g.msg_bits == msg_bits, "lattice");
    need((1 << g.log2l) == l && (1 << g.log2t) == tile, "log2");
    need(g.tw == w / tile && g.tiles == (h / tile) * (w / tile) && g.tiles >= 1, "tiles");
    need(g.n_t == (int64_t)C * tile * tile * l, "n_t");
    need(g.rowbytes * 8ll == nb && g.rowbytes % 8 == 0 && g.nblk == (g.rowbytes + 63) / 64, "row");
    need(g.msg_bytes * 8 == msg_bits && (int64_t)g.copies * msg_bits == nb, "copies");
    need(g.log2s >= 0 && g.log2s <= 3 && (1 << g.log2s) <= g.copies && ((64 >> g.log2s) % 8) == 0, "log2s");
}

static std::string broken(const RobustQuery& q, const RobustPlan& p) {
    std::string bad;
    auto need = [&](bool ok, const char* name) { if (!ok) bad += std::string(bad.empty() ? "" : ",") + name; };
    const int64_t nb = (int64_t)q.C * q.h * q.w * q.l;
    const int64_t lmax = q.P > 0 ? (1 << q.P) - 1 : 1, n_t = (int64_t)q.C * q.tile * q.tile * q.l;
    need(p.lds <= 131072u, "lds<=131072");
    geometry(bad, p.g, q.C, q.h, q.w, q.l, q.tile, q.msg_bits);
    need(p.lmax == lmax, "lmax");
    need(p.grid == q.B && p.wg == TM_WG, "grid");
    need(p.level_rounds == (q.P > 0 && q.iters >= q.sign_rounds ? 1 : 0), "level_rounds");
    // the regions are disjoint and in order: row | planes | wgt | wtot | wsq | msg | end
    const int64_t tile_bytes = 4ll * p.g.tiles, shared = p.level_rounds ? tile_bytes : 0;
    need((int64_t)p.planes_off == 64ll * p.g.nblk && (int64_t)p.planes_off >= p.g.rowbytes, "row|planes");
    need((int64_t)p.wgt_off == (int64_t)p.planes_off + (int64_t)q.P * p.g.rowbytes, "planes|wgt");
    need((int64_t)p.wtot_off == (int64_t)p.wgt_off + tile_bytes, "wgt|wtot");
    need((int64_t)p.wsq_off == (int64_t)p.wtot_off + shared, "wtot|wsq");
    need((int64_t)p.msg_off == (int64_t)p.wsq_off + shared, "wsq|msg");
    need((int64_t)p.lds >= (int64_t)p.msg_off + p.g.msg_bytes && (int64_t)p.lds < (int64_t)p.msg_off + p.g.msg_bytes + 4, "msg|end");
    need(p.planes_off % 4 == 0 && p.wgt_off % 4 == 0 && p.wtot_off % 4 == 0 && p.wsq_off % 4 == 0 && p.msg_off % 4 == 0 && p.lds % 4 == 0, "aligned");
    // the int32 bound really holds: the largest weight, vote, score and sum of squares, computed in 64 bits
    const int64_t wmax = lmax * n_t, vote = lmax * wmax, score = (int64_t)p.g.copies * vote, wsq = lmax * lmax * n_t;
    need(wmax <= INT32_MAX && vote <= INT32_MAX && score <= INT32_MAX && wsq <= INT32_MAX && 2 * wmax <= INT32_MAX, "int32");
    need(nb * (1 + q.P) <= GSW_ROW_MAX_BITS, "domain");
    return bad;
}

// the map's or the vote's accepted decision: the row is all of its LDS, and a uint16 weight on every copy fits the vote's int32
static std::string broken(const TileQuery& q, const TilePlan& p, bool vote) {
    std::string bad;
    auto need = [&](bool ok, const char* name) { if (!ok) bad += std::string(bad.empty() ? "" : ",") + name; };
    geometry(bad, p.g, q.C, q.h, q.w, q.l, q.tile, q.msg_bits);
    need(p.lds == 64u * (uint32_t)p.g.nblk && p.lds <= 131072u && (int64_t)p.lds >= p.g.rowbytes, "lds==64nblk<=131072");
    need(p.grid == q.B && p.wg == TM_WG, "grid");
    need(!vote || (int64_t)p.g.copies * 65535 <= INT32_MAX, "int32");
    return bad;
}

static bool zero_geometry(const TileGeom& g) {
    const TileGeom zero{};
    return memcmp(&g, &zero, sizeof g) == 0;           // ints only: no padding
}

static bool decided_nothing(const RobustPlan& p) {
    return zero_geometry(p.g) && p.lmax == 0 && p.level_rounds == 0 && p.grid == 0 && p.wg == 0 && p.planes_off == 0 && p.wgt_off == 0 && p.wtot_off == 0 && p.wsq_off == 0 &&
           p.msg_off == 0 && p.lds == 0;
}

static bool decided_nothing(const TilePlan& p) { return zero_geometry(p.g) && p.grid == 0 && p.wg == 0 && p.lds == 0; }

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
    // what the refusal of an input must be, restated: the order is BAD_ARG (none in the grid), UNSUPPORTED (lattice), RAGGED, UNSUPPORTED (rounds; the vote's int32)
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
                                            int shared = GSW_OK;                       // the refusals the three decisions share
                                            const char* why = "ok";
                                            if (h % tile || w % tile) { shared = GSW_ERR_UNSUPPORTED; why = "lattice"; }
                                            else if (nb > GSW_ROW_MAX_BITS) { shared = GSW_ERR_UNSUPPORTED; why = "row"; }
                                            else if (nb % M) { shared = GSW_ERR_RAGGED; why = "ragged"; }
                                            if (P == 0 && iters == 0 && W == 0) {      // the map and the vote of the same lattice, once per (lattice, B)
                                                for (const bool vote : {false, true}) {
                                                    const TileQuery tq = tile_query(B, C, h, w, l, tile, M);
                                                    const TilePlan tp = tile_decide(tq, vote);
                                                    ++n;
                                                    int want = shared;
                                                    const char* twhy = why;
                                                    if (vote && shared == GSW_OK) {
                                                        if ((nb / M) * 65535 > (int64_t)INT32_MAX) { want = GSW_ERR_UNSUPPORTED; twhy = "vote_int32"; }
                                                        else if ((nb / M + 1) * 65535 > (int64_t)INT32_MAX) twhy = "vote_at_int32";          // accepted at the boundary: 32768 copies
                                                        if (twhy != why) seen.insert(twhy);
                                                    }
                                                    const char* name = vote ? "vote" : "map";
                                                    if (tp.status != want) { printf("%s status\t%s\twant=%d\tgot=%d\tC=%d h=%d w=%d l=%d tile=%d M=%d\n", name, twhy, want, tp.status, C, h, w, l, tile, M); ++bad; continue; }
                                                    if (tp.status != GSW_OK) {
                                                        if (!decided_nothing(tp)) { printf("%s refusal decides\t%s\tC=%d h=%d w=%d l=%d tile=%d M=%d\n", name, twhy, C, h, w, l, tile, M); ++bad; }
                                                        continue;
                                                    }
                                                    std::string b = broken(tq, tp, vote);
                                                    if (p.status == GSW_OK && memcmp(&tp.g, &p.g, sizeof tp.g) != 0) b += ",geometry!=robust";
                                                    if (!b.empty()) { printf("%s %s\tC=%d h=%d w=%d l=%d tile=%d M=%d lds=%u\n", name, b.c_str(), C, h, w, l, tile, M, tp.lds); ++bad; }
                                                }
                                            }
                                            int want = shared;
                                            if (shared != GSW_OK) {}                   // (decided above)
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
                                            seen.insert("s" + std::to_string(p.g.log2s));
                                            const std::string b = broken(q, p);
                                            if (!b.empty()) { printf("%s\tP=%d C=%d h=%d w=%d l=%d tile=%d M=%d I=%d W=%d lds=%u\n", b.c_str(), P, C, h, w, l, tile, M, iters, W, p.lds); ++bad; }
                                        }
    // ---- every refusal precedes a launch: the status, and a decision of zeros
    struct Refusal { const char* name; RobustQuery q; int status; };
    auto with = [](auto q, auto change) { change(q); return q; };
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
    // ---- the map's and the vote's: the statuses the C ABI returns for a 2 x (4, 16, 16) lattice, l = 1, tile 8, 64-bit messages, and the order when an input breaks
    // several rules: own pointers, packed / keys, sizes, l, alignment (BAD_ARG), tile, lattice or msg_bits % 8, row (UNSUPPORTED), RAGGED, the vote's int32 (UNSUPPORTED)
    struct TileRefusal { const char* name; TileQuery q; int map, vote; };
    const TileQuery tok = tile_query(2, 4, 16, 16, 1, 8, 64);
    const int BAD = GSW_ERR_BAD_ARG, UNS = GSW_ERR_UNSUPPORTED, RAG = GSW_ERR_RAGGED;
    const TileRefusal tile_refusals[] = {
        {"ok", tok, GSW_OK, GSW_OK},
        {"own_null", with(tok, [](TileQuery& q) { q.own_null = true; }), BAD, BAD},
        {"weights_misaligned", with(tok, [](TileQuery& q) { q.weights_aligned = false; }), GSW_OK, BAD},          // the map has no weights
        {"packed_null", with(tok, [](TileQuery& q) { q.packed_null = true; }), BAD, BAD},
        {"keys_null", with(tok, [](TileQuery& q) { q.keys_null = true; }), BAD, BAD},
        {"b_zero", with(tok, [](TileQuery& q) { q.B = 0; }), BAD, BAD},
        {"c_zero", with(tok, [](TileQuery& q) { q.C = 0; }), BAD, BAD},
        {"h_zero", with(tok, [](TileQuery& q) { q.h = 0; }), BAD, BAD},
        {"w_zero", with(tok, [](TileQuery& q) { q.w = 0; }), BAD, BAD},
        {"m_zero", with(tok, [](TileQuery& q) { q.msg_bits = 0; }), BAD, BAD},
        {"l_three", with(tok, [](TileQuery& q) { q.l = 3; }), BAD, BAD},
        {"l_zero", with(tok, [](TileQuery& q) { q.l = 0; }), BAD, BAD},
        {"packed_misaligned", with(tok, [](TileQuery& q) { q.packed_aligned = false; }), BAD, BAD},
        {"keys_misaligned", with(tok, [](TileQuery& q) { q.keys_aligned = false; }), BAD, BAD},
        {"tile_four", with(tok, [](TileQuery& q) { q.tile = 4; }), UNS, UNS},
        {"tile_64", with(tok, [](TileQuery& q) { q.tile = 64; }), UNS, UNS},
        {"h_not_tiles", with(tok, [](TileQuery& q) { q.h = 12; }), UNS, UNS},
        {"w_not_tiles", with(tok, [](TileQuery& q) { q.w = 20; }), UNS, UNS},
        {"m_not_bytes", with(tok, [](TileQuery& q) { q.msg_bits = 60; }), UNS, UNS},
        {"row_past_domain", with(tok, [](TileQuery& q) { q.h = 512; q.w = 520; }), UNS, UNS},                       // 1 064 960 bits > 1 048 576
        {"ragged", with(tok, [](TileQuery& q) { q.msg_bits = 384; }), RAG, RAG},
        {"vote_int32", with(tok, [](TileQuery& q) { q.h = 512; q.w = 512; q.msg_bits = 8; }), GSW_OK, UNS},         // 131 072 copies x 65535 does not fit int32
        {"ok/vote_at_int32", with(tok, [](TileQuery& q) { q.h = 256; q.w = 256; q.msg_bits = 8; }), GSW_OK, GSW_OK}, // 32 768 x 65535 = 2^31 - 32 768
        {"ok/full_row", with(tok, [](TileQuery& q) { q.h = 512; q.w = 512; q.tile = 32; q.msg_bits = 4096; }), GSW_OK, GSW_OK},   // the row alone is the 131 072-byte cap
        {"order/own_null_before_tile", with(tok, [](TileQuery& q) { q.own_null = true; q.tile = 4; }), BAD, BAD},
        {"order/packed_null_before_row", with(tok, [](TileQuery& q) { q.packed_null = true; q.h = 512; q.w = 520; }), BAD, BAD},
        {"order/sizes_before_tile", with(tok, [](TileQuery& q) { q.B = 0; q.tile = 4; }), BAD, BAD},
        {"order/l_before_tile", with(tok, [](TileQuery& q) { q.l = 3; q.tile = 4; }), BAD, BAD},
        {"order/l_before_ragged", with(tok, [](TileQuery& q) { q.l = 3; q.msg_bits = 384; }), BAD, BAD},
        {"order/alignment_before_tile", with(tok, [](TileQuery& q) { q.keys_aligned = false; q.tile = 64; }), BAD, BAD},
        {"order/alignment_before_ragged", with(tok, [](TileQuery& q) { q.packed_aligned = false; q.msg_bits = 384; }), BAD, BAD},
        {"order/tile_before_ragged", with(tok, [](TileQuery& q) { q.tile = 4; q.msg_bits = 384; }), UNS, UNS},
        {"order/lattice_before_ragged", with(tok, [](TileQuery& q) { q.h = 12; q.msg_bits = 384; }), UNS, UNS},
        {"order/row_before_ragged", with(tok, [](TileQuery& q) { q.h = 512; q.w = 520; q.msg_bits = 384; }), UNS, UNS},
        {"order/ragged_before_vote_int32", with(tok, [](TileQuery& q) { q.h = 512; q.w = 512; q.msg_bits = 24; }), RAG, RAG},   // 43 690 copies and a remainder
        {"order/weights_before_ragged", with(tok, [](TileQuery& q) { q.weights_aligned = false; q.msg_bits = 384; }), RAG, BAD},
    };
    for (const TileRefusal& r : tile_refusals)
        for (const bool vote : {false, true}) {
            const TilePlan p = tile_decide(r.q, vote);
            const int want = vote ? r.vote : r.map;
            ++n;
            if (p.status != want || (want != GSW_OK && !decided_nothing(p)) || (want == GSW_OK && !broken(r.q, p, vote).empty())) {
                printf("%s refusal\t%s\tstatus=%d want=%d\t%s\n", vote ? "vote" : "map", r.name, p.status, want, want == GSW_OK && p.status == GSW_OK ? broken(r.q, p, vote).c_str() : "");
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
