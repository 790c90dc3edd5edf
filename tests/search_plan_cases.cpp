// search_plan_cases.cpp -- prints what search_decide (csrc/gswm_search_plan.h) decides for every row of tests/golden/search_plan_cases.tsv, in the table's decision
// columns; with --sweep, walks a grid of inputs wider than the table and prints every input whose decision breaks an invariant of a launch.  Host code only:
// tests/test_search_plan_host.py builds it with the library's compiler; built with -fsanitize=address,undefined it is the sanitizer run of the policy.
//   search_plan_cases <table.tsv> | --sweep
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "gswm_search_plan.h"

static SearchQuery query(int kind, int B, int64_t n_bits, int msg_bytes, int64_t stride, int64_t n_records, int k, int levels, int signs = 1, int planes = 1, int wsum = 1,
                         int records = 1, int outs = 1) {
    return SearchQuery{kind, B, n_bits, stride, n_records, msg_bytes, k, levels, signs != 2, planes != 2, wsum != 2, records != 2,
                       signs == 0, planes == 0, wsum == 0, records == 0, outs != 1};
}

// The invariants of a launch that no kernel checks.  Returns the names of the broken ones ("" if none).
static std::string broken(const SearchQuery& q, const SearchPlan& p) {
    std::string bad;
    auto need = [&](bool ok, const char* name) { if (!ok) bad += std::string(bad.empty() ? "" : ",") + name; };
    const bool key = q.kind == SEARCH_KEY;
    const int lists = key ? KS_WG / p.G : KY_WAVES * p.T;                   // running lists the top-k tail puts into the LDS
    need(p.lds <= 131072u, "lds<=131072");
    need(p.lds >= (uint32_t)lists * SEARCH_LIST * 8u, "lds>=tail");
    need(p.T == 1 || p.T == 4 || p.T == 16 || p.T == 64, "T");
    need((int64_t)p.grid_y * p.T >= q.B && p.grid_y >= 1 && p.grid_y <= 65535, "grid_y");
    need(p.grid_x >= 1 && p.grid_x <= search_grid_cap(q.kind, q.n_records), "grid_x");
    need(p.ws_bytes == (size_t)q.B * (size_t)search_grid_cap(q.kind, q.n_records) * (size_t)q.k * 8u && p.ws_bytes == search_workspace_bytes(q.kind, q.B, q.n_records, q.k), "ws");
    need(p.rowbytes * 8ll == q.n_bits && p.nblk == (p.rowbytes + 63) / 64, "row");
    if (key) {
        need(p.G >= 1 && p.G <= 64 && (p.G & (p.G - 1)) == 0, "G");
        need(p.kpi >= 1, "kpi>=1");
        need((int64_t)p.G * p.T * p.kpi <= KS_WG, "G*T*kpi<=256");
        need(p.srow >= 16 * p.nblk, "srow");
        need(p.sg ? p.T == 1 : (int64_t)p.T * p.srow * 4 + (int64_t)p.kpi * p.nblk * 64 <= (int64_t)p.lds, "rows+keystreams<=lds");
        need((int64_t)p.copies * 8 * q.msg_bytes == q.n_bits, "copies");
        need(p.planes == 0 || (p.planes % 4 == 0 && p.planes <= 16 && (int64_t)p.copies < (1ll << p.planes) && q.msg_bytes % 4 == 0 && (!p.sg || p.signs_aligned)), "PL");
    } else {
        need((int64_t)(1 + p.planes) * p.T * p.nblk * 64 <= (int64_t)p.lds, "rows<=lds");
        need(p.msg4 == (q.msg_bytes % 4 == 0), "msg4");
    }
    return bad;
}

static int sweep() {
    const int Bs[] = {1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 4096, 65535};
    const int mbs[] = {1, 2, 3, 4, 5, 7, 8, 12, 16, 31, 32, 33, 64, 100, 128, 255, 256};
    const int64_t Us[] = {1, 2, 7, 8, 9, 63, 64, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 1000003, 2147483647};
    long long n = 0, bad = 0;
    for (int kind = 0; kind < 3; ++kind)
        for (int levels : {1, 2, 3, 4, 7, 8, 15}) {
            if (kind != SEARCH_LEVEL && levels != 1) continue;
            const int P = kind != SEARCH_LEVEL ? 0 : levels < 2 ? 1 : levels < 4 ? 2 : levels < 8 ? 3 : 4;
            for (int mb : mbs) {
                // copies: small ones, the PL boundaries, the tile and SG edges of this message length (both sides), the domain's edge
                std::vector<int64_t> copies = {1, 2, 3, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097};
                for (int64_t edge : {2048, 8192, 32768, 65408, 131072})
                    for (int64_t bytes : {edge / (1 + P), edge})
                        for (int64_t d = -2; d <= 2; ++d) copies.push_back(bytes / mb + d);
                for (int64_t c : copies) {
                    if (c < 1) continue;
                    const int64_t n_bits = c * 8 * mb;
                    for (int B : Bs)
                        for (int64_t U : Us)
                            for (int k : {1, 8})
                                for (int signs : {1, 2}) {
                                    const SearchQuery q = query(kind, B, n_bits, mb, kind == SEARCH_KEY ? 48 : (48 + mb + 15) / 16 * 16, U, k, levels, signs);
                                    const SearchPlan p = search_decide(q);
                                    ++n;
                                    if (p.status != GSW_OK) {
                                        if (p.status != GSW_ERR_UNSUPPORTED || n_bits * (1 + P) <= GSW_ROW_MAX_BITS) { printf("refused\t%d\t%d\t%lld\t%d\n", kind, B, (long long)n_bits, mb); ++bad; }
                                        continue;
                                    }
                                    const std::string b = broken(q, p);
                                    if (!b.empty()) { printf("%s\tkind=%d\tlevels=%d\tB=%d\tn_bits=%lld\tmsg_bytes=%d\tn_records=%lld\tk=%d\tsigns=%d\tlds=%u\n", b.c_str(), kind, levels, B, (long long)n_bits, mb, (long long)U, k, signs, p.lds); ++bad; }
                                }
                }
            }
        }
    fprintf(stderr, "%lld inputs, %lld broken\n", n, bad);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s <table.tsv> | --sweep\n", argv[0]); return 2; }
    if (!strcmp(argv[1], "--sweep")) return sweep();
    std::ifstream in(argv[1]);
    std::string line;
    if (!in || !std::getline(in, line)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    while (std::getline(in, line)) {
        std::vector<std::string> f;
        std::stringstream ss(line);
        for (std::string cell; std::getline(ss, cell, '\t');) f.push_back(cell);
        if (f.size() < 14) { fprintf(stderr, "short row: %s\n", line.c_str()); return 2; }
        int c = 1;
        auto next = [&] { return atoll(f[c++].c_str()); };
        const int kind = (int)next(), B = (int)next();
        const int64_t n_bits = next();
        const int msg_bytes = (int)next();
        const int64_t stride = next(), n_records = next();
        const int k = (int)next(), levels = (int)next(), signs = (int)next(), planes = (int)next(), wsum = (int)next(), records = (int)next(), outs = (int)next();
        const SearchPlan p = search_decide(query(kind, B, n_bits, msg_bytes, stride, n_records, k, levels, signs, planes, wsum, records, outs));
        printf("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%u\t%zu\t%zu\n", f[0].c_str(), p.status, p.T, (int)p.msg4, p.planes, (int)p.sg, p.G, p.kpi, p.srow, p.copies,
               p.rowbytes, p.nblk, p.signs_aligned, p.grid_x, p.grid_y, p.wg, p.lds, p.ws_bytes, search_workspace_bytes(kind, B, n_records, k));
    }
    return 0;
}
