// attn_plan_cases.cpp -- prints what attn_decide (csrc/gswm_attn_plan.h) decides for every row of tests/golden/attn_plan_cases.tsv, in the table's decision columns.
// Host code only: tests/test_attn_plan_host.py builds it with the library's compiler and compares the output with the recorded columns; built with
// -fsanitize=address,undefined it is the sanitizer run of the policy (64-bit products next to 32-bit fields).
//   attn_plan_cases <table.tsv>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "gswm_attn_plan.h"

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s <table.tsv>\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    if (!in || !std::getline(in, line)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    while (std::getline(in, line)) {
        std::vector<std::string> f;
        std::stringstream ss(line);
        for (std::string cell; std::getline(ss, cell, '\t');) f.push_back(cell);
        if (f.size() < 12) { fprintf(stderr, "short row: %s\n", line.c_str()); return 2; }
        int c = 1;
        auto next = [&] { return atoll(f[c++].c_str()); };
        const int B = (int)next(), H = (int)next(), head_dim = (int)next(), Sq = (int)next(), Sk = (int)next(), Sk_valid = (int)next();
        const int64_t ws_bytes = next();
        AttnSwitches sw;
        sw.qb = (int)next(); sw.pair = (int)next(); sw.dma = (int)next(); sw.kvs = (int)next();
        const AttnLaunch d = attn_decide(B, H, head_dim, Sq, Sk, Sk_valid, ws_bytes, sw);
        printf("%s\t%d\t%d\t%d\t%d\t%d\t%u\t%u\t%u\t%u\t%u\t%lld\n", f[0].c_str(), d.status, d.QB, (int)d.ragged, (int)d.pair, (int)d.dma, d.ksplit, d.nqt, d.total, d.grid,
               d.lds_bytes, (long long)d.ws_need);
    }
    return 0;
}
