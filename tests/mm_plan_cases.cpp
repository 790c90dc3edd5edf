// mm_plan_cases.cpp -- prints what mm_decide (csrc/gswm_mm_plan.h) decides for every row of tests/golden/mm_plan_cases.tsv, in the table's decision columns.
// Host code only: tests/test_mm_plan_host.py builds it with the library's compiler and compares the output with the recorded columns; built with
// -fsanitize=address,undefined it is the sanitizer run of the policy (64-bit products next to 32-bit fields).
//   mm_plan_cases <table.tsv>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "gswm_mm_plan.h"

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s <table.tsv>\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    std::string line;
    if (!in || !std::getline(in, line)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    auto ptr = [](long long kind) { return (char*)(uintptr_t)(kind == 0 ? 0 : kind == 2 ? 0x10004 : 0x10000); };      // null / aligned / misaligned; never dereferenced
    while (std::getline(in, line)) {
        std::vector<std::string> f;
        std::stringstream ss(line);
        for (std::string cell; std::getline(ss, cell, '\t');) f.push_back(cell);
        if (f.size() < 33) { fprintf(stderr, "short row: %s\n", line.c_str()); return 2; }
        int c = 1;
        auto next = [&] { return atoll(f[c++].c_str()); };
        MMArgs a = mm_args_rows(ptr(1), 0, 0, ptr(1), 0, ptr(1), 0, 0);
        a.mode = (int32_t)next(); a.M = (int32_t)next(); a.N = (int32_t)next(); a.P = (int32_t)next(); a.nseg = (int32_t)next();
        const int32_t ld_max = (int32_t)next();
        for (MMSeg& s : a.seg) s.ld = ld_max;
        a.ldw = (int32_t)next(); a.ldy = (int32_t)next(); a.ldr = (int32_t)next();
        a.resid = next() ? ptr(1) : nullptr; a.rowbias = next() ? ptr(1) : nullptr; a.ln_stat = next() ? ptr(1) : nullptr; a.bias = ptr(next());
        a.flags = (int32_t)next(); a.Hp = (int32_t)next(); a.Wp = (int32_t)next(); a.in_Hp = (int32_t)next(); a.in_Wp = (int32_t)next(); a.S = (int32_t)next();
        a.n_rows = (int32_t)next(); a.y2 = next() ? ptr(1) : nullptr;
        a.ldrb = a.N;
        GswMmExtras ex{};
        ex.workspace_dev = ptr(next()); ex.workspace_bytes = next(); ex.max_splits = (int)next();
        ex.colstats_dev = (float*)ptr(next()); ex.colstats_capacity = next();
        ex.rowstats_dev = (float*)ptr(next()); ex.rowstats_capacity = next();
        ex.flags = (int)next(); ex.splits = 1;
        MMKnobs k{0, 0, 256, 0, 7, 5, 64, 8};      // the defaults of every knob the table does not vary
        k.tile_rows = (int)next(); k.split_mask = (int)next();
        const int dtype = (int)next();
        const MMLaunch d = mm_decide(a, dtype, ex, k);
        // what the convolution front end asks (mm_predict_us: M x N outputs over P stages) is this launch's own prediction unless LayerNorm statistics forbid a split
        if (d.status == GSW_OK && !a.ln_stat && mm_predict_us(a.M, a.N, a.P, ex, k) != d.t_us) { fprintf(stderr, "mm_predict_us != t_us: %s\n", f[0].c_str()); return 3; }
        printf("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%u\t%d\t%d\t%d\t%d\t%d\t%d\t%lld\t%a\n", f[0].c_str(), d.status, d.tile_rows, d.tile_cols, d.mt, (int)d.wide, d.splits,
               d.panel, d.tiles_n, d.ntiles, d.grid, d.epi, (int)d.wave12, (int)d.lnf, d.rowstats_slots, d.colstats_rows_per_block, d.colstats_blocks,
               (long long)d.ws_need, d.t_us);
    }
    return 0;
}
