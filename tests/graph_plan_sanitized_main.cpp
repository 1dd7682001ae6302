// Stand-alone driver of csrc/gnode_graph_plan.cpp for a sanitizer build (tests/test_graph_plan.py compiles both with
// -fsanitize=address,undefined and runs the program once): plans every CSR of the file named by argv[1] -- per graph the line
// "n nnz", then n + 1 row pointers and nnz column ids -- and walks every edge-table entry, so that a read or a write outside
// the plan's vectors stops the run.  Prints one line per graph: nnz, symmetric, entries without a reverse.
#include "gnode_graph_plan.h"
#include <cstdio>

int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    long n, nnz;
    while (fscanf(f, "%ld %ld", &n, &nnz) == 2) {
        std::vector<int32_t> rp((size_t)n + 1), ci((size_t)nnz);
        for (int32_t& v : rp) if (fscanf(f, "%d", &v) != 1) return 2;
        for (int32_t& v : ci) if (fscanf(f, "%d", &v) != 1) return 2;
        const GnGraphPlan P = gn_plan_graph(rp.data(), ci.data(), (int32_t)n, nnz);
        if (!P.error.empty() || P.src.size() != (size_t)nnz || P.rev.size() != (size_t)nnz) return 3;
        long lost = 0;
        for (long p = 0; p < nnz; ++p) {
            const int32_t r = P.rev[p];
            if (r < 0) { ++lost; continue; }
            if (r >= nnz || ci[r] != P.src[p] || P.src[r] != ci[p]) return 4;
        }
        if (P.symmetric != (lost == 0)) return 5;
        printf("%ld %d %ld\n", nnz, (int)P.symmetric, lost);
    }
    fclose(f);
    return 0;
}
