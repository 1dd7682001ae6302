// Recorder of tests/golden/sir_plan_parent.json.  It is built AT THE COMMIT BEFORE csrc/gnode_sir_plan.cpp EXISTED (where the
// layout and the planners are static functions of gnode_sir.hip), needs no GPU, and prints what tests/sir_plan_shim.cpp's main
// prints for the same case file; `python tests/test_sir_plan.py <rows file>` turns the rows into the fixture:
//   python tests/test_sir_plan.py --cases > cases.txt                         (at this commit)
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -x hip -Iinclude -Ign-ode-sir_amd/csrc tests/golden/make_sir_plan_parent.cpp -o rec
//   ./rec cases.txt > rows.txt                                                (in a checkout of the parent; ~17 s to build)
#include "gnode_sir.hip"

void gnode_set_error(const char*, ...) {}
int gn_zero_async(void*, size_t, hipStream_t) { return 0; }
bool gn_prof_begin(int, hipStream_t) { return false; }
void gn_prof_end(int, hipStream_t) {}
int gn_device_setup_once(int) { return 0; }

int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    long n, nnz, nb, T, cu, sims, es;
    while (fscanf(f, "%ld %ld %ld %ld %ld %ld %ld", &n, &nnz, &nb, &T, &cu, &sims, &es) == 7) {
        gnode_graph_s gs{};
        gs.info.n = (int32_t)n; gs.info.num_cu = (int32_t)cu; gs.nnz = nnz; gs.n_bigrow = (int32_t)nb;
        gnode_graph_t g = &gs;
        const bool edge_scan = es != 0;
        // the workspace pointers of sir_mc_philox_impl, as offsets
        const size_t hist_b = gn_align((size_t)2 * T * g->info.n * sizeof(uint32_t));
        const size_t seeds = hist_b, src = hist_b + gn_align(4096 * sizeof(int32_t));
        const size_t gstate = hist_b + gn_align(4096 * sizeof(int32_t)) + gn_align((size_t)std::max<int64_t>(g->nnz, 1) * sizeof(int32_t));
        const size_t thr_b = gnode_sir_workspace_bytes(g, (int32_t)T), thr_init = gnode_sir_edges_workspace_bytes(g, (int32_t)T);
        // its launch lambda
        int per_cu_f = 1;
        const int threads_f = frontier_threads(g->info.n, g->n_bigrow, &per_cu_f);
        const size_t fl = frontier_lds_bytes(g->info.n, g->n_bigrow, threads_f);
        const size_t lds = (size_t)2 * g->info.n;
        int path, grid, threads;
        size_t dyn;
        if (fl <= kLdsStateLimit && !edge_scan) {
            const int per_cu = per_cu_f;
            threads = threads_f; dyn = fl;
            if (frontier_lists_in_lds(g->info.n, g->n_bigrow)) { path = 0; grid = (int)std::min<int64_t>(sims, (int64_t)g->info.num_cu * per_cu); }
            else { path = 1; grid = (int)std::min<int64_t>(std::min<int64_t>(sims, (int64_t)g->info.num_cu * per_cu), kFrontierGlobalGrid); }
        } else if (lds <= kLdsStateLimit) {
            const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / std::max<size_t>(lds, 1)));
            threads = per_cu >= 4 ? 256 : (per_cu >= 2 ? 512 : 1024);
            grid = (int)std::min<int64_t>(sims, (int64_t)g->info.num_cu * per_cu);
            path = 2; dyn = lds;
        } else { path = 3; grid = (int)std::min<int64_t>(sims, 2048); threads = 256; dyn = 0; }
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %zu %d %d %d %zu\n", gnode_sir_workspace_bytes(g, (int32_t)T),
               gnode_sir_nodes_workspace_bytes(g, (int32_t)T), gnode_sir_edges_workspace_bytes(g, (int32_t)T),
               gnode_sir_init_workspace_bytes(g, (int32_t)T), gnode_sir_traj_workspace_bytes(g, (int32_t)T), seeds, src, gstate, thr_b,
               thr_init, (int)frontier_lists_in_lds(g->info.n, g->n_bigrow), threads_f, per_cu_f, fl, path, grid, threads, dyn);
    }
    const double ps[] = {0.0, 1.0, 0x1p-33, 1.0 - 0x1p-33, 0.3, 0x1p-32, 0.5};
    for (double p : ps) printf("coin %llu\n", coin_threshold(p));
    return 0;
}
