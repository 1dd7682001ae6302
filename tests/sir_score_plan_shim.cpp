// extern "C" face of the source-score half of csrc/gnode_sir_plan.cpp for tests/test_sir_score_plan.py (ctypes): the layout of a
// scored sweep as a row of integers next to the plain sweep's, the launch plan with and without the tallies' static LDS, and
// the staging function's verdict with what it staged.
#include "gnode_sir_plan.h"
#include <cstring>

extern "C" {
int sco_maxo(void) { return GN_SIR_SCORE_MAXO; }
int64_t sco_static_lds(void) { return (int64_t)kSirScoreLds; }

// rows, tail, thr, start, phase, cand, shifts, obs, marked, seen, total | sir_sweep_layout's tail, thr and total
void sco_layout(int n, int64_t nnz, int nb, int T, int P, int L, int C, int O, int64_t* o) {
    const SirScoreLayout W = sir_score_layout(n, nnz, nb, T, P, L, C, O);
    const SirSweepLayout S = sir_sweep_layout(n, nnz, nb, T, P, L, C);
    const int64_t row[14] = {(int64_t)W.rows, (int64_t)W.tail, (int64_t)W.thr, (int64_t)W.start, (int64_t)W.phase, (int64_t)W.cand, (int64_t)W.shifts,
                             (int64_t)W.obs, (int64_t)W.marked, (int64_t)W.seen, (int64_t)W.total, (int64_t)S.tail, (int64_t)S.thr, (int64_t)S.total};
    memcpy(o, row, sizeof row);
}

// path, threads, grid, dynamic lds, lists in lds -- of the launch plan under `static_lds` bytes of static LDS
void sco_plan(int n, int nb, int cu, int64_t jobs, int edge_scan, int64_t static_lds, int64_t* o) {
    const SirLaunch P = sir_launch_plan(n, nb, cu, jobs, edge_scan != 0, (size_t)static_lds);
    const int64_t row[5] = {(int64_t)P.path, P.threads, P.grid, (int64_t)P.lds, frontier_lists_in_lds(n, nb, (size_t)static_lds)};
    memcpy(o, row, sizeof row);
}

// the error text ("" = accepted); obs_out int8 [n][O], marked / seen int32 [O] are written when accepted
const char* sco_stage(int n, int64_t nnz, int T, int P, int L, const int32_t* phase, const double* w, const double* gamma, const double* init,
                      int C, const int32_t* shifts, const int8_t* obs, int O, int measure, int bins, int8_t* obs_out, int32_t* marked,
                      int32_t* seen, int64_t* n_rates, int64_t* n_obs) {
    static std::string err;
    const SirScoreStaged s = sir_stage_score("entry", n, nnz, T, P, L, phase, w, gamma, init, C, shifts, obs, O, measure, bins);
    *n_rates = (int64_t)s.thr.rates.size(); *n_obs = (int64_t)s.obs.size();
    if (s.thr.error.empty()) {
        memcpy(obs_out, s.obs.data(), s.obs.size());
        memcpy(marked, s.marked.data(), s.marked.size() * sizeof(int32_t));
        memcpy(seen, s.seen.data(), s.seen.size() * sizeof(int32_t));
    }
    err = s.thr.error;
    return err.c_str();
}
}
