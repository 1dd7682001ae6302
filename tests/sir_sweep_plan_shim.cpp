// extern "C" face of the sweep half of csrc/gnode_sir_plan.cpp for tests/test_sir_sweep_plan.py (ctypes): the layout of a
// candidate sweep as a row of integers next to the scheduled call's, and the staging function's verdict.
#include "gnode_sir_plan.h"
#include <cstring>

extern "C" {
// rows, tail, thr, start, phase, cand, shifts, total | sir_schedule_layout's rows, total and its histogram's size (= seeds)
void swp_layout(int n, int64_t nnz, int nb, int T, int P, int L, int C, int64_t* o) {
    const SirSweepLayout W = sir_sweep_layout(n, nnz, nb, T, P, L, C);
    const SirScheduleLayout S = sir_schedule_layout(n, nnz, nb, T, P);
    const int64_t row[11] = {(int64_t)W.rows, (int64_t)W.tail, (int64_t)W.thr, (int64_t)W.start, (int64_t)W.phase, (int64_t)W.cand,
                             (int64_t)W.shifts, (int64_t)W.total, (int64_t)S.rows, (int64_t)S.total, (int64_t)(S.seeds - S.hist)};
    memcpy(o, row, sizeof row);
}

// the error text ("" = accepted) and the number of thresholds staged
const char* swp_stage(int n, int64_t nnz, int T, int P, int L, const int32_t* phase, const double* w, const double* gamma, const double* init,
                      int C, const int32_t* shifts, int64_t* n_rates, int64_t* n_start) {
    static std::string err;
    const SirThresholds t = sir_stage_sweep("entry", n, nnz, T, P, L, phase, w, gamma, init, C, shifts);
    *n_rates = (int64_t)t.rates.size(); *n_start = (int64_t)t.start.size();
    err = t.error;
    return err.c_str();
}
}
