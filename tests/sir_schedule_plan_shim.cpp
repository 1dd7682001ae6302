// extern "C" face of the schedule half of csrc/gnode_sir_plan.cpp for tests/test_sir_schedule_plan.py (ctypes): the layout of
// a scheduled call as a row of integers, and the staging function.
#include "gnode_sir_plan.h"
#include <cstring>

extern "C" {
// hist, seeds, rows, tail, thr, start, phase, total | sir_layout's thr and its per-edge form's size, for comparison
void ssp_layout(int n, int64_t nnz, int nb, int T, int P, int64_t* o) {
    const SirScheduleLayout L = sir_schedule_layout(n, nnz, nb, T, P);
    const SirLayout B = sir_layout(n, nnz, nb, T);
    const int64_t row[10] = {(int64_t)L.hist, (int64_t)L.seeds, (int64_t)L.rows, (int64_t)L.tail, (int64_t)L.thr, (int64_t)L.start,
                             (int64_t)L.phase, (int64_t)L.total, (int64_t)B.thr, (int64_t)B.bytes[SIR_INIT]};
    memcpy(o, row, sizeof row);
}

// the error text ("" = accepted); rates[n_rates] and start[n_start] receive the thresholds (room for P * (nnz + n) and 2n)
const char* ssp_stage(int n, int64_t nnz, int T, int P, const int32_t* phase, const double* w, const double* gamma, const double* init,
                      unsigned long long* rates, int64_t* n_rates, unsigned long long* start, int64_t* n_start) {
    static std::string err;
    const SirThresholds t = sir_stage_schedule("entry", n, nnz, T, P, phase, w, gamma, init);
    *n_rates = (int64_t)t.rates.size(); *n_start = (int64_t)t.start.size();
    if (!t.rates.empty()) memcpy(rates, t.rates.data(), t.rates.size() * sizeof(unsigned long long));
    if (!t.start.empty()) memcpy(start, t.start.data(), t.start.size() * sizeof(unsigned long long));
    err = t.error;
    return err.c_str();
}
}
