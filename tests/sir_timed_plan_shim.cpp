// extern "C" face of the timed-evidence half of csrc/gnode_sir_plan.cpp for tests/test_sir_timed_plan.py (ctypes): the layout of
// a timed sweep as a row of integers next to the plain sweep's, the launch plan with and without the difference array's static
// LDS, and the staging function's verdict with what it staged.
#include "gnode_sir_plan.h"
#include <cstring>

extern "C" {
int tmd_maxo(void) { return GN_SIR_SCORE_MAXO; }
int tmd_cells(void) { return GN_SIR_TIMED_CELLS; }
int64_t tmd_static_lds(void) { return (int64_t)kSirTimedLds; }

// rows, tail, thr, start, phase, cand, shifts, rec_ptr, rec, zeros, records, total | sir_sweep_layout's tail, thr and total
void tmd_layout(int n, int64_t nnz, int nb, int T, int P, int L, int C, int O, int R, int64_t* o) {
    const SirTimedLayout W = sir_timed_layout(n, nnz, nb, T, P, L, C, O, R);
    const SirSweepLayout S = sir_sweep_layout(n, nnz, nb, T, P, L, C);
    const int64_t row[15] = {(int64_t)W.rows, (int64_t)W.tail, (int64_t)W.thr, (int64_t)W.start, (int64_t)W.phase, (int64_t)W.cand, (int64_t)W.shifts,
                             (int64_t)W.rec_ptr, (int64_t)W.rec, (int64_t)W.zeros, (int64_t)W.records, (int64_t)W.total, (int64_t)S.tail, (int64_t)S.thr,
                             (int64_t)S.total};
    memcpy(o, row, sizeof row);
}

// path, threads, grid, dynamic lds, lists in lds -- of the launch plan under `static_lds` bytes of static LDS
void tmd_plan(int n, int nb, int cu, int64_t jobs, int edge_scan, int64_t static_lds, int64_t* o) {
    const SirLaunch P = sir_launch_plan(n, nb, cu, jobs, edge_scan != 0, (size_t)static_lds);
    const int64_t row[5] = {(int64_t)P.path, P.threads, P.grid, (int64_t)P.lds, frontier_lists_in_lds(n, nb, (size_t)static_lds)};
    memcpy(o, row, sizeof row);
}

// the error text ("" = accepted); rec_ptr int32 [n + 1], rec uint32 [R], zeros / records int32 [O] are written when accepted
const char* tmd_stage(int n, int64_t nnz, int T, int P, int L, const int32_t* phase, const double* w, const double* gamma, const double* init,
                      int C, const int32_t* shifts, const int32_t* rec_set, const int32_t* rec_node, const int32_t* rec_offset,
                      const int32_t* rec_kind, int R, int O, int bins, int32_t* rec_ptr, uint32_t* rec, int32_t* zeros, int32_t* records,
                      int64_t* n_rates, int64_t* n_rec) {
    static std::string err;
    const SirTimedStaged s = sir_stage_timed("entry", n, nnz, T, P, L, phase, w, gamma, init, C, shifts, rec_set, rec_node, rec_offset, rec_kind, R, O, bins);
    *n_rates = (int64_t)s.thr.rates.size(); *n_rec = (int64_t)(s.rec.size() + s.rec_ptr.size() + s.zeros.size() + s.records.size());
    if (s.thr.error.empty()) {
        memcpy(rec_ptr, s.rec_ptr.data(), s.rec_ptr.size() * sizeof(int32_t));
        memcpy(rec, s.rec.data(), s.rec.size() * sizeof(uint32_t));
        memcpy(zeros, s.zeros.data(), s.zeros.size() * sizeof(int32_t));
        memcpy(records, s.records.data(), s.records.size() * sizeof(int32_t));
    }
    err = s.thr.error;
    return err.c_str();
}
}
