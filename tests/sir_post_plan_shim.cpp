// extern "C" face of the posterior half of csrc/gnode_sir_plan.cpp for tests/test_sir_post_plan.py (ctypes): the layout of a
// posterior sweep as a row of integers next to the plain sweep's, the launch plan under a given static LDS, and the two staging
// functions' verdicts with what they staged, so that the records of one can be held against the other's.
#include "gnode_sir_plan.h"
#include <cstring>

extern "C" {
int pst_maxo(void) { return GN_SIR_SCORE_MAXO; }
int pst_maxh(void) { return GN_SIR_POST_MAXH; }
int64_t pst_static_lds(void) { return (int64_t)kSirPostLds; }

// rows, tail, thr, start, phase, cand, shifts, rec_ptr, rec, zeros, records, horizons, total | sir_sweep_layout's tail, thr and total
void pst_layout(int n, int64_t nnz, int nb, int T, int P, int L, int C, int O, int R, int H, int64_t* o) {
    const SirPostLayout W = sir_post_layout(n, nnz, nb, T, P, L, C, O, R, H);
    const SirSweepLayout S = sir_sweep_layout(n, nnz, nb, T, P, L, C);
    const int64_t row[16] = {(int64_t)W.rows, (int64_t)W.tail, (int64_t)W.thr, (int64_t)W.start, (int64_t)W.phase, (int64_t)W.cand, (int64_t)W.shifts,
                             (int64_t)W.rec_ptr, (int64_t)W.rec, (int64_t)W.zeros, (int64_t)W.records, (int64_t)W.horizons, (int64_t)W.total,
                             (int64_t)S.tail, (int64_t)S.thr, (int64_t)S.total};
    memcpy(o, row, sizeof row);
}

// path, threads, grid, dynamic lds, lists in lds -- of the launch plan under `static_lds` bytes of static LDS
void pst_plan(int n, int nb, int cu, int64_t jobs, int edge_scan, int64_t static_lds, int64_t* o) {
    const SirLaunch P = sir_launch_plan(n, nb, cu, jobs, edge_scan != 0, (size_t)static_lds);
    const int64_t row[5] = {(int64_t)P.path, P.threads, P.grid, (int64_t)P.lds, frontier_lists_in_lds(n, nb, (size_t)static_lds)};
    memcpy(o, row, sizeof row);
}

static const char* put(const SirTimedStaged& s, int32_t* rec_ptr, uint32_t* rec, int32_t* zeros, int32_t* records, int64_t* n_rates, int64_t* n_rec) {
    static std::string err;
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

// the error text ("" = accepted); rec_ptr int32 [n + 1], rec uint32 [R], zeros / records int32 [O], staged_h int32 [H] are written
// when accepted; n_h: the horizons staged
const char* pst_stage(int n, int64_t nnz, int T, int P, int L, const int32_t* phase, const double* w, const double* gamma, const double* init,
                      int C, const int32_t* shifts, const int32_t* rec_set, const int32_t* rec_node, const int32_t* rec_offset,
                      const int32_t* rec_kind, int R, int O, int now, const int32_t* horizons, int H, int32_t* rec_ptr, uint32_t* rec, int32_t* zeros,
                      int32_t* records, int32_t* staged_h, int64_t* n_rates, int64_t* n_rec, int64_t* n_h) {
    const SirPostStaged s = sir_stage_post("entry", n, nnz, T, P, L, phase, w, gamma, init, C, shifts, rec_set, rec_node, rec_offset, rec_kind, R, O, now,
                                           horizons, H);
    *n_h = (int64_t)s.horizons.size();
    if (s.thr.error.empty()) memcpy(staged_h, s.horizons.data(), s.horizons.size() * sizeof(int32_t));
    return put(s, rec_ptr, rec, zeros, records, n_rates, n_rec);
}
// sir_stage_timed through the same face, for the comparison of the staged records
const char* pst_stage_timed(int n, int64_t nnz, int T, int P, int L, const int32_t* phase, const double* w, const double* gamma, const double* init,
                            int C, const int32_t* shifts, const int32_t* rec_set, const int32_t* rec_node, const int32_t* rec_offset,
                            const int32_t* rec_kind, int R, int O, int bins, int32_t* rec_ptr, uint32_t* rec, int32_t* zeros, int32_t* records,
                            int64_t* n_rates, int64_t* n_rec) {
    return put(sir_stage_timed("entry", n, nnz, T, P, L, phase, w, gamma, init, C, shifts, rec_set, rec_node, rec_offset, rec_kind, R, O, bins), rec_ptr,
               rec, zeros, records, n_rates, n_rec);
}
}
