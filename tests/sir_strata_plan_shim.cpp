// extern "C" face of sir_stage_strata (csrc/gnode_sir_plan.cpp) for tests/test_sir_strata_plan.py (ctypes), which loads it next
// to tests/sir_post_plan_shim.cpp: the staging's verdict with what it staged, in the form of that shim's pst_stage, so that
// the two can be held against each other.
#include "gnode_sir_plan.h"
#include <cstring>

extern "C" {
int xst_maxd(void) { return GN_SIR_POST_MAXD; }

// the error text ("" = accepted); rec_ptr int32 [n + 1], rec uint32 [R], zeros / records int32 [O], staged_h int32 [H] are written
// when accepted; n_rates, n_rec, n_h: the thresholds, record words and table entries, and horizons staged
const char* xst_stage(int n, int64_t nnz, int T, int P, int L, const int32_t* phase, const double* w, const double* gamma, const double* init,
                      int C, const int32_t* shifts, const int32_t* rec_set, const int32_t* rec_node, const int32_t* rec_offset,
                      const int32_t* rec_kind, int R, int O, int now, const int32_t* horizons, int H, int mismatches, int32_t* rec_ptr,
                      uint32_t* rec, int32_t* zeros, int32_t* records, int32_t* staged_h, int64_t* n_rates, int64_t* n_rec, int64_t* n_h) {
    static std::string err;
    const SirPostStaged s = sir_stage_strata("entry", n, nnz, T, P, L, phase, w, gamma, init, C, shifts, rec_set, rec_node, rec_offset, rec_kind, R, O,
                                             now, horizons, H, mismatches);
    *n_rates = (int64_t)s.thr.rates.size();
    *n_rec = (int64_t)(s.rec.size() + s.rec_ptr.size() + s.zeros.size() + s.records.size());
    *n_h = (int64_t)s.horizons.size();
    if (s.thr.error.empty()) {
        memcpy(rec_ptr, s.rec_ptr.data(), s.rec_ptr.size() * sizeof(int32_t));
        memcpy(rec, s.rec.data(), s.rec.size() * sizeof(uint32_t));
        memcpy(zeros, s.zeros.data(), s.zeros.size() * sizeof(int32_t));
        memcpy(records, s.records.data(), s.records.size() * sizeof(int32_t));
        memcpy(staged_h, s.horizons.data(), s.horizons.size() * sizeof(int32_t));
    }
    err = s.thr.error;
    return err.c_str();
}
}
