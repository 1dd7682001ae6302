// extern "C" face of csrc/gnode_mf_plan.cpp for tests/test_mf_plan.py (ctypes): check a step list, lay out the backward workspace.
#include "gnode_mf_plan.h"
#include <cstdio>

extern "C" {
// 0 and *max_steps, or 1 and the message in err
int mp_check(const double* t_out, int32_t n_out, const double* h, int64_t n_h, const int32_t* n_acc, int32_t* max_steps, char* err,
             int err_cap) {
    const MfStepPlan p = mf_check_steps("mp_check", t_out, n_out, h, n_h, n_acc);
    snprintf(err, (size_t)err_cap, "%s", p.error.c_str());
    *max_steps = p.max_interval_steps;
    return p.error.empty() ? 0 : 1;
}
// ybar, ystage, k, ybar_st, c, w_in, store, bytes
void mp_layout(int64_t rows, int64_t nnz, int32_t max_interval_steps, uint64_t* o) {
    const MfBwdLayout L = mf_bwd_layout(rows, nnz, max_interval_steps);
    const size_t f[8] = {L.ybar, L.ystage, L.k, L.ybar_st, L.c, L.w_in, L.store, L.bytes};
    for (int i = 0; i < 8; ++i) o[i] = f[i];
}
}
