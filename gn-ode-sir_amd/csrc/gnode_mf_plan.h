// The host side of the mean-field's reverse sweep that never touches the device, stated once: whether a list of accepted step
// sizes is one that the forward's controller can have walked over the output times (mf_check_steps), and where every array of
// gnode_meanfield_rates_backward_f64 sits in the caller's workspace (mf_bwd_layout).  Plain C++, like gnode_graph_plan.h and
// gnode_sir_plan.h: tests/test_mf_plan.py compiles this unit with the system compiler.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

// The forward walks an interval (t_out[to - 1], t_out[to]] as  t = t_out[to - 1];  while (t < t_end) { hh = min(h, t_end - t); ...
// t = (hh == t_end - t) ? t_end : t + hh; }  -- so the n_acc[to] steps of interval `to` are finite and > 0, every one but the last
// leaves t + h < t_end, and the last one IS t_end - t, bit for bit.  n_acc[0] = 0, an interval of no length has no step, one of
// positive length has at least one, and the counts add up to n_h.
struct MfStepPlan {
    std::string error;                 // non-empty: refused; names `who` and the interval
    int32_t max_interval_steps = 0;    // the largest n_acc[to]
};
MfStepPlan mf_check_steps(const char* who, const double* t_out, int32_t n_out, const double* h, int64_t n_h, const int32_t* n_acc);

// Byte offsets into the backward's workspace (each 256-byte aligned) for a state of `rows` = B * n rows, len = 3 * rows doubles
// per state ([S | I | R] planes of `rows`):
struct MfBwdLayout {
    size_t ybar;      // [len]       the adjoint of y, carried down the whole sweep
    size_t ystage;    // [5][len]    Y_2 .. Y_6 of the step being swept (Y_1 is the step's y in `store`)
    size_t k;         // [6][len]    k_1 .. k_6, back to back in elements (mf_comb_at's indexing)
    size_t ybar_st;   // [6][2][rows] Ybar_1 .. Ybar_6, S and I planes (Rbar_s = 0; Ybar_7 is ybar)
    size_t c;         // [2][rows]   c = d beta S of the stage just done and of the one before: read by neighbours, so double-buffered
    size_t w_in;      // [max(nnz, 1)] w[rev[p]], staged as the forward stages it
    size_t store;     // [max_interval_steps + 1][len]  y at every accepted step of the interval being swept
    size_t bytes;
};
MfBwdLayout mf_bwd_layout(int64_t rows, int64_t nnz, int32_t max_interval_steps);
