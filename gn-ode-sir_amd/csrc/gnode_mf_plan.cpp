// Step-list validation and workspace layout of the mean-field's reverse sweep (gnode_mf_plan.h); gnode_meanfield_bwd.hip holds
// the kernels and the call.
#include "gnode_mf_plan.h"
#include <algorithm>
#include <cmath>
#include <cstdio>

static size_t al(size_t x) { return (x + 255) / 256 * 256; }

static MfStepPlan refuse(const char* who, int to, const char* fmt, double a, double b) {
    char what[160], msg[256];
    snprintf(what, sizeof what, fmt, a, b);
    snprintf(msg, sizeof msg, "%s: step list, interval %d: %s", who, to, what);
    MfStepPlan p;
    p.error = msg;
    return p;
}

MfStepPlan mf_check_steps(const char* who, const double* t_out, int32_t n_out, const double* h, int64_t n_h, const int32_t* n_acc) {
    MfStepPlan p;
    if (n_acc[0] != 0) return refuse(who, 0, "%.0f steps in front of the first output time", (double)n_acc[0], 0.0);
    int64_t at = 0;
    for (int to = 1; to < n_out; ++to) {
        const int32_t m = n_acc[to];
        const double t_end = t_out[to];
        if (m < 0) return refuse(who, to, "a negative step count %.0f", (double)m, 0.0);
        if (m > n_h - at) return refuse(who, to, "its %.0f steps run past the list's %.0f", (double)m, (double)n_h);
        if (m == 0 && t_end > t_out[to - 1]) return refuse(who, to, "no step from t=%.17g to t=%.17g", t_out[to - 1], t_end);
        double t = t_out[to - 1];
        for (int32_t i = 0; i < m; ++i) {
            const double hh = h[at + i];
            if (!(hh > 0.0) || !std::isfinite(hh)) return refuse(who, to, "h=%g is not a finite step > 0 (step %.0f of the interval)", hh, (double)i);
            if (i + 1 < m) {
                t = t + hh;
                if (!(t < t_end)) return refuse(who, to, "a step before the last reaches t=%.17g, not short of t_end=%.17g", t, t_end);
            } else if (hh != t_end - t) {
                return refuse(who, to, "the last step h=%.17g is not t_end - t=%.17g", hh, t_end - t);
            }
        }
        at += m;
        p.max_interval_steps = std::max(p.max_interval_steps, m);
    }
    if (at != n_h) return refuse(who, n_out - 1, "the counts add up to %.0f steps, the list has %.0f", (double)at, (double)n_h);
    return p;
}

MfBwdLayout mf_bwd_layout(int64_t rows, int64_t nnz, int32_t max_interval_steps) {
    MfBwdLayout L;
    const size_t r = (size_t)rows, v = al(3 * r * sizeof(double));
    size_t off = 0;
    L.ybar = off;    off += v;
    L.ystage = off;  off += 5 * v;
    L.k = off;       off += al(18 * r * sizeof(double));
    L.ybar_st = off; off += al(12 * r * sizeof(double));
    L.c = off;       off += 2 * al(r * sizeof(double));
    L.w_in = off;    off += al((size_t)std::max<int64_t>(nnz, 1) * sizeof(double));
    L.store = off;   off += ((size_t)max_interval_steps + 1) * v;
    L.bytes = off;
    return L;
}
