// The mean-field's arithmetic, stated once for the forward (gnode_meanfield.hip) and its reverse sweep
// (gnode_meanfield_bwd.hip): the Dormand-Prince 5(4) tableau, a stage's argument y + h sum_j c_j k_j, and one row of the
// right-hand side.  The reverse sweep integrates an interval again from the recorded steps and has to arrive at the forward's
// bits, so both call these functions (the library is built with -ffp-contract=off: the same expression rounds the same way).
#pragma once
#include "gnode_common.h"

struct MfCoef { double c[7]; int n; };

// Dormand-Prince 5(4): row s holds the coefficients of stage s + 1's argument; row 6 is the 5th-order solution
static const double kMfA[7][6] = {
    {0, 0, 0, 0, 0, 0},
    {1.0 / 5, 0, 0, 0, 0, 0},
    {3.0 / 40, 9.0 / 40, 0, 0, 0, 0},
    {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0, 0},
    {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0, 0},
    {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656, 0},
    {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84}};
static const double kMfB4[7] = {5179.0 / 57600, 0, 7571.0 / 16695, 393.0 / 640, -92097.0 / 339200, 187.0 / 2100, 1.0 / 40};

static inline MfCoef mf_stage_coef(int s) {                           // the first s entries of row s
    MfCoef cf; cf.n = s;
    for (int j = 0; j < s; ++j) cf.c[j] = kMfA[s][j];
    return cf;
}

// (y + h * sum_j c_j k_j)[i]        (k_j = K + j * len)
__device__ static inline double mf_comb_at(const double* __restrict__ y, const double* __restrict__ K, const MfCoef& cf, double h,
                                           long len, long i) {
    double s = 0.0;
    for (int j = 0; j < cf.n; ++j) s += cf.c[j] * K[(size_t)j * len + i];
    return y[i] + h * s;
}

// Row r = b * n + v of k = f(y) for the [3][rows] state y: the infection and the recovery flow (k_S = -inf, k_I = inf - rec,
// k_R = rec).  Row r gathers from its own sample's I; w_in[p] is the weight of the contact col[p] -> v; the infection rate is
// beta[r] with BETA, else the one number beta_s.
template <bool W, bool BETA>
__device__ static inline void mf_rhs_row(const int* __restrict__ rowptr, const int* __restrict__ col, int n, int rows, int r,
                                         const double* __restrict__ beta, double beta_s, const double* __restrict__ w_in,
                                         const double* __restrict__ gamma, const double* __restrict__ y, double* inf, double* rec) {
    const int v = r % n;
    const double* I = y + rows + (r - v);                             // sample b's I: y[rows + b * n + .]
    double ai = 0.0;
    for (int e = rowptr[v]; e < rowptr[v + 1]; ++e) ai += W ? w_in[e] * I[col[e]] : I[col[e]];
    *inf = (BETA ? beta[r] : beta_s) * (ai * y[r]);
    *rec = gamma[r] * I[v];
}

// w_in[p] = w[rev[p]] on the stream (gnode_meanfield.hip's k_mf_w_in; rev is the handle's table of a symmetric pattern)
int gn_mf_stage_w_in(const gnode_graph_s* g, const double* w, double* w_in, hipStream_t st);
