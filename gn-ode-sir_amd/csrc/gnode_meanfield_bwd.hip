// The reverse sweep of the mean-field's Dormand-Prince 5(4) solve on MI355X (gfx950): gnode_meanfield_rates_backward_f64.
//
// With the accepted step sizes held fixed, a step is an explicit 6-stage Runge-Kutta map
//     Y_1 = y,  Y_s = y + h sum_{j<s} a_sj k_j  (s = 2..7),  k_s = f(Y_s),  y' = Y_7
// and its reverse, given ybar', is
//     Ybar_7 = ybar';  for s = 6..1:  kbar_s = h sum_{t>s} a_ts Ybar_t,  Ybar_s = VJP_f(Y_s; kbar_s);  ybar = sum_s Ybar_s
// (DESIGN.md 4.7 states VJP_f).  The sweep goes interval by interval from the last output time down: it integrates the interval
// again from the forward's own output row with the recorded steps -- the arithmetic is gnode_meanfield.h's, so the states are the
// forward's -- keeps y at every step, and then walks the steps backwards, recomputing Y_2..Y_6 of each.  fp64, no atomics, one
// writer per accumulator and launch, row sums in ascending CSR position: two calls return the same bits.
#include "gnode_meanfield.h"
#include "gnode_mf_plan.h"
#include <algorithm>

// k_{j+1} = f(Ys) and, row-locally, the next stage's argument out = y + h sum_{i<=j} c_i k_{i+1}: one launch per stage where the
// forward has two (every k_i[r] that row r's combination reads was written by row r's thread).
template <bool W, bool BETA>
__global__ __launch_bounds__(256) void k_mfb_stage(const int* __restrict__ rowptr, const int* __restrict__ col, int n, int rows,
                                                  const double* __restrict__ beta, const double* __restrict__ w_in,
                                                  const double* __restrict__ gamma, const double* __restrict__ Ys,
                                                  const double* __restrict__ y, double* K, int j, MfCoef cf, double h,
                                                  double* __restrict__ out) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    double inf, rec;
    mf_rhs_row<W, BETA>(rowptr, col, n, rows, r, beta, 1.0, w_in, gamma, Ys, &inf, &rec);
    const long len = 3L * rows;
    const double kv[3] = {-inf, inf - rec, rec};
    for (int c = 0; c < 3; ++c) {
        const long i = (long)c * rows + r;
        K[(size_t)j * len + i] = kv[c];
        out[i] = mf_comb_at(y, K, cf, h, len, i);
    }
}

// One launch of a step's reverse: see k_mfb_rev.  Stage numbers are 1-based as in the text above.
struct MfbRev {
    const int *rowptr, *col;
    int n, rows;
    long nnz;
    const double *beta, *w, *w_in, *gamma;      // beta [rows] or null = 1; w, w_in [nnz] or null = 1
    const double *Y, *Yg;                       // Y_sl and Y_sg, [3][rows] each
    double* ybar;                               // [3][rows]: Ybar_7 on the way in, the step's ybar after the last launch
    double* yst;                                // Ybar_s = yst + (s - 1) * 2 * rows: S plane, then I plane
    const double* c_prev;                       // c of stage sg, [rows]
    double* c_cur;                              // c of stage sl
    double *gb, *gw, *gg;                       // grad_beta [rows], grad_w [B][nnz], grad_gamma [rows]; null = not wanted
    int sg, sl;                                 // the stage whose gather is completed (0: none), the stage whose row part is done (0: none, sum up)
    double hc[8];                               // hc[t] = h a_{t,sl} for t = sl + 1 .. 7
};

// sum_{q in [lo, hi)} w[q] * x[col[q]] in ascending q, four independent loads in flight
template <bool W>
__device__ static inline double mfb_row_dot(const int* __restrict__ col, const double* __restrict__ w, const double* __restrict__ x,
                                            int lo, int hi) {
    double acc = 0.0;
    int q = lo;
    for (; q + 4 <= hi; q += 4) {
        const int c0 = col[q], c1 = col[q + 1], c2 = col[q + 2], c3 = col[q + 3];
        const double x0 = x[c0], x1 = x[c1], x2 = x[c2], x3 = x[c3];
        if (W) {
            const double w0 = w[q], w1 = w[q + 1], w2 = w[q + 2], w3 = w[q + 3];
            acc += w0 * x0; acc += w1 * x1; acc += w2 * x2; acc += w3 * x3;
        } else {
            acc += x0; acc += x1; acc += x2; acc += x3;
        }
    }
    for (; q < hi; ++q) acc += W ? w[q] * x[col[q]] : x[col[q]];
    return acc;
}

// Per row r = b * n + v, two things that meet in one grid-wide dependency per stage:
//   * stage sg's neighbour gather  Ibar_r = e gamma_r + sum_{q in row v} w[q] c_{b n + col q}, which completes Ybar_sg[r], and
//     in the same walk  wbar[b][q] += c_{b n + col q} I_b[v]  for q in row v (w[q] is the weight that row col q's sum took for
//     I_v): the row's own slots of grad_w, contiguous, one writer per (b, q);
//   * stage sl = sg - 1's row part: kbar_sl[r] from the stored Ybar_t[r], then d = kbarI - kbarS, e = kbarR - kbarI,
//     ai = sum_p w_in[p] I[col p], c = d beta S, Sbar = d beta ai, betabar += d ai S, gammabar += e I.
// The first launch of a step has no gather (sg = 0), the last no row part (sl = 0): it sums ybar = Ybar_7 + Ybar_6 + .. + Ybar_1.
template <bool W, bool BETA>
__global__ __launch_bounds__(256) void k_mfb_rev(MfbRev a) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.rows) return;
    const int rows = a.rows, v = r % a.n, base = r - v;
    const int lo = a.rowptr[v], hi = a.rowptr[v + 1];
    double ib_g = 0.0;
    if (a.sg) {
        double* ybI = a.yst + (size_t)(a.sg - 1) * 2 * rows + rows;
        const double* cp = a.c_prev + base;
        double acc;
        if (a.gw) {                                                   // the walk that gathers c also owns row v's slots of wbar
            double* gw = a.gw + (size_t)(base / a.n) * a.nnz;
            const double Iv = a.Yg[rows + r];
            acc = 0.0;
            int q = lo;
            for (; q + 4 <= hi; q += 4) {
                const int c0 = a.col[q], c1 = a.col[q + 1], c2 = a.col[q + 2], c3 = a.col[q + 3];
                const double x0 = cp[c0], x1 = cp[c1], x2 = cp[c2], x3 = cp[c3];
                const double g0 = gw[q], g1 = gw[q + 1], g2 = gw[q + 2], g3 = gw[q + 3];
                if (W) {
                    acc += a.w[q] * x0; acc += a.w[q + 1] * x1; acc += a.w[q + 2] * x2; acc += a.w[q + 3] * x3;
                } else {
                    acc += x0; acc += x1; acc += x2; acc += x3;
                }
                gw[q] = g0 + x0 * Iv; gw[q + 1] = g1 + x1 * Iv; gw[q + 2] = g2 + x2 * Iv; gw[q + 3] = g3 + x3 * Iv;
            }
            for (; q < hi; ++q) {
                const double x = cp[a.col[q]];
                acc += W ? a.w[q] * x : x;
                gw[q] += x * Iv;
            }
        } else {
            acc = mfb_row_dot<W>(a.col, a.w, cp, lo, hi);
        }
        ib_g = ybI[r] + acc;
        ybI[r] = ib_g;
    }
    if (!a.sl) {
        double sS = a.ybar[r], sI = a.ybar[rows + r];
        for (int t = 6; t >= 1; --t) {
            const double* yb = a.yst + (size_t)(t - 1) * 2 * rows;
            sS += yb[r];
            sI += (t == a.sg) ? ib_g : yb[rows + r];
        }
        a.ybar[r] = sS; a.ybar[rows + r] = sI;
        return;
    }
    double kbS = 0.0, kbI = 0.0;
    for (int t = 7; t > a.sl; --t) {
        const double* yb = (t == 7) ? a.ybar : a.yst + (size_t)(t - 1) * 2 * rows;
        kbS += a.hc[t] * yb[r];
        kbI += a.hc[t] * ((t == a.sg) ? ib_g : yb[rows + r]);
    }
    const double kbR = a.hc[7] * a.ybar[2 * (size_t)rows + r];
    const double d = kbI - kbS, e = kbR - kbI;
    const double S = a.Y[r], bet = BETA ? a.beta[r] : 1.0;
    const double* I = a.Y + rows + base;
    const double c = d * bet * S;
    a.c_cur[r] = c;
    const double ai = mfb_row_dot<W>(a.col, a.w_in, I, lo, hi);
    double* yb = a.yst + (size_t)(a.sl - 1) * 2 * rows;
    yb[r] = d * bet * ai;
    yb[rows + r] = e * a.gamma[r];                                    // the row's share of Ibar; the next launch adds the gather
    if (a.gb) a.gb[r] += d * ai * S;
    if (a.gg) a.gg[r] += e * I[v];
}

// ybar += grad_out[to]  (S, I, R planes from gS, gI, gR rows of [n_out][rows])
__global__ __launch_bounds__(256) void k_mfb_add_out(const double* __restrict__ gS, const double* __restrict__ gI,
                                                    const double* __restrict__ gR, int rows, double* __restrict__ ybar) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    ybar[r] += gS[r]; ybar[rows + r] += gI[r]; ybar[2 * (size_t)rows + r] += gR[r];
}

// y = the forward's output row: [S | I | R] planes
__global__ __launch_bounds__(256) void k_mfb_load_state(const double* __restrict__ oS, const double* __restrict__ oI,
                                                       const double* __restrict__ oR, int rows, double* __restrict__ y) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    y[r] = oS[r]; y[rows + r] = oI[r]; y[2 * (size_t)rows + r] = oR[r];
}

// grad_init[r][c] = ybar[c][r]
__global__ __launch_bounds__(256) void k_mfb_emit_init(const double* __restrict__ ybar, int rows, double* __restrict__ grad_init) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    for (int c = 0; c < 3; ++c) grad_init[(size_t)r * 3 + c] = ybar[(size_t)c * rows + r];
}

extern "C" size_t gnode_meanfield_rates_backward_workspace_bytes(gnode_graph_t g, int32_t B, int32_t max_interval_steps) {
    if (!g || B < 1 || max_interval_steps < 0) return 0;
    return mf_bwd_layout((int64_t)B * g->info.n, g->nnz, max_interval_steps).bytes;
}

extern "C" int gnode_meanfield_rates_backward_f64(gnode_graph_t g, int32_t B, const double* init, const double* beta, const double* w,
                                                  const double* gamma, const double* t_out_host, int32_t n_out, const double* h_host,
                                                  int64_t n_h, const int32_t* n_acc_host, const double* outI, const double* outS,
                                                  const double* outR, const double* gI, const double* gS, const double* gR,
                                                  double* grad_init, double* grad_beta, double* grad_w, double* grad_gamma,
                                                  void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "gnode_meanfield_rates_backward_f64";
    GN_CHECK_ARG(g && init && gamma && t_out_host && n_acc_host && outI && outS && outR && gI && gS && gR && workspace && n_h >= 0 &&
                 (h_host || n_h == 0), "%s: null pointer", who);
    GN_CHECK_ARG(grad_init || grad_beta || grad_w || grad_gamma, "%s: no gradient is asked for", who);
    GN_CHECK_ARG(B >= 1 && (int64_t)B * g->info.n <= INT32_MAX / 3, "%s: need 1 <= B and 3 * B * n < 2^31", who);
    GN_CHECK_ARG(n_out >= 1 && t_out_host[0] == 0.0, "%s: need output times starting at 0", who);
    for (int i = 1; i < n_out; ++i)
        GN_CHECK_ARG(t_out_host[i] >= t_out_host[i - 1], "%s: output times must be ascending", who);
    GN_CHECK_ARG(g->symmetric, "%s: the sparsity pattern is not symmetric (the transpose gather needs every contact's reverse entry)", who);
    const MfStepPlan plan = mf_check_steps(who, t_out_host, n_out, h_host, n_h, n_acc_host);
    GN_CHECK_ARG(plan.error.empty(), "%s", plan.error.c_str());
    const int rows = B * g->info.n;
    const MfBwdLayout L = mf_bwd_layout(rows, g->nnz, plan.max_interval_steps);
    if (workspace_bytes < L.bytes) {
        gnode_set_error("%s: workspace %zu < %zu", who, workspace_bytes, L.bytes);
        return GNODE_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const long len = 3L * rows;
    const size_t vd = gn_align((size_t)len * sizeof(double)) / sizeof(double);   // doubles per state slot
    char* ws = (char*)workspace;
    double* ybar = (double*)(ws + L.ybar);
    double* ystage = (double*)(ws + L.ystage);
    double* K = (double*)(ws + L.k);
    double* cbuf[2] = {(double*)(ws + L.c), (double*)(ws + L.c) + gn_align((size_t)rows * sizeof(double)) / sizeof(double)};
    double* store = (double*)(ws + L.store);
    const unsigned ng = (unsigned)((rows + 255) / 256);
    const bool has_w = w && g->nnz > 0;
    const double* w_in = nullptr;
    if (has_w) {
        if (int rc = gn_mf_stage_w_in(g, w, (double*)(ws + L.w_in), st)) return rc;
        w_in = (const double*)(ws + L.w_in);
    }
    GnZeroRegions z;
    z.n = 0;
    auto zero = [&](void* p, size_t bytes) { if (p && bytes) { z.p[z.n] = p; z.bytes[z.n] = bytes; ++z.n; } };
    zero(ybar, (size_t)len * sizeof(double));
    zero(grad_beta, (size_t)rows * sizeof(double));
    zero(grad_gamma, (size_t)rows * sizeof(double));
    zero(grad_w, (size_t)B * g->nnz * sizeof(double));
    if (int rc = gn_zero_regions_async(z, st)) return rc;

    auto stage = has_w ? (beta ? k_mfb_stage<true, true> : k_mfb_stage<true, false>) : (beta ? k_mfb_stage<false, true> : k_mfb_stage<false, false>);
    auto rev = has_w ? (beta ? k_mfb_rev<true, true> : k_mfb_rev<true, false>) : (beta ? k_mfb_rev<false, true> : k_mfb_rev<false, false>);
    // stages 1 .. n_stages of the step from `y`: Y_2 .. Y_6 into ystage, Y_7 (with n_stages = 6) into `ynext`
    auto run_stages = [&](const double* y, double hh, int n_stages, double* ynext) {
        for (int j = 0; j < n_stages; ++j)
            hipLaunchKernelGGL(stage, dim3(ng), dim3(256), 0, st, g->rowptr, g->col, g->info.n, rows, beta, w_in, gamma,
                               j == 0 ? y : ystage + (size_t)(j - 1) * vd, y, K, j, mf_stage_coef(j + 1), hh,
                               j == 5 ? ynext : ystage + (size_t)j * vd);
    };
    MfbRev a;
    a.rowptr = g->rowptr; a.col = g->col; a.n = g->info.n; a.rows = rows; a.nnz = (long)g->nnz;
    a.beta = beta; a.w = has_w ? w : nullptr; a.w_in = w_in; a.gamma = gamma; a.ybar = ybar; a.yst = (double*)(ws + L.ybar_st);
    a.gb = grad_beta; a.gw = g->nnz > 0 ? grad_w : nullptr; a.gg = grad_gamma;

    int64_t at = n_h;
    for (int to = n_out - 1; to >= 1; --to) {
        hipLaunchKernelGGL(k_mfb_add_out, dim3(ng), dim3(256), 0, st, gS + (size_t)to * rows, gI + (size_t)to * rows, gR + (size_t)to * rows, rows, ybar);
        const int m = n_acc_host[to];
        if (m == 0) continue;
        at -= m;
        hipLaunchKernelGGL(k_mfb_load_state, dim3(ng), dim3(256), 0, st, outS + (size_t)(to - 1) * rows, outI + (size_t)(to - 1) * rows,
                           outR + (size_t)(to - 1) * rows, rows, store);
        for (int i = 0; i < m; ++i) run_stages(store + (size_t)i * vd, h_host[at + i], 6, store + (size_t)(i + 1) * vd);
        GN_LAUNCH_CHECK();
        for (int i = m - 1; i >= 0; --i) {
            const double hh = h_host[at + i];
            const double* y = store + (size_t)i * vd;
            if (i < m - 1) run_stages(y, hh, 5, nullptr);             // (the integration above left the last step's Y_2 .. Y_6)
            for (int l = 0; l < 7; ++l) {
                a.sg = l == 0 ? 0 : 7 - l;
                a.sl = 6 - l;
                a.Y = a.sl == 1 ? y : ystage + (size_t)std::max(a.sl - 2, 0) * vd;
                a.Yg = a.sg == 1 ? y : ystage + (size_t)std::max(a.sg - 2, 0) * vd;
                a.c_cur = cbuf[l & 1]; a.c_prev = cbuf[(l & 1) ^ 1];
                for (int t = 0; t < 8; ++t) a.hc[t] = (a.sl >= 1 && t > a.sl) ? hh * kMfA[t - 1][a.sl - 1] : 0.0;
                hipLaunchKernelGGL(rev, dim3(ng), dim3(256), 0, st, a);
            }
            GN_LAUNCH_CHECK();
        }
    }
    hipLaunchKernelGGL(k_mfb_add_out, dim3(ng), dim3(256), 0, st, gS, gI, gR, rows, ybar);
    if (grad_init) hipLaunchKernelGGL(k_mfb_emit_init, dim3(ng), dim3(256), 0, st, ybar, rows, grad_init);
    GN_LAUNCH_CHECK();
    return 0;
}
