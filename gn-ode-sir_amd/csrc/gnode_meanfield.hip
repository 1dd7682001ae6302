// Mean-field SIR baseline on MI355X (gfx950) -- SURVEY 8f rank 4.
//
// The reference integrates  dS = -beta (A I) * S,  dI = beta (A I) * S - gamma * I,  dR = gamma * I  (ode_nn.py:214-220,
// `sir`) with scipy's LSODA on the DENSE adjacency and samples it at t = 0, 1, .., maxTime-1 (`runge_kutta_order4`,
// :222-233).  Here: float64 state on the device, A I as a CSR sparse mat-vec, and an adaptive Dormand-Prince 5(4)
// pair whose steps are clipped to land exactly on the output times.  The step-size control runs on the host (one
// 8-byte error norm per step comes back); tolerances default far below LSODA's own (rtol = atol = 1.5e-8), so the
// two agree to ~1e-7 -- the test tolerance is 1e-6 absolute on probabilities.
#include "gnode_meanfield.h"
#include <algorithm>
#include <cmath>
#include <cstring>

// ytmp = y + h * sum_j c_j k_j        (3n doubles; k_j = K + j * 3n)
__global__ __launch_bounds__(256) void k_mf_comb(const double* __restrict__ y, const double* __restrict__ K, MfCoef cf, double h,
                                                long len, double* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    out[i] = mf_comb_at(y, K, cf, h, len, i);
}

// k = f(y) for B samples on one graph, one thread per row r = b * n + v of the [3][B * n] state (the scalar entries: B = 1,
// rows = n).  Row r gathers from its own sample's I; w_in[p] is the weight of the contact col[p] -> v, gamma is [B][n].  The
// infection rate is beta[r] with BETA, else the one number beta_s: the scalar entries' beta, and 1.0 (an exact factor) for
// gnode_meanfield_rates_f64 without a beta array.
template <bool W, bool BETA>
__global__ __launch_bounds__(256) void k_mf_rhs_rates(const int* __restrict__ rowptr, const int* __restrict__ col, int n, int rows,
                                                     const double* __restrict__ beta, double beta_s, const double* __restrict__ w_in,
                                                     const double* __restrict__ gamma, const double* __restrict__ y,
                                                     double* __restrict__ k) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    double inf, rec;
    mf_rhs_row<W, BETA>(rowptr, col, n, rows, r, beta, beta_s, w_in, gamma, y, &inf, &rec);
    k[r] = -inf; k[rows + r] = inf - rec; k[2 * (size_t)rows + r] = rec;
}

// w_in[p] = w[rev[p]]: the weight of the contact col[p] -> v for position p of row v (w is source = row, target = column).
// rev is the handle's table of a symmetric pattern (every entry >= 0); a self-loop is its own reverse.
__global__ __launch_bounds__(256) void k_mf_w_in(const int* __restrict__ rev, long nnz, const double* __restrict__ w,
                                                double* __restrict__ w_in) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p < nnz) w_in[p] = w[rev[p]];
}

int gn_mf_stage_w_in(const gnode_graph_s* g, const double* w, double* w_in, hipStream_t st) {
    hipLaunchKernelGGL(k_mf_w_in, dim3((unsigned)((g->nnz + 255) / 256)), dim3(256), 0, st, g->rev, (long)g->nnz, w, w_in);
    GN_LAUNCH_CHECK();
    return 0;
}

// err = max_i |h sum_j e_j k_j| / (atol + rtol max(|y_i|, |ynew_i|))   (non-negative doubles order like their bits)
__global__ __launch_bounds__(256) void k_mf_err(const double* __restrict__ y, const double* __restrict__ ynew,
                                               const double* __restrict__ K, MfCoef ef, double h, double rtol, double atol,
                                               long len, unsigned long long* __restrict__ err_bits) {
    __shared__ double red[256];
    double m = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < len; i += (long)gridDim.x * 256) {
        double s = 0.0;
        for (int j = 0; j < ef.n; ++j) s += ef.c[j] * K[(size_t)j * len + i];
        const double sc = atol + rtol * fmax(fabs(y[i]), fabs(ynew[i]));
        m = fmax(m, fabs(h * s) / sc);
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(err_bits, (unsigned long long)__double_as_longlong(red[0]));
}

__global__ __launch_bounds__(256) void k_mf_init(const double* __restrict__ seed, int n, double* __restrict__ y) {
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= n) return;
    y[u] = 1.0 - seed[u]; y[n + u] = seed[u]; y[2 * (size_t)n + u] = 0.0;
}

// gnode_meanfield_init_f64: y(0) = the caller's [n][3] = (pS, pI, pR)
__global__ __launch_bounds__(256) void k_mf_init_state(const double* __restrict__ init, int n, double* __restrict__ y) {
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= n) return;
    y[u] = init[(size_t)u * 3]; y[n + u] = init[(size_t)u * 3 + 1]; y[2 * (size_t)n + u] = init[(size_t)u * 3 + 2];
}

// out rows (I, S, R order of the reference's return value, ode_nn.py:233): out[c][t][u]
__global__ __launch_bounds__(256) void k_mf_emit(const double* __restrict__ y, int n, int t, int T, double* __restrict__ outI,
                                                double* __restrict__ outS, double* __restrict__ outR) {
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= n) return;
    outS[(size_t)t * n + u] = y[u]; outI[(size_t)t * n + u] = y[n + u]; outR[(size_t)t * n + u] = y[2 * (size_t)n + u];
}

// rows = the state's rows: n, or B * n of the rates entry
static size_t mf_workspace_bytes(size_t rows) {
    const size_t v = gn_align(3 * rows * sizeof(double));
    return 10 * v + gn_align(rows * sizeof(double)) + 256;                   // y, ynew, ytmp, K[7] | seed | err
}

extern "C" size_t gnode_meanfield_workspace_bytes(gnode_graph_t g) {
    if (!g) return 0;
    return mf_workspace_bytes((size_t)g->info.n);
}

extern "C" size_t gnode_meanfield_rates_workspace_bytes(gnode_graph_t g, int32_t B) {
    if (!g || B < 1) return 0;
    return mf_workspace_bytes((size_t)B * g->info.n) + gn_align((size_t)std::max<int64_t>(g->nnz, 1) * sizeof(double));   // ... | w_in
}

// gnode_meanfield_rates_f64's part of a call: B samples, beta device [B][n] or null = 1, w device [nnz] or null = 1
struct MfRates { int B; const double* beta; const double* w; };
// gnode_meanfield_rates_steps_f64's record of the accepted steps: their sizes in order (the first `cap` of them), how many there
// were, and how many carried t_out[to - 1] to t_out[to]
struct MfRecord { double* h; int64_t cap; int64_t n; int32_t* n_acc; };

// `who`: the entry's name for the messages.  init: device fp64 [n][3] (gnode_meanfield_init_f64), or null: then the seed list holds.
// rates: null for the scalar entries; else init is [B][n][3], gamma [B][n], the scalar beta rests and the state has B * n rows.
static int meanfield_impl(const char* who, gnode_graph_t g, const int32_t* seeds_host, int32_t n_seeds, const double* init, double beta,
                          const double* gamma, const double* t_out_host, int32_t n_out, double rtol, double atol,
                          double* outI, double* outS,
                          double* outR, int64_t* steps_host, void* workspace, size_t workspace_bytes, void* stream,
                          const MfRates* rates = nullptr, MfRecord* rec = nullptr) {
    GN_CHECK_ARG(g && gamma && outI && outS && outR && workspace && (init || seeds_host || n_seeds == 0), "%s: null pointer", who);
    GN_CHECK_ARG(!rates || (rates->B >= 1 && (int64_t)rates->B * g->info.n <= INT32_MAX / 3), "%s: need 1 <= B and 3 * B * n < 2^31", who);
    GN_CHECK_ARG(t_out_host && n_out >= 1 && t_out_host[0] == 0.0, "%s: need output times starting at 0", who);
    for (int i = 1; i < n_out; ++i)
        GN_CHECK_ARG(t_out_host[i] >= t_out_host[i - 1], "%s: output times must be ascending", who);
    GN_CHECK_ARG(rtol > 0 && atol > 0, "%s: tolerances must be positive", who);
    for (int i = 0; i < n_seeds; ++i)
        GN_CHECK_ARG(seeds_host[i] >= 0 && seeds_host[i] < g->info.n, "%s: seed %d out of range", who, seeds_host[i]);
    const size_t need = rates ? gnode_meanfield_rates_workspace_bytes(g, rates->B) : gnode_meanfield_workspace_bytes(g);
    if (workspace_bytes < need) {
        gnode_set_error("%s: workspace %zu < %zu", who, workspace_bytes, need);
        return GNODE_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const int n = (rates ? rates->B : 1) * g->info.n;                 // rows of the state
    const long len = 3L * n;
    const size_t v = gn_align((size_t)len * sizeof(double));
    char* ws = (char*)workspace;
    double* y = (double*)ws; double* ynew = (double*)(ws + v); double* ytmp = (double*)(ws + 2 * v);
    double* K = (double*)(ws + 3 * v);                                // K[j] = K + j * len needs contiguity in `len` units
    double* seed = (double*)(ws + 10 * v);
    unsigned long long* err = (unsigned long long*)(ws + 10 * v + gn_align((size_t)n * sizeof(double)));
    // K is indexed K[j * len + i]: lay the 7 stages out back to back in elements (7 * len doubles fit in 7 aligned slots)
    const unsigned ng = (unsigned)((n + 255) / 256), lg = (unsigned)((len + 255) / 256);
    const double* beta_rows = rates ? rates->beta : nullptr;          // [B][n], or null: the scalar beta (1 for the rates entry)
    const double* w_in = nullptr;
    if (rates && rates->w && g->nnz > 0) {                            // before anything is written to the outputs
        GN_CHECK_ARG(g->symmetric, "%s: the sparsity pattern is not symmetric (a directed contact is a zero weight on the reverse entry)", who);
        double* tab = (double*)(ws + mf_workspace_bytes((size_t)n));
        if (int rc = gn_mf_stage_w_in(g, rates->w, tab, st)) return rc;
        w_in = tab;
    }
    const double one = 1.0;
    if (init) {
        hipLaunchKernelGGL(k_mf_init_state, dim3(ng), dim3(256), 0, st, init, n, y);
    } else {
        GN_HIP(hipMemsetAsync(seed, 0, (size_t)n * sizeof(double), st));
        for (int i = 0; i < n_seeds; ++i) GN_HIP(hipMemcpyAsync(seed + seeds_host[i], &one, sizeof(double), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_mf_init, dim3(ng), dim3(256), 0, st, seed, n, y);
    }
    hipLaunchKernelGGL(k_mf_emit, dim3(ng), dim3(256), 0, st, y, n, 0, n_out, outI, outS, outR);
    GN_LAUNCH_CHECK();
    GN_HIP(hipStreamSynchronize(st));                                 // `one` / seeds_host are done with

    auto rhs = [&](const double* yy, double* kk) {
        auto kern = w_in ? (beta_rows ? k_mf_rhs_rates<true, true> : k_mf_rhs_rates<true, false>)
                         : (beta_rows ? k_mf_rhs_rates<false, true> : k_mf_rhs_rates<false, false>);
        hipLaunchKernelGGL(kern, dim3(ng), dim3(256), 0, st, g->rowptr, g->col, g->info.n, n, beta_rows, rates ? 1.0 : beta, w_in, gamma, yy, kk);
    };
    rhs(y, K);                                                        // k1 (FSAL: later steps reuse k7)
    double t = 0.0, h = 1e-3;
    long steps = 0;
    if (rec) std::fill(rec->n_acc, rec->n_acc + n_out, 0);
    for (int to = 1; to < n_out; ++to) {
        const double t_end = t_out_host[to];
        while (t < t_end) {
            const double hh = std::min(h, t_end - t);
            for (int s = 1; s < 7; ++s) {
                const MfCoef cf = mf_stage_coef(s);
                double* dst = (s == 6) ? ynew : ytmp;                 // stage 7's argument IS the 5th-order solution
                hipLaunchKernelGGL(k_mf_comb, dim3(lg), dim3(256), 0, st, y, K, cf, hh, len, dst);
                rhs(dst, K + (size_t)s * len);
            }
            MfCoef ef; ef.n = 7;
            for (int j = 0; j < 7; ++j) ef.c[j] = (j < 6 ? kMfA[6][j] : 0.0) - kMfB4[j];
            GN_HIP(hipMemsetAsync(err, 0, sizeof(unsigned long long), st));
            hipLaunchKernelGGL(k_mf_err, dim3((unsigned)std::min<long>(lg, 1024)), dim3(256), 0, st, y, ynew, K, ef, hh, rtol, atol,
                               len, err);
            GN_LAUNCH_CHECK();
            unsigned long long eb = 0;
            GN_HIP(hipMemcpyAsync(&eb, err, sizeof(eb), hipMemcpyDeviceToHost, st));
            GN_HIP(hipStreamSynchronize(st));
            double e;
            memcpy(&e, &eb, sizeof(e));
            GN_CHECK_ARG(std::isfinite(e), "%s: non-finite state at t=%g", who, t);
            ++steps;
            GN_CHECK_ARG(steps < 2000000, "%s: step count exploded (h=%g at t=%g)", who, hh, t);
            if (e <= 1.0) {                                           // accept
                if (rec) {
                    if (rec->n < rec->cap) rec->h[rec->n] = hh;
                    ++rec->n; ++rec->n_acc[to];
                }
                t = (hh == t_end - t) ? t_end : t + hh;
                std::swap(y, ynew);
                GN_HIP(hipMemcpyAsync(K, K + (size_t)6 * len, (size_t)len * sizeof(double), hipMemcpyDeviceToDevice, st));   // FSAL
            }
            const double fac = (e == 0.0) ? 5.0 : std::min(5.0, std::max(0.2, 0.9 * std::pow(e, -0.2)));
            h = hh * fac;
        }
        hipLaunchKernelGGL(k_mf_emit, dim3(ng), dim3(256), 0, st, y, n, to, n_out, outI, outS, outR);
        GN_LAUNCH_CHECK();
    }
    if (steps_host) *steps_host = steps;
    return 0;
}

extern "C" int gnode_meanfield_f64(gnode_graph_t g, const int32_t* seeds_host, int32_t n_seeds, double beta,
                                   const double* gamma, const double* t_out_host, int32_t n_out, double rtol, double atol,
                                   double* outI, double* outS,
                                   double* outR, int64_t* steps_host, void* workspace, size_t workspace_bytes, void* stream) {
    return meanfield_impl("gnode_meanfield_f64", g, seeds_host, n_seeds, nullptr, beta, gamma, t_out_host, n_out, rtol, atol, outI, outS, outR, steps_host,
                          workspace, workspace_bytes, stream);
}

// The same integration from y(0) = init (device fp64 [n][3]); the workspace is gnode_meanfield_workspace_bytes'.
extern "C" int gnode_meanfield_init_f64(gnode_graph_t g, const double* init, double beta, const double* gamma,
                                        const double* t_out_host, int32_t n_out, double rtol, double atol, double* outI,
                                        double* outS, double* outR, int64_t* steps_host, void* workspace, size_t workspace_bytes,
                                        void* stream) {
    GN_CHECK_ARG(init, "gnode_meanfield_init_f64: null pointer");
    return meanfield_impl("gnode_meanfield_init_f64", g, nullptr, 0, init, beta, gamma, t_out_host, n_out, rtol, atol, outI, outS, outR, steps_host, workspace,
                          workspace_bytes, stream);
}

// B samples on one graph with per-sample, per-node beta and gamma and per-contact weights: see include/gnode.h.
extern "C" int gnode_meanfield_rates_f64(gnode_graph_t g, int32_t B, const double* init, const double* beta, const double* w,
                                         const double* gamma, const double* t_out_host, int32_t n_out, double rtol, double atol,
                                         double* outI, double* outS, double* outR, int64_t* steps_host, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    GN_CHECK_ARG(init, "gnode_meanfield_rates_f64: null pointer");
    const MfRates rates = {B, beta, w};
    return meanfield_impl("gnode_meanfield_rates_f64", g, nullptr, 0, init, 0.0, gamma, t_out_host, n_out, rtol, atol, outI, outS, outR,
                          steps_host, workspace, workspace_bytes, stream, &rates);
}

// The same integration, and the accepted steps: what gnode_meanfield_rates_backward_f64 sweeps back over (include/gnode.h).
extern "C" int gnode_meanfield_rates_steps_f64(gnode_graph_t g, int32_t B, const double* init, const double* beta, const double* w,
                                               const double* gamma, const double* t_out_host, int32_t n_out, double rtol, double atol,
                                               double* outI, double* outS, double* outR, int64_t* steps_host, void* workspace,
                                               size_t workspace_bytes, void* stream, double* h_host, int64_t h_cap,
                                               int64_t* n_h_host, int32_t* n_acc_host) {
    GN_CHECK_ARG(init && n_h_host && n_acc_host && h_cap >= 0 && (h_host || h_cap == 0), "gnode_meanfield_rates_steps_f64: null pointer");
    const MfRates rates = {B, beta, w};
    MfRecord rec = {h_host, h_cap, 0, n_acc_host};
    const int rc = meanfield_impl("gnode_meanfield_rates_steps_f64", g, nullptr, 0, init, 0.0, gamma, t_out_host, n_out, rtol, atol, outI, outS,
                                  outR, steps_host, workspace, workspace_bytes, stream, &rates, &rec);
    if (rc == 0) *n_h_host = rec.n;
    return rc;
}
