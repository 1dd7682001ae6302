// The DMP recurrence, stated once for the marginals and their reverse sweep (gnode_dmp_batch.h: gnode_dmp.hip under constant
// rates, gnode_dmp_schedule.hip and gnode_dmp_schedule_bwd.hip under a rate schedule) and for the candidate sweeps
// (gnode_dmp_sweep.h: the source scores of gnode_dmp_source.hip, gnode_dmp_source_batch.hip, gnode_dmp_source_events.hip and
// the outbreak sizes of gnode_dmp_outbreak.hip): the four dmp_* functions below and nothing else, and their reverses, the
// dmp_rev_* functions after them.  They work on values and on pointers that are already the sample's own, in global memory or
// in LDS.  The library is built with -ffp-contract=off, so they round as written wherever they are inlined; their operand order
// is the reference's.  Behind them: the fixed-order fp64 sums, the source units' one-hot start and likelihood terms, and the
// LDS of a one-workgroup kernel.  The kernels, workspaces, preambles and launches are gnode_dmp_batch.h's (marginals and
// gradients) and gnode_dmp_sweep.h's (candidate sweeps).
#pragma once
#include "gnode_common.h"
#include <vector>

// t = 1 (dmp.py:104-121): theta_1 = 1 - w phi_0 + 1e-10, phi_0 = Pi0[src] (what 1 - Ps0 is when Pr0 = 0), Ps_e^{prev} = Ps0[src]
__device__ __forceinline__ void dmp_edge_start(float ps0_u, float pi0_u, float w_e, float& theta, float& phi, float& ps) {
    theta = (1.0f - w_e * pi0_u) + 1e-10f;
    phi = pi0_u;
    ps = ps0_u;
}

// P_k: theta of the reverses of row k's edges [lo, hi), in ascending position from 1
__device__ __forceinline__ float dmp_row_product(const int* rev, const float* theta, int lo, int hi) {
    float p = 1.0f;
    for (int e = lo; e < hi; ++e) p = p * theta[rev[e]];
    return p;
}

// the marginals of node k at this step from P_k and the previous step's Pi_k, Pr_k
__device__ __forceinline__ void dmp_node_update(float P_k, float ps0_k, float pi_prev, float pr_prev, float gamma_k, float& ps,
                                                float& pi, float& pr) {
    ps = ps0_k * P_k;
    pr = pr_prev + gamma_k * pi_prev;
    pi = 1.0f - ps - pr;
}

// Ps_e and phi_e of this step (in place), theta_e of the NEXT step; `theta` is a reference so that it is loaded where it is
// used.  Two weights (rates that change over time; under constant rates both are the edge's one): phi_t is what survived THIS
// step, so it takes this step's w_e and gamma_u; theta_{t+1} - theta_t is what is transmitted DURING the next step, so it takes
// the next step's w_next.
__device__ __forceinline__ void dmp_edge_update(float P_u, float theta_rev, float ps0_u, float w_e, float w_next, float gamma_u, float& phi,
                                                float& ps, const float& theta, float& theta_next) {
    const float mul = P_u / theta_rev;
    const float ps_new = ps0_u * mul;
    const float ph = (1.0f - w_e) * (1.0f - gamma_u) * phi - (ps_new - ps);
    phi = ph;
    ps = ps_new;
    theta_next = theta - w_next * ph;
}
// constant rates: both weights are the edge's one
__device__ __forceinline__ void dmp_edge_update(float P_u, float theta_rev, float ps0_u, float w_e, float gamma_u, float& phi,
                                                float& ps, const float& theta, float& theta_next) {
    dmp_edge_update(P_u, theta_rev, ps0_u, w_e, w_e, gamma_u, phi, ps, theta, theta_next);
}

// The reverse of the recurrence, for gnode_dmp_batch.h's sweep under constant rates and under a schedule; what the adjoints are
// and why nothing is atomic is told where that sweep begins.
// the reverse of dmp_edge_update at step t for one edge: theta_bar is that of theta_{t+1}; phi_bar, q_bar come in as step
// t + 1 left them and go out for step t - 1.  q_tot (the adjoint of Ps_e of this step) and gamma_part (this edge's share of
// gamma_bar[src]) are for the node pass.  Two weights and two w_bar targets, as dmp_edge_update has two weights:
// theta_{t+1} = theta_t - w_next phi_t gives ITS weight's adjoint, w_bar_next, the term
// phi_t theta_bar, and phi_t's own weight and gamma are this step's.  The two targets may be one slot (the phases of steps t and
// t + 1 are equal, or the rates are constant): the two updates then happen in the order written.
__device__ __forceinline__ void dmp_rev_edge(float w_e, float w_next, float gamma_u, float phi_t, float phi_prev, float theta_bar,
                                             float& phi_bar, float& q_bar, float& w_bar, float& w_bar_next, float& q_tot,
                                             float& gamma_part) {
    const float pb = phi_bar - w_next * theta_bar;              // the adjoint of phi_t: theta_{t+1} = theta_t - w_next phi_t
    w_bar_next = w_bar_next - phi_t * theta_bar;
    w_bar = w_bar - ((1.0f - gamma_u) * phi_prev) * pb;         // phi_t = (1 - w)(1 - gamma) phi_{t-1} - (Ps_e - Ps_e^{prev})
    gamma_part = -(((1.0f - w_e) * phi_prev) * pb);
    q_tot = q_bar - pb;
    q_bar = pb;
    phi_bar = ((1.0f - w_e) * (1.0f - gamma_u)) * pb;
}
// constant rates: both weights are the edge's one, and both targets its one slot
__device__ __forceinline__ void dmp_rev_edge(float w_e, float gamma_u, float phi_t, float phi_prev, float theta_bar, float& phi_bar,
                                             float& q_bar, float& w_bar, float& q_tot, float& gamma_part) {
    dmp_rev_edge(w_e, w_e, gamma_u, phi_t, phi_prev, theta_bar, phi_bar, q_bar, w_bar, w_bar, q_tot, gamma_part);
}

// what row u's edges [lo, hi) hand to their source: S = sum c_bar c, the shares of ps0_bar[u] and of gamma_bar[u]
struct DmpRowSums { float S, ps0, gamma; };
__device__ __forceinline__ DmpRowSums dmp_rev_row_sums(const int* rev, const float* theta, const float* q_tot, const float* gamma_part,
                                                       int lo, int hi, float P_u, float ps0_u) {
    DmpRowSums s = {0.0f, 0.0f, 0.0f};
    for (int e = lo; e < hi; ++e) {
        const float c = P_u / theta[rev[e]];                    // the cavity product, as dmp_edge_update divides
        s.ps0 = s.ps0 + c * q_tot[e];
        s.S = s.S + (ps0_u * q_tot[e]) * c;
        s.gamma = s.gamma + gamma_part[e];
    }
    return s;
}

// the reverse of dmp_node_update for node k at step t: (gS, gI, gR) is grad_out's row, pi_prev the forward's Pi_{t-1}[k]
__device__ __forceinline__ void dmp_rev_node(float gS, float gI, float gR, float P_k, float ps0_k, float pi_prev, float gamma_k,
                                             float& pi_bar, float& pr_bar, float& gamma_bar, float& ps0_bar, float& P_bar) {
    const float aI = gI + pi_bar;
    const float aR = (gR + pr_bar) - aI;                        // pi = 1 - ps - pr
    const float aS = gS - aI;
    gamma_bar = gamma_bar + pi_prev * aR;                       // pr = pr_prev + gamma pi_prev
    pr_bar = aR;
    pi_bar = gamma_k * aR;
    ps0_bar = ps0_bar + P_k * aS;                               // ps = ps0 P
    P_bar = ps0_k * aS;
}

// theta_bar of step t for the reverses of row u's edges: the carried theta_bar plus the derivative of P_u and of the other
// edges' cavity products.  q_tot == nullptr: there was no edge pass (t = maxTime - 1, S = 0).
__device__ __forceinline__ void dmp_rev_theta(const int* rev, const float* theta, const float* q_tot, int lo, int hi, float P_u,
                                              float ps0_u, float PbarP, float S, const float* tb_cur, float* tb_next) {
    for (int f = lo; f < hi; ++f) {
        const int r = rev[f];
        const float th = theta[r];
        const float own = q_tot ? (ps0_u * q_tot[f]) * (P_u / th) : 0.0f;
        tb_next[r] = tb_cur[r] + ((PbarP + S) - own) / th;
    }
}

struct DmpAdjoint {                     // sample b's own adjoint state, in the workspace or in LDS
    float *tb, *tb_next, *phb, *qb, *q_tot, *gamma_part, *pib, *prb;      // tb: theta_bar as the step finds it, tb_next: as it leaves it
};
__host__ __device__ static inline void dmp_adjoint_swap(DmpAdjoint& A) { float* t = A.tb; A.tb = A.tb_next; A.tb_next = t; }

// The fp64 sums of gnode_dmp_source.hip and gnode_dmp_outbreak.hip, in a fixed order.  The sum of the 64 lanes' values in lane 0:
// a fixed tree, 32 16 8 4 2 1 (every lane of the wave is active where this is called)
__device__ __forceinline__ double dmp_wave_sum(double v) {
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off, 64);
    return v;
}
__device__ __forceinline__ double dmp_sum_in_order(const double* v, int count) {
    double s = 0.0;
    for (int i = 0; i < count; ++i) s = s + v[i];
    return s;
}

// Source inference (the readers of gnode_dmp_source.hip, gnode_dmp_source_batch.hip, gnode_dmp_source_events.hip).  The start of node k in the sample of candidate `cand`:
// (1 - seed, seed, 0) like k_dmp_seed_out0; Pr_0 = 0
__device__ __forceinline__ void dmp_source_state(int k, int cand, float& ps0, float& pi0) {
    const float seed = k == cand ? 1.0f : 0.0f;
    ps0 = 1.0f - seed;
    pi0 = seed;
}

// the log-likelihood term of a node observed in state o; anything but 0 / 1 / 2 is "not observed"
__device__ __forceinline__ double dmp_source_term(int o, float ps, float pi, float pr, float floor) {
    if ((unsigned)o > 2u) return 0.0;
    const float p = o == 0 ? ps : o == 1 ? pi : pr;
    return log((double)fminf(fmaxf(p, floor), 1.0f));
}

// The same term for many observations of one node: its three possible values, once, and the choice among them by an
// observation's code -- the double dmp_source_term(o, ...) returns, selected and never indexed.
struct DmpSourceLogs { double s, i, r; };
__device__ __forceinline__ DmpSourceLogs dmp_source_logs(float ps, float pi, float pr, float floor) {
    return {log((double)fminf(fmaxf(ps, floor), 1.0f)), log((double)fminf(fmaxf(pi, floor), 1.0f)),
            log((double)fminf(fmaxf(pr, floor), 1.0f))};
}
__device__ __forceinline__ double dmp_source_pick(int o, const DmpSourceLogs& l) {
    return o == 0 ? l.s : o == 1 ? l.i : o == 2 ? l.r : 0.0;
}

// With the two event terms (gnode_dmp_source_events.hip): node k became infected AT this step with p = Ps(t-1) - Ps(t), and
// recovered AT it with p = Pr(t) - Pr(t-1); ps_prev, pr_prev are the previous step's marginals, (1, 0) before the start.  The
// first three are dmp_source_logs' doubles, so a row of codes 0 / 1 / 2 selects what dmp_source_pick selects.
struct DmpSourceEventLogs { double s, i, r, on, off; };
__device__ __forceinline__ DmpSourceEventLogs dmp_source_event_logs(float ps, float pi, float pr, float ps_prev, float pr_prev,
                                                                    float floor) {
    const DmpSourceLogs l = dmp_source_logs(ps, pi, pr, floor);
    return {l.s, l.i, l.r, log((double)fminf(fmaxf(ps_prev - ps, floor), 1.0f)), log((double)fminf(fmaxf(pr - pr_prev, floor), 1.0f))};
}
__device__ __forceinline__ double dmp_source_event_pick(int o, const DmpSourceEventLogs& l) {
    return o == 0 ? l.s : o == 1 ? l.i : o == 2 ? l.r : o == 3 ? l.on : o == 4 ? l.off : 0.0;
}

// The P tables of a scheduled call (gnode_dmp_batch.h's dmp_stage_schedule, gnode_dmp_sweep.h's dmp_sweep_run) are
// probabilities, and they live on the device: they come back once, on the caller's stream (which the call synchronises anyway),
// and the first entry that is a NaN or outside [0, 1] is named by sample, phase and position.  Nothing has been written when
// this refuses.  `samples`: 1 for a shared table (stride 0), else B.  Host code.
static inline int dmp_check_rate_tables(const char* who, const char* what, const float* dev, size_t samples, size_t P, size_t len, hipStream_t st) {
    std::vector<float> host(samples * P * len);
    if (host.empty()) return 0;
    GN_HIP(hipMemcpyAsync(host.data(), dev, host.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    GN_HIP(hipStreamSynchronize(st));
    for (size_t i = 0; i < host.size(); ++i)
        GN_CHECK_ARG(host[i] >= 0.0f && host[i] <= 1.0f, "%s: sample %zu, phase %zu: %s[%zu] = %g is not in [0,1]", who, i / (P * len),
                     (i / len) % P, what, i % len, (double)host[i]);          // (a NaN fails both comparisons)
    return 0;
}

__host__ __device__ static inline size_t dmp_align16(size_t x) { return (x + 15) / 16 * 16; }
static constexpr size_t kDmpLdsLimit = 160 * 1024;      // what a gfx950 workgroup may declare

// The LDS of a one-workgroup kernel's sample, carved from the kernel's dynamic LDS: theta x2, phi, ps, rev over the edges | P,
// Pi, Pr over the nodes (gnode_dmp_batch_lds_bytes), and `rest`, whatever the kernel declares behind them.
// (gnode_dmp_batch.h's k_dmp_batch_wg carves the same by hand, with theta[2] indexed: through this struct, which selects theta,
// its constant instance takes 23 VGPRs and its scheduled one 24 where both have 22 -- tried when they were restated over a
// rates policy)
struct DmpLds {
    float *theta0, *theta1, *phi, *ps;
    int* rev;
    float *P, *Pi, *Pr;
    char* rest;
    __device__ __forceinline__ float* theta(int i) const { return i ? theta1 : theta0; }       // (selected, not indexed: the struct stays in registers)
};
__device__ __forceinline__ DmpLds dmp_lds(char* smem, int n, int nnz) {
    const size_t eb = dmp_align16((size_t)nnz * 4), nb = dmp_align16((size_t)n * 4);
    return {(float*)smem, (float*)(smem + eb), (float*)(smem + 2 * eb), (float*)(smem + 3 * eb), (int*)(smem + 4 * eb),
            (float*)(smem + 5 * eb), (float*)(smem + 5 * eb + nb), (float*)(smem + 5 * eb + 2 * nb), smem + 5 * eb + 3 * nb};
}
