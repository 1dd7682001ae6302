// The DMP marginals of a batch of samples and their reverse sweep, stated once over a RATES policy: the kernels of both forms,
// the workspace, the preamble and the launches behind gnode_dmp_f32, gnode_dmp_init_f32, gnode_dmp_batch_f32 and
// gnode_dmp_batch_backward_f32, gnode_dmp_backward_f32 (gnode_dmp.hip: constant rates) and behind gnode_dmp_batch_schedule_f32
// and gnode_dmp_batch_schedule_backward_f32 (gnode_dmp_schedule.hip, gnode_dmp_schedule_bwd.hip: rates that change over time).
// The units instantiate; the recurrence and its reverse are gnode_dmp.h's functions and nothing else, called with the same
// operands whatever the policy.
//
// B samples on one graph, sample b starting from init[b] = (pS, pI, pR) per node with its tables at weights + b * w_stride and
// gamma + b * gamma_stride (a stride of 0 shares them).  Two forms, chosen by the graph's size alone:
//   general                    kernels over rows b * n + k and edge slots b * nnz + e of the workspace: two launches per time
//                              step (node pass, edge pass); theta ping-pongs because the edge pass reads its neighbours'
//   one workgroup per sample   the messages and marginals of a sample live in LDS for the whole horizon: one launch
// A sample's numbers do not depend on the form or on B: same expressions, same per-element order.
//
// RATES.  A sample's tables are w[tables][nnz] and gamma[tables][n], and no kernel indexes them but through DmpStepTables, the
// offsets of a step's tables inside them: step t's phi and Pr read step t's w and gamma, theta_{t+1} reads the weight of step
// t + 1 (gnode_dmp.h's two-weight dmp_edge_update and dmp_rev_edge), and theta_1 reads step 1's.  A policy R names
//   Args, GradArgs   what the forward's and the reverse sweep's kernels receive
//   kOneSlot         whether both weights of an edge pass are always one slot (a compile-time fact; else a run-time test)
//   tables(a)        how many tables of each kind a sample has: the per-sample stride of grad_w and grad_gamma in tables
//   step(a, t)       step t's offsets for the one-workgroup form, uniform over the workgroup
//   launch(a)        this launch's offsets for the general form, which set_step(a, phase, t) wrote into `a` on the host
//   head_bytes       the head of the workspace, before the carve's regions
//   HostSchedule     what the host side takes as the schedule: DmpSchedule, or DmpNoSchedule under constant rates
// DmpBatchConstantRates: one table of each kind, every offset a constant 0, so its instances are the kernels that gnode_dmp.hip
// held before the policy existed.  DmpBatchScheduledRates: P tables of each kind and a phase row, phase[t] in [0, P) naming
// step t's; the one-workgroup form reads the device copy of the row at the head of the workspace, uniformly, and the barriers
// stay in uniform control flow.  The tables stay in memory, never in LDS, so the forms are chosen by the same sizes whatever
// the rates are.
#pragma once
#include "gnode_dmp.h"
#include <algorithm>

struct DmpBatchArgs {
    const float* w; long w_stride;      // [tables][nnz] per sample, sample b at w + b * w_stride
    const float* gamma; long gamma_stride;
    const float* init;                  // [B][n][3]
    float* out;                         // [B][maxTime][n][3]
    int n, maxTime; long nnz;
};
struct DmpGradArgs {
    const float* w; long w_stride;
    const float* gamma; long gamma_stride;
    const float* init;                  // [B][n][3]
    const float* out;                   // [B][maxTime][n][3], the forward's
    const float* gout;                  // the same shape
    float *gw, *gg, *gi;                // [B][tables][nnz], [B][tables][n], [B][n][3]; null: not wanted
    float *th_tape, *ph_tape;           // [B][maxTime - 1][nnz]: theta_1 .. theta_{T-1} and phi_0 .. phi_{T-2}
    int n, maxTime; long nnz;
};

// Where a step's tables lie inside a sample's: w = phase[t] * nnz, w_next = phase[t + 1] * nnz (w again where t + 1 = maxTime:
// nothing reads it there), g = phase[t] * n.
struct DmpStepTables { long w, w_next, g; };

// A rate schedule as a scheduled entry receives it: the phase row [maxTime] on the host and the number of tables of each kind;
// and what a constant entry has in its place.  A policy names which of the two its host side takes (HostSchedule), so an
// instance cannot be called with the other's.
struct DmpSchedule { const int32_t* phase_host; int32_t P; };
struct DmpNoSchedule {};

struct DmpBatchConstantRates {
    using HostSchedule = DmpNoSchedule;
    static const DmpSchedule* schedule_of(const DmpNoSchedule&) { return nullptr; }
    using Args = DmpBatchArgs;
    using GradArgs = DmpGradArgs;
    static constexpr bool kScheduled = false, kOneSlot = true;
    template <class A> static __device__ __forceinline__ size_t tables(const A&) { return 1; }
    template <class A> static __device__ __forceinline__ DmpStepTables step(const A&, int) { return {0, 0, 0}; }
    template <class A> static __device__ __forceinline__ DmpStepTables launch(const A&) { return {0, 0, 0}; }
    template <class A> static void set_step(A&, const int32_t*, int) {}
    // room that no kernel uses any more (src, rev and a status word lay there while every call built them; the handle holds them
    // now): the size queries are pinned by tests/golden/dmp_parent.json and edge_tables_parent.json
    static size_t head_bytes(gnode_graph_t g, size_t) { return 2 * gn_align((size_t)std::max<int64_t>(g->nnz, 1) * 4) + 256; }
};
struct DmpBatchScheduledRates {
    struct Schedule {
        DmpStepTables at;               // the general form: the launch's step, set by the host loop
        const int32_t* phase;           // device int32 [maxTime], at the head of the workspace (the one-workgroup form reads it)
        int P;
    };
    struct Args : DmpBatchArgs, Schedule {};
    struct GradArgs : DmpGradArgs, Schedule {};
    using HostSchedule = DmpSchedule;
    static const DmpSchedule* schedule_of(const DmpSchedule& s) { return &s; }
    static constexpr bool kScheduled = true, kOneSlot = false;
    template <class A> static __device__ __forceinline__ size_t tables(const A& a) { return (size_t)a.P; }
    template <class A> static __host__ __device__ __forceinline__ DmpStepTables step(const A& a, const int32_t* phase, int t) {
        const long p = phase[t], p_next = t + 1 < a.maxTime ? phase[t + 1] : p;      // (maxTime >= 2: entry 1 exists)
        return {p * a.nnz, p_next * a.nnz, p * a.n};
    }
    template <class A> static __device__ __forceinline__ DmpStepTables step(const A& a, int t) { return step(a, a.phase, t); }
    template <class A> static __device__ __forceinline__ DmpStepTables launch(const A& a) { return a.at; }
    template <class A> static void set_step(A& a, const int32_t* phase_host, int t) { a.at = step(a, phase_host, t); }
    static size_t head_bytes(gnode_graph_t, size_t maxTime) { return gn_align(maxTime * sizeof(int32_t)); }
};

// ------------------------------------------------------------------------------------------------ the forward's kernels
struct DmpSample {                      // sample b's own tables: w, gamma, the start s0[n][3], out[maxTime][n][3]
    const float* __restrict__ w; const float* __restrict__ gamma; const float* __restrict__ s0; float* __restrict__ out;
};
__device__ __forceinline__ DmpSample dmp_sample(const DmpBatchArgs& a, size_t b) {
    return {a.w + b * a.w_stride, a.gamma + b * a.gamma_stride, a.init + b * (size_t)a.n * 3, a.out + b * (size_t)a.maxTime * a.n * 3};
}
__device__ __forceinline__ void dmp_store3(float* __restrict__ row, int k, float ps, float pi, float pr) {
    row[(size_t)k * 3 + 0] = ps; row[(size_t)k * 3 + 1] = pi; row[(size_t)k * 3 + 2] = pr;
}

// One workgroup = one sample, every step.  Thread `tid` owns nodes and edges tid, tid + blockDim.x, ... in both passes; the
// barriers sit in uniform control flow (the step loop's bounds are kernel arguments), so every thread reaches each of them.
template <class R>
__global__ __launch_bounds__(1024) void k_dmp_batch_wg(const int* __restrict__ rowptr, const int* __restrict__ src,
                                                      const int* __restrict__ rev_g, typename R::Args a) {
    extern __shared__ __attribute__((aligned(16))) char dmp_smem[];
    const int n = a.n, nnz = (int)a.nnz, tid = threadIdx.x, nt = blockDim.x;
    const size_t eb = dmp_align16((size_t)nnz * 4), nb = dmp_align16((size_t)n * 4);
    float* theta[2] = {(float*)dmp_smem, (float*)(dmp_smem + eb)};
    float* phi = (float*)(dmp_smem + 2 * eb); float* ps = (float*)(dmp_smem + 3 * eb);
    int* rev = (int*)(dmp_smem + 4 * eb);
    float* P = (float*)(dmp_smem + 5 * eb); float* Pi = (float*)(dmp_smem + 5 * eb + nb); float* Pr = (float*)(dmp_smem + 5 * eb + 2 * nb);
    const DmpSample s = dmp_sample(a, blockIdx.x);
    for (int k = tid; k < n; k += nt) {                                   // output row 0; Pi, Pr hold the start for step 1
        const float ps0 = s.s0[(size_t)k * 3], pi0 = s.s0[(size_t)k * 3 + 1], pr0 = s.s0[(size_t)k * 3 + 2];
        dmp_store3(s.out, k, ps0, pi0, pr0);
        Pi[k] = pi0; Pr[k] = pr0;
    }
    {
        const float* w1 = s.w + R::step(a, 1).w;
        for (int e = tid; e < nnz; e += nt) {
            const int u = src[e];
            dmp_edge_start(s.s0[(size_t)u * 3], s.s0[(size_t)u * 3 + 1], w1[e], theta[0][e], phi[e], ps[e]);
            rev[e] = rev_g[e];
        }
    }
    __syncthreads();
    for (int t = 1; t < a.maxTime; ++t) {
        const float* th = theta[(t - 1) & 1];
        float* th_next = theta[t & 1];
        const DmpStepTables at = R::step(a, t);
        const float* w = s.w + at.w;
        const float* gam = s.gamma + at.g;
        for (int k = tid; k < n; k += nt) {                               // node pass
            const float p = dmp_row_product(rev, th, rowptr[k], rowptr[k + 1]);
            P[k] = p;
            float sk, pi, pr;
            dmp_node_update(p, s.s0[(size_t)k * 3], Pi[k], Pr[k], gam[k], sk, pi, pr);
            Pr[k] = pr; Pi[k] = pi;
            dmp_store3(s.out + (size_t)t * n * 3, k, sk, pi, pr);
        }
        __syncthreads();                                                  // P is complete; theta[cur] is still this step's
        if (t + 1 < a.maxTime) {                                          // (the last step's messages have no reader)
            const float* w_next = s.w + at.w_next;
            for (int e = tid; e < nnz; e += nt) {                         // edge pass
                const int u = src[e];
                dmp_edge_update(P[u], th[rev[e]], s.s0[(size_t)u * 3], w[e], w_next[e], gam[u], phi[e], ps[e], th[e], th_next[e]);
            }
        }
        __syncthreads();                                                  // theta[next] is complete before its node pass
    }
}

// The general form: `per` blocks of 256 per sample, sample b = blockIdx.x / per.  Per-sample state is at row b * n + k and
// edge slot b * nnz + e of the workspace arrays.
template <class R>
__global__ __launch_bounds__(256) void k_dmp_batch_out0(typename R::Args a, unsigned per) {
    const int k = (int)(blockIdx.x % per) * 256 + threadIdx.x;
    if (k >= a.n) return;
    const DmpSample s = dmp_sample(a, blockIdx.x / per);
    dmp_store3(s.out, k, s.s0[(size_t)k * 3], s.s0[(size_t)k * 3 + 1], s.s0[(size_t)k * 3 + 2]);
}

// gnode_dmp_f32's start (gnode_dmp.hip): row 0 from a 0/1 seed vector.  The run reads it back from there as its `init`.
__global__ __launch_bounds__(256) void k_dmp_seed_out0(const float* __restrict__ seed, int n, float* __restrict__ out0);

template <class R>
__global__ __launch_bounds__(256) void k_dmp_batch_init(const int* __restrict__ src, typename R::Args a, unsigned per,
                                                       float* __restrict__ theta, float* __restrict__ phi, float* __restrict__ ps) {
    const size_t b = blockIdx.x / per;
    const long e = (long)(blockIdx.x % per) * 256 + threadIdx.x;
    if (e >= a.nnz) return;
    const DmpSample s = dmp_sample(a, b);
    const size_t slot = b * (size_t)a.nnz + e, u = src[e];
    dmp_edge_start(s.s0[u * 3], s.s0[u * 3 + 1], s.w[R::launch(a).w + e], theta[slot], phi[slot], ps[slot]);
}

template <class R>
__global__ __launch_bounds__(256) void k_dmp_batch_node(const int* __restrict__ rowptr, const int* __restrict__ rev,
                                                       const float* __restrict__ theta, typename R::Args a, unsigned per, int t,
                                                       float* __restrict__ P, float* __restrict__ Pr, float* __restrict__ Pi) {
    const size_t b = blockIdx.x / per;
    const int k = (int)(blockIdx.x % per) * 256 + threadIdx.x;
    if (k >= a.n) return;
    const DmpSample s = dmp_sample(a, b);
    const size_t r = b * (size_t)a.n + k;
    const float p = dmp_row_product(rev, theta + b * (size_t)a.nnz, rowptr[k], rowptr[k + 1]);
    P[r] = p;
    float sk, pi, pr;                                                     // step 1 starts from the state itself
    dmp_node_update(p, s.s0[(size_t)k * 3], t == 1 ? s.s0[(size_t)k * 3 + 1] : Pi[r], t == 1 ? s.s0[(size_t)k * 3 + 2] : Pr[r],
                    s.gamma[R::launch(a).g + k], sk, pi, pr);
    Pr[r] = pr; Pi[r] = pi;
    dmp_store3(s.out + (size_t)t * a.n * 3, k, sk, pi, pr);
}

template <class R>
__global__ __launch_bounds__(256) void k_dmp_batch_edge(const int* __restrict__ src, const int* __restrict__ rev,
                                                       const float* __restrict__ P, const float* __restrict__ theta, typename R::Args a,
                                                       unsigned per, float* __restrict__ phi, float* __restrict__ ps,
                                                       float* __restrict__ theta_next) {
    const size_t b = blockIdx.x / per;
    const long e = (long)(blockIdx.x % per) * 256 + threadIdx.x;
    if (e >= a.nnz) return;
    const DmpSample s = dmp_sample(a, b);
    const DmpStepTables at = R::launch(a);
    const size_t base = b * (size_t)a.nnz, slot = base + e;
    const int u = src[e];
    dmp_edge_update(P[b * (size_t)a.n + u], theta[base + rev[e]], s.s0[(size_t)u * 3], s.w[at.w + e], s.w[at.w_next + e], s.gamma[at.g + u],
                    phi[slot], ps[slot], theta[slot], theta_next[slot]);
}

// ------------------------------------------------------------------------------------------------ the reverse sweep's kernels
// The gradient of sum(grad_out * out) with respect to each table of w and gamma and to the start.  Adjoints carried from step
// t + 1 to step t: per edge theta_bar, phi_bar, q_bar (of Ps_e), per node pi_bar, pr_bar; all start at 0.  A step is an edge pass
// (the reverse of dmp_edge_update, absent at t = maxTime - 1, whose messages had no reader) and a node pass (the reverse of
// dmp_node_update and of both products: P_u and the cavity product P_u / theta[rev e], which does not depend on theta[rev e]).
// The edge pass leaves two numbers per edge for the node pass of its source's row, which sums them in ascending position from
// 0; the node pass writes theta_bar of the reverses of its row's edges into the OTHER theta_bar buffer: rev is a permutation, so
// every slot is written once per step.  With p_t the table of step t:
//   edge pass t   pb = phi_bar - w^{p_{t+1}} theta_bar          theta_{t+1} = theta_t - w^{p_{t+1}} phi_t
//                 w_bar^{p_{t+1}} -= phi_t theta_bar            the NEXT step's table: theta_{t+1}'s weight
//                 w_bar^{p_t}     -= ((1 - gamma^{p_t}_u) phi_{t-1}) pb
//                 the share of gamma_bar^{p_t}_u is -((1 - w^{p_t}) phi_{t-1}) pb;  phi_bar <- ((1 - w^{p_t})(1 - gamma^{p_t}_u)) pb
//   node pass t   gamma_bar^{p_t}_k += Pi_{t-1}[k] aR + its row's shares;  pi_bar <- gamma^{p_t}_k aR
//   after t = 1   w_bar^{p_1} -= Pi_0[src] theta_bar;  pi0_bar sums phi_bar - w^{p_1} theta_bar over the row
// Ownership: in one pass thread e writes grad_w[p_t][e] and grad_w[p_{t+1}][e] and nothing else of grad_w, thread k writes
// grad_gamma[p_t][k]; passes are separated by a launch boundary or a barrier, and in the one-workgroup form an element has one
// thread for the whole sweep.  So nothing is atomic, the result is deterministic, and a table no step names keeps the zeros the
// entry wrote.  Where p_t = p_{t+1} the two updates of the one slot happen in dmp_rev_edge's order, on one register.  Like the
// recurrence these round as written, and both forms call them on the sample's own pointers, in global memory or in LDS.
struct DmpGradSample {                  // sample b's own tables (the tapes are not __restrict__: written and read in one launch)
    const float* __restrict__ w; const float* __restrict__ gamma; const float* __restrict__ s0; const float* __restrict__ out;
    const float* __restrict__ gout;
    float *gw, *gg, *gi, *th_tape, *ph_tape;
    int n, maxTime; long nnz;
    __device__ __forceinline__ float* theta(int t) const { return th_tape + (size_t)(t - 1) * nnz; }    // theta_t, t >= 1
    __device__ __forceinline__ float* phi(int t) const { return ph_tape + (size_t)t * nnz; }            // phi_t, t >= 0
};
template <class R>
__device__ __forceinline__ DmpGradSample dmp_grad_sample(const typename R::GradArgs& a, size_t b) {
    const size_t nn = (size_t)a.n, ne = (size_t)a.nnz, np = R::tables(a), tape = b * (size_t)(a.maxTime - 1) * ne;
    return {a.w + b * a.w_stride, a.gamma + b * a.gamma_stride, a.init + b * nn * 3, a.out + b * (size_t)a.maxTime * nn * 3,
            a.gout + b * (size_t)a.maxTime * nn * 3, a.gw ? a.gw + b * np * ne : nullptr, a.gg ? a.gg + b * np * nn : nullptr,
            a.gi ? a.gi + b * nn * 3 : nullptr, a.th_tape + tape, a.ph_tape + tape, a.n, a.maxTime, a.nnz};
}
// The work of one thread on one element, for both forms.  The tape first: the forward's own functions, theta and phi kept.
__device__ __forceinline__ void dmp_tape_start(const DmpGradSample& s, const int* src, float* ps, long w_at, long e) {
    const size_t u = src[e];
    dmp_edge_start(s.s0[u * 3], s.s0[u * 3 + 1], s.w[w_at + e], s.theta(1)[e], s.phi(0)[e], ps[e]);
}
__device__ __forceinline__ void dmp_tape_edge(const DmpGradSample& s, const int* src, const int* rev, const float* P, float* ps, int t,
                                              const DmpStepTables& at, long e) {
    const size_t u = src[e];
    float ph = s.phi(t - 1)[e];
    dmp_edge_update(P[u], s.theta(t)[rev[e]], s.s0[u * 3], s.w[at.w + e], s.w[at.w_next + e], s.gamma[at.g + u], ph, ps[e], s.theta(t)[e],
                    s.theta(t + 1)[e]);
    s.phi(t)[e] = ph;
}
template <class R>
__device__ __forceinline__ void dmp_grad_edge(const DmpGradSample& s, const DmpAdjoint& A, const int* src, int t, const DmpStepTables& at,
                                              long e) {
    const int u = src[e];
    if (R::kOneSlot || at.w == at.w_next) {                     // one slot: both updates on one register, in dmp_rev_edge's order
        float w_bar = s.gw ? s.gw[at.w + e] : 0.0f;
        dmp_rev_edge(s.w[at.w + e], s.gamma[at.g + u], s.phi(t)[e], s.phi(t - 1)[e], A.tb[e], A.phb[e], A.qb[e], w_bar, A.q_tot[e],
                     A.gamma_part[e]);
        if (s.gw) s.gw[at.w + e] = w_bar;
        return;
    }
    float w_bar = s.gw ? s.gw[at.w + e] : 0.0f, w_bar_next = s.gw ? s.gw[at.w_next + e] : 0.0f;
    dmp_rev_edge(s.w[at.w + e], s.w[at.w_next + e], s.gamma[at.g + u], s.phi(t)[e], s.phi(t - 1)[e], A.tb[e], A.phb[e], A.qb[e], w_bar,
                 w_bar_next, A.q_tot[e], A.gamma_part[e]);
    if (s.gw) { s.gw[at.w + e] = w_bar; s.gw[at.w_next + e] = w_bar_next; }
}
__device__ __forceinline__ void dmp_grad_node(const DmpGradSample& s, const DmpAdjoint& A, const int* rowptr, const int* rev, int t,
                                              long g_at, int k) {
    const int lo = rowptr[k], hi = rowptr[k + 1];
    const bool edge_pass = t + 1 < s.maxTime;                   // (the last step's messages had no reader)
    const float* theta = s.theta(t);
    const float ps0 = s.s0[(size_t)k * 3];
    const float P = dmp_row_product(rev, theta, lo, hi);
    float gamma_bar = s.gg ? s.gg[g_at + k] : 0.0f, ps0_bar = s.gi ? s.gi[(size_t)k * 3] : 0.0f, S = 0.0f, P_bar;
    if (edge_pass) {
        const DmpRowSums sums = dmp_rev_row_sums(rev, theta, A.q_tot, A.gamma_part, lo, hi, P, ps0);
        gamma_bar = gamma_bar + sums.gamma;
        ps0_bar = ps0_bar + sums.ps0;
        S = sums.S;
    }
    const float* g = s.gout + ((size_t)t * s.n + k) * 3;
    dmp_rev_node(g[0], g[1], g[2], P, ps0, s.out[((size_t)(t - 1) * s.n + k) * 3 + 1], s.gamma[g_at + k], A.pib[k], A.prb[k], gamma_bar,
                 ps0_bar, P_bar);
    if (s.gg) s.gg[g_at + k] = gamma_bar;
    if (s.gi) s.gi[(size_t)k * 3] = ps0_bar;
    dmp_rev_theta(rev, theta, edge_pass ? A.q_tot : nullptr, lo, hi, P, ps0, P_bar * P, S, A.tb, A.tb_next);
}
// after step 1: theta_1 = (1 - w^{p_1} Pi_0[src]) + 1e-10, phi_0 = Pi_0[src], Ps_e^{prev} = Ps_0[src], and row 0 of `out` is the start
__device__ __forceinline__ void dmp_grad_start_edge(const DmpGradSample& s, const DmpAdjoint& A, const int* src, long w_at, long e) {
    if (s.gw) s.gw[w_at + e] = s.gw[w_at + e] - s.s0[(size_t)src[e] * 3 + 1] * A.tb[e];
}
__device__ __forceinline__ void dmp_grad_start_node(const DmpGradSample& s, const DmpAdjoint& A, const int* rowptr, long w_at, int k) {
    if (!s.gi) return;
    float pi0_bar = 0.0f, ps0_bar = s.gi[(size_t)k * 3];
    float q_sum = 0.0f;
    for (int e = rowptr[k]; e < rowptr[k + 1]; ++e) {
        pi0_bar = pi0_bar + (A.phb[e] - s.w[w_at + e] * A.tb[e]);
        q_sum = q_sum + A.qb[e];
    }
    ps0_bar = ps0_bar + q_sum;
    const float* g = s.gout + (size_t)k * 3;
    s.gi[(size_t)k * 3] = ps0_bar + g[0];
    s.gi[(size_t)k * 3 + 1] = pi0_bar + (A.pib[k] + g[1]);
    s.gi[(size_t)k * 3 + 2] = A.prb[k] + g[2];
}

// One workgroup = one sample: the forward again with theta and phi kept on the tape (in the workspace; Ps_e and P use the
// room of q_tot and pi_bar meanwhile), then the sweep with the adjoint state in LDS.  Thread `tid` owns nodes and edges tid,
// tid + blockDim.x, ... in every pass, so a gradient slot of any table has one writer for the whole sweep; the barriers sit in
// uniform control flow (the loops' bounds are kernel arguments).  What one thread writes to the tape another reads only after a
// barrier.
template <class R>
__global__ __launch_bounds__(1024) void k_dmp_grad_wg(const int* __restrict__ rowptr, const int* __restrict__ src,
                                                     const int* __restrict__ rev_g, typename R::GradArgs a) {
    extern __shared__ __attribute__((aligned(16))) char dmp_smem[];
    const int n = a.n, nnz = (int)a.nnz, T = a.maxTime, tid = threadIdx.x, nt = blockDim.x;
    const size_t eb = dmp_align16((size_t)nnz * 4), nb = dmp_align16((size_t)n * 4);
    auto edges = [&](int i) { return (float*)(dmp_smem + i * eb); };
    DmpAdjoint A = {edges(0), edges(1), edges(2), edges(3), edges(4), edges(5), (float*)(dmp_smem + 7 * eb),
                          (float*)(dmp_smem + 7 * eb + nb)};
    int* rev = (int*)(dmp_smem + 6 * eb);
    float* ps = A.q_tot; float* P = A.pib;
    const DmpGradSample s = dmp_grad_sample<R>(a, blockIdx.x);
    const long w1 = R::step(a, 1).w;
    for (int e = tid; e < nnz; e += nt) {
        rev[e] = rev_g[e];
        dmp_tape_start(s, src, ps, w1, e);
    }
    __syncthreads();
    for (int t = 1; t + 1 < T; ++t) {
        const DmpStepTables at = R::step(a, t);
        for (int k = tid; k < n; k += nt) P[k] = dmp_row_product(rev, s.theta(t), rowptr[k], rowptr[k + 1]);
        __syncthreads();
        for (int e = tid; e < nnz; e += nt) dmp_tape_edge(s, src, rev, P, ps, t, at, e);
        __syncthreads();
    }
    for (int e = tid; e < nnz; e += nt) { A.tb[e] = 0.0f; A.phb[e] = 0.0f; A.qb[e] = 0.0f; }
    for (int k = tid; k < n; k += nt) { A.pib[k] = 0.0f; A.prb[k] = 0.0f; }
    __syncthreads();
    for (int t = T - 1; t >= 1; --t, dmp_adjoint_swap(A)) {
        const DmpStepTables at = R::step(a, t);
        if (t + 1 < T)
            for (int e = tid; e < nnz; e += nt) dmp_grad_edge<R>(s, A, src, t, at, e);
        __syncthreads();
        for (int k = tid; k < n; k += nt) dmp_grad_node(s, A, rowptr, rev, t, at.g, k);
        __syncthreads();
    }
    for (int e = tid; e < nnz; e += nt) dmp_grad_start_edge(s, A, src, w1, e);
    for (int k = tid; k < n; k += nt) dmp_grad_start_node(s, A, rowptr, w1, k);
}

// The general form: `per` blocks of 256 per sample; the adjoint state of sample b is at row b * n and edge slot b * nnz of
// the workspace arrays.
__device__ __forceinline__ DmpAdjoint dmp_adjoint_of(const DmpAdjoint& A, size_t b, int n, long nnz) {
    const size_t e = b * (size_t)nnz, k = b * (size_t)n;
    return {A.tb + e, A.tb_next + e, A.phb + e, A.qb + e, A.q_tot + e, A.gamma_part + e, A.pib + k, A.prb + k};
}
template <class R>
__global__ __launch_bounds__(256) void k_dmp_tape_start(const int* __restrict__ src, typename R::GradArgs a, unsigned per, float* ps) {
    const size_t b = blockIdx.x / per;
    const long e = (long)(blockIdx.x % per) * 256 + threadIdx.x;
    if (e < a.nnz) dmp_tape_start(dmp_grad_sample<R>(a, b), src, ps + b * (size_t)a.nnz, R::launch(a).w, e);
}
template <class R>
__global__ __launch_bounds__(256) void k_dmp_tape_node(const int* __restrict__ rowptr, const int* __restrict__ rev, typename R::GradArgs a,
                                                      unsigned per, int t, float* __restrict__ P) {
    const size_t b = blockIdx.x / per;
    const int k = (int)(blockIdx.x % per) * 256 + threadIdx.x;
    if (k < a.n) P[b * (size_t)a.n + k] = dmp_row_product(rev, dmp_grad_sample<R>(a, b).theta(t), rowptr[k], rowptr[k + 1]);
}
template <class R>
__global__ __launch_bounds__(256) void k_dmp_tape_edge(const int* __restrict__ src, const int* __restrict__ rev, const float* __restrict__ P,
                                                      typename R::GradArgs a, unsigned per, int t, float* ps) {
    const size_t b = blockIdx.x / per;
    const long e = (long)(blockIdx.x % per) * 256 + threadIdx.x;
    if (e < a.nnz) dmp_tape_edge(dmp_grad_sample<R>(a, b), src, rev, P + b * (size_t)a.n, ps + b * (size_t)a.nnz, t, R::launch(a), e);
}
template <class R>
__global__ __launch_bounds__(256) void k_dmp_grad_edge(const int* __restrict__ src, typename R::GradArgs a, DmpAdjoint A, unsigned per,
                                                      int t) {
    const size_t b = blockIdx.x / per;
    const long e = (long)(blockIdx.x % per) * 256 + threadIdx.x;
    if (e < a.nnz) dmp_grad_edge<R>(dmp_grad_sample<R>(a, b), dmp_adjoint_of(A, b, a.n, a.nnz), src, t, R::launch(a), e);
}
template <class R>
__global__ __launch_bounds__(256) void k_dmp_grad_node(const int* __restrict__ rowptr, const int* __restrict__ rev, typename R::GradArgs a,
                                                      DmpAdjoint A, unsigned per, int t) {
    const size_t b = blockIdx.x / per;
    const int k = (int)(blockIdx.x % per) * 256 + threadIdx.x;
    if (k < a.n) dmp_grad_node(dmp_grad_sample<R>(a, b), dmp_adjoint_of(A, b, a.n, a.nnz), rowptr, rev, t, R::launch(a).g, k);
}
template <class R>
__global__ __launch_bounds__(256) void k_dmp_grad_start_edge(const int* __restrict__ src, typename R::GradArgs a, DmpAdjoint A,
                                                            unsigned per) {
    const size_t b = blockIdx.x / per;
    const long e = (long)(blockIdx.x % per) * 256 + threadIdx.x;
    if (e < a.nnz) dmp_grad_start_edge(dmp_grad_sample<R>(a, b), dmp_adjoint_of(A, b, a.n, a.nnz), src, R::launch(a).w, e);
}
template <class R>
__global__ __launch_bounds__(256) void k_dmp_grad_start_node(const int* __restrict__ rowptr, typename R::GradArgs a, DmpAdjoint A,
                                                            unsigned per) {
    const size_t b = blockIdx.x / per;
    const int k = (int)(blockIdx.x % per) * 256 + threadIdx.x;
    if (k < a.n) dmp_grad_start_node(dmp_grad_sample<R>(a, b), dmp_adjoint_of(A, b, a.n, a.nnz), rowptr, R::launch(a).w, k);
}

// once per device, from gnode_graph_create, each in the unit that instantiates the direction's kernels
template <class R> static int dmp_batch_set_attributes() {
    GN_HIP(hipFuncSetAttribute((const void*)k_dmp_batch_wg<R>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDmpLdsLimit));
    return 0;
}
template <class R> static int dmp_grad_set_attributes() {
    GN_HIP(hipFuncSetAttribute((const void*)k_dmp_grad_wg<R>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDmpLdsLimit));
    return 0;
}

// ------------------------------------------------------------------------------------------------ the host side, once
// Which form serves a graph: the LDS of a sample, whatever the rates are (gnode_dmp.hip answers the two sizes).
static inline bool dmp_batch_one_workgroup(gnode_graph_t g) {
#ifdef GN_DMP_BATCH_GENERAL_ONLY        // a measurement build (tools/bench_dmp_batch.py --lib): the general form at every size
    return false;
#else
    return gnode_dmp_batch_lds_bytes(g) <= kDmpLdsLimit;
#endif
}
static inline bool dmp_grad_one_workgroup(gnode_graph_t g) { return gnode_dmp_batch_backward_lds_bytes(g) <= kDmpLdsLimit; }

// The workspace of a forward call: the policy's head (R::head_bytes: unused room, or the device copy of the phase row), then
// for the general form theta x2, phi, ps over B * nnz edge slots and P, Pr, Pi over B * n rows; for the solo entries the 0/1
// seed vector after them.  With `base` null only `bytes` means anything.  maxTime sizes the scheduled head alone: under
// constant rates nothing here depends on it (kDmpAnyHorizon for a size query that has none).
static constexpr size_t kDmpAnyHorizon = 2;
struct DmpWorkspace {
    int32_t* phase;
    float *theta[2], *phi, *ps, *P, *Pr, *Pi, *seed;
    size_t bytes;
};
template <class R>
static DmpWorkspace dmp_carve(gnode_graph_t g, size_t B, size_t maxTime, bool general, bool seed_vector, void* base) {
    const size_t edges = (size_t)std::max<int64_t>(g->nnz, 1);
    const size_t EB = general ? gn_align(B * edges * 4) : 0, NB = general ? gn_align(B * (size_t)g->info.n * 4) : 0;
    size_t at = 0;
    auto take = [&](size_t bytes) { char* p = base ? (char*)base + at : nullptr; at += bytes; return (float*)p; };
    DmpWorkspace w;
    w.phase = (int32_t*)take(R::head_bytes(g, maxTime));
    w.theta[0] = take(EB); w.theta[1] = take(EB); w.phi = take(EB); w.ps = take(EB);
    w.P = take(NB); w.Pr = take(NB); w.Pi = take(NB);
    w.seed = take(seed_vector ? gn_align((size_t)g->info.n * 4) : 0);
    w.bytes = at;
    return w;
}
// The workspace of a backward call: the policy's head | the tapes of theta and phi, B * (maxTime - 1) * nnz each; for the
// general form Ps_e, theta_bar x2, phi_bar, q_bar, q_tot, gamma_part over B * nnz edge slots and P, pi_bar, pr_bar over B * n rows.
struct DmpGradWorkspace {
    int32_t* phase;
    float *th_tape, *ph_tape, *ps, *P;
    DmpAdjoint adj;
    size_t bytes;
};
template <class R>
static DmpGradWorkspace dmp_grad_carve(gnode_graph_t g, size_t B, size_t maxTime, bool general, void* base) {
    const size_t edges = (size_t)std::max<int64_t>(g->nnz, 1), tape = gn_align(B * (maxTime - 1) * edges * 4);
    const size_t EB = general ? gn_align(B * edges * 4) : 0, NB = general ? gn_align(B * (size_t)g->info.n * 4) : 0;
    size_t at = 0;
    auto take = [&](size_t bytes) { char* p = base ? (char*)base + at : nullptr; at += bytes; return (float*)p; };
    DmpGradWorkspace w;
    w.phase = (int32_t*)take(R::head_bytes(g, maxTime));
    w.th_tape = take(tape); w.ph_tape = take(tape);
    w.ps = take(EB); w.P = take(NB);
    w.adj.tb = take(EB); w.adj.tb_next = take(EB); w.adj.phb = take(EB); w.adj.qb = take(EB); w.adj.q_tot = take(EB);
    w.adj.gamma_part = take(EB); w.adj.pib = take(NB); w.adj.prb = take(NB);
    w.bytes = at;
    return w;
}

// What a forward or a backward call settles before it writes anything, in this order: its arguments, the form and its launch
// shape, the workspace's size, the pattern's symmetry.
//   who       the entry's name for the messages        pointers   whether the entry's own pointers are all there
//   wanted    whether some output is asked for         solo       a solo entry: the general form at every size
//   fits      whether the direction's one-workgroup form serves this graph; need(general): its workspace bytes
//   schedule  null under constant rates; else its P and its phase entries are checked where the seeds are
struct DmpShape {
    int n; long nnz;
    bool one_wg;
    unsigned ng, eg;                    // blocks of 256 per sample over the nodes and over the edges (the general form)
    unsigned threads;                   // of the one workgroup per sample
};
template <class Need>
static int dmp_preamble(const char* who, gnode_graph_t g, const float* weights, long w_stride, const float* gamma, long gamma_stride,
                        bool pointers, const int32_t* seeds_host, int32_t n_seeds, const DmpSchedule* schedule, bool wanted, int32_t B,
                        int32_t maxTime, bool solo, bool (*fits)(gnode_graph_t), Need need, size_t workspace_bytes, DmpShape* s) {
    GN_CHECK_ARG(g && gamma && pointers, "%s: null pointer", who);
    GN_CHECK_ARG(weights || g->nnz == 0, "%s: weights is null", who);          // no edge, no weight: an empty tensor has no address
    GN_CHECK_ARG(maxTime >= 2, "%s: maxTime must be >= 2 (got %d)", who, maxTime);
    GN_CHECK_ARG(B >= 1, "%s: B must be >= 1 (got %d)", who, B);
    if (!schedule) {
        GN_CHECK_ARG(w_stride == 0 || w_stride == g->nnz, "%s: w_stride must be 0 or nnz = %ld (got %ld)", who, (long)g->nnz, w_stride);
        GN_CHECK_ARG(gamma_stride == 0 || gamma_stride == g->info.n, "%s: gamma_stride must be 0 or n = %d (got %ld)", who, g->info.n, gamma_stride);
    } else {
        const int64_t P = schedule->P;
        GN_CHECK_ARG(P >= 1, "%s: a schedule has at least one phase (P = %d)", who, schedule->P);
        GN_CHECK_ARG(w_stride == 0 || w_stride == P * g->nnz, "%s: w_stride must be 0 or P * nnz = %lld (got %lld)", who,
                     (long long)(P * g->nnz), (long long)w_stride);
        GN_CHECK_ARG(gamma_stride == 0 || gamma_stride == P * g->info.n, "%s: gamma_stride must be 0 or P * n = %lld (got %lld)", who,
                     (long long)(P * g->info.n), (long long)gamma_stride);
        for (int t = 1; t < maxTime; ++t)
            GN_CHECK_ARG(schedule->phase_host[t] >= 0 && schedule->phase_host[t] < P, "%s: phase[%d] = %d is not in [0, %d)", who, t,
                         schedule->phase_host[t], schedule->P);
    }
    for (int i = 0; i < n_seeds; ++i)
        GN_CHECK_ARG(seeds_host[i] >= 0 && seeds_host[i] < g->info.n, "%s: seed %d out of range", who, seeds_host[i]);
    GN_CHECK_ARG(wanted, "%s: no gradient is asked for", who);
    s->n = g->info.n; s->nnz = g->nnz;
    s->ng = (unsigned)((s->n + 255) / 256); s->eg = (unsigned)std::max<long>(1, (s->nnz + 255) / 256);
    s->one_wg = !solo && fits(g);
    s->threads = (unsigned)std::min<long>(1024, std::max<long>(64, (std::max<long>(s->n, s->nnz) + 63) / 64 * 64));
    GN_CHECK_ARG(s->one_wg || (size_t)B * std::max(s->ng, s->eg) < ((size_t)1 << 31), "%s: B = %d is too many samples for this graph", who, B);
    const size_t bytes = need(!s->one_wg);
    if (workspace_bytes < bytes) {
        gnode_set_error("%s: workspace %zu < %zu", who, workspace_bytes, bytes);
        return GNODE_ERR_WORKSPACE;
    }
    GN_CHECK_ARG(g->symmetric, "%s: the sparsity pattern is not symmetric (DMP here serves undirected graphs)", who);
    return 0;
}

// What a scheduled call does between its preamble and its first launch: the tables are probabilities (dmp_check_rate_tables reads
// them back and names the first that is not), then the phase row goes to the head of the workspace.  Entry 0 is never read; it
// travels as 0 so that the device copy holds no number out of range.  The caller synchronises: phase_host is done with then.
static inline int dmp_stage_schedule(const char* who, gnode_graph_t g, const float* weights, long w_stride, const float* gamma,
                                     long gamma_stride, const DmpSchedule& schedule, int32_t B, int32_t maxTime, int32_t* phase,
                                     hipStream_t st) {
    const size_t P = (size_t)schedule.P;
    if (int rc = dmp_check_rate_tables(who, "weights", weights, w_stride ? (size_t)B : 1, P, (size_t)g->nnz, st)) return rc;
    if (int rc = dmp_check_rate_tables(who, "gamma", gamma, gamma_stride ? (size_t)B : 1, P, (size_t)g->info.n, st)) return rc;
    GN_HIP(hipMemsetAsync(phase, 0, sizeof(int32_t), st));
    GN_HIP(hipMemcpyAsync(phase + 1, schedule.phase_host + 1, sizeof(int32_t) * (size_t)(maxTime - 1), hipMemcpyHostToDevice, st));
    return 0;
}

// B samples forward.  `solo`: one of the two solo entries, which take the general form at every size and carve the seed
// vector's room.  init == nullptr: gnode_dmp_f32, whose n_seeds seeds become output row 0, the run's init.  `host_schedule`:
// the policy's HostSchedule (a DmpSchedule left at its default is refused: null pointer); a scheduled call synchronises the
// stream again before it returns.
template <class R>
static int dmp_run(const char* who, gnode_graph_t g, const float* weights, long w_stride, const float* gamma, long gamma_stride,
                   const float* init, const int32_t* seeds_host, int32_t n_seeds, int32_t B, int32_t maxTime, float* out, bool solo,
                   void* workspace, size_t workspace_bytes, void* stream, const typename R::HostSchedule& host_schedule = {}) {
    constexpr bool kScheduled = R::kScheduled;
    const DmpSchedule* schedule = R::schedule_of(host_schedule);        // null exactly where !kScheduled
    DmpShape s;
    if (int rc = dmp_preamble(who, g, weights, w_stride, gamma, gamma_stride,
                              (init || seeds_host || n_seeds == 0) && out && workspace && (!schedule || schedule->phase_host), seeds_host,
                              n_seeds, schedule, true, B, maxTime, solo, dmp_batch_one_workgroup,
                              [&](bool general) { return dmp_carve<R>(g, (size_t)B, (size_t)maxTime, general, solo, nullptr).bytes; },
                              workspace_bytes, &s))
        return rc;
    const int n = s.n;
    const unsigned ng = s.ng, eg = s.eg;
    const DmpWorkspace ws = dmp_carve<R>(g, (size_t)B, (size_t)maxTime, !s.one_wg, solo, workspace);
    hipStream_t st = (hipStream_t)stream;
    typename R::Args a;
    static_cast<DmpBatchArgs&>(a) = {weights, w_stride, gamma, gamma_stride, init ? init : out, out, n, maxTime, s.nnz};
    const float one = 1.0f;
    if constexpr (kScheduled) {
        if (int rc = dmp_stage_schedule(who, g, weights, w_stride, gamma, gamma_stride, *schedule, B, maxTime, ws.phase, st)) return rc;
        a.at = {0, 0, 0}; a.phase = ws.phase; a.P = schedule->P;
    } else if (!init) {
        GN_HIP(hipMemsetAsync(ws.seed, 0, (size_t)n * 4, st));
        for (int i = 0; i < n_seeds; ++i) GN_HIP(hipMemcpyAsync(ws.seed + seeds_host[i], &one, 4, hipMemcpyHostToDevice, st));
    }
    // `one`, seeds_host and phase_host are done with.  For the entries that stage nothing, nothing waits on the host any more:
    // only the documented contract ("Synchronises `stream`", include/gnode.h) keeps the call there
    GN_HIP(hipStreamSynchronize(st));
    const int32_t* phase_host = schedule ? schedule->phase_host : nullptr;
    if (s.one_wg) {
        hipLaunchKernelGGL(k_dmp_batch_wg<R>, dim3((unsigned)B), dim3(s.threads), gnode_dmp_batch_lds_bytes(g), st, g->rowptr, g->src, g->rev, a);
        GN_LAUNCH_CHECK();
    } else {
        const dim3 gn((unsigned)B * ng), ge((unsigned)B * eg);
        if constexpr (!kScheduled) {
            if (init) hipLaunchKernelGGL(k_dmp_batch_out0<R>, gn, dim3(256), 0, st, a, ng);
            else hipLaunchKernelGGL(k_dmp_seed_out0, gn, dim3(256), 0, st, ws.seed, n, out);
        } else {
            hipLaunchKernelGGL(k_dmp_batch_out0<R>, gn, dim3(256), 0, st, a, ng);
        }
        R::set_step(a, phase_host, 1);
        hipLaunchKernelGGL(k_dmp_batch_init<R>, ge, dim3(256), 0, st, g->src, a, eg, ws.theta[0], ws.phi, ws.ps);
        GN_LAUNCH_CHECK();
        for (int t = 1; t < maxTime; ++t) {
            const int cur = (t - 1) & 1;
            R::set_step(a, phase_host, t);
            hipLaunchKernelGGL(k_dmp_batch_node<R>, gn, dim3(256), 0, st, g->rowptr, g->rev, ws.theta[cur], a, ng, t, ws.P, ws.Pr, ws.Pi);
            if (t + 1 < maxTime)                 // (the last step's messages have no reader)
                hipLaunchKernelGGL(k_dmp_batch_edge<R>, ge, dim3(256), 0, st, g->src, g->rev, ws.P, ws.theta[cur], a, eg, ws.phi, ws.ps,
                                   ws.theta[cur ^ 1]);
            GN_LAUNCH_CHECK();
        }
    }
    if constexpr (kScheduled) GN_HIP(hipStreamSynchronize(st));
    return 0;
}

// B samples backward; `solo`: gnode_dmp_backward_f32, the general form at every size.  `host_schedule` as dmp_run's.
template <class R>
static int dmp_grad_run(const char* who, gnode_graph_t g, const float* weights, long w_stride, const float* gamma, long gamma_stride,
                        const float* init, int32_t B, int32_t maxTime, const float* out, const float* grad_out, float* grad_w,
                        float* grad_gamma, float* grad_init, bool solo, void* workspace, size_t workspace_bytes, void* stream,
                        const typename R::HostSchedule& host_schedule = {}) {
    constexpr bool kScheduled = R::kScheduled;
    const DmpSchedule* schedule = R::schedule_of(host_schedule);        // null exactly where !kScheduled
    DmpShape s;
    if (int rc = dmp_preamble(who, g, weights, w_stride, gamma, gamma_stride,
                              init && out && grad_out && workspace && (!schedule || schedule->phase_host), nullptr, 0, schedule,
                              grad_w || grad_gamma || grad_init, B, maxTime, solo, dmp_grad_one_workgroup,
                              [&](bool general) { return dmp_grad_carve<R>(g, (size_t)B, (size_t)maxTime, general, nullptr).bytes; },
                              workspace_bytes, &s))
        return rc;
    const long nnz = s.nnz;
    const int n = s.n;
    const unsigned ng = s.ng, eg = s.eg;
    const DmpGradWorkspace ws = dmp_grad_carve<R>(g, (size_t)B, (size_t)maxTime, !s.one_wg, workspace);
    hipStream_t st = (hipStream_t)stream;
    typename R::GradArgs a;
    static_cast<DmpGradArgs&>(a) = {weights, w_stride, gamma, gamma_stride, init, out, grad_out, grad_w, grad_gamma, grad_init, ws.th_tape,
                                    ws.ph_tape, n, maxTime, nnz};
    size_t tables = 1;
    if constexpr (kScheduled) {
        if (int rc = dmp_stage_schedule(who, g, weights, w_stride, gamma, gamma_stride, *schedule, B, maxTime, ws.phase, st)) return rc;
        a.at = {0, 0, 0}; a.phase = ws.phase; a.P = schedule->P;
        tables = (size_t)schedule->P;
    }
    // phase_host is done with; under constant rates nothing waits on the host here: only the documented contract
    // (include/gnode.h) keeps it
    GN_HIP(hipStreamSynchronize(st));
    if (grad_w && nnz) GN_HIP(hipMemsetAsync(grad_w, 0, (size_t)B * tables * nnz * 4, st));        // the sweep accumulates into them
    if (grad_gamma) GN_HIP(hipMemsetAsync(grad_gamma, 0, (size_t)B * tables * n * 4, st));
    if (grad_init) GN_HIP(hipMemsetAsync(grad_init, 0, (size_t)B * n * 12, st));
    const int32_t* phase_host = schedule ? schedule->phase_host : nullptr;
    if (s.one_wg) {
        hipLaunchKernelGGL(k_dmp_grad_wg<R>, dim3((unsigned)B), dim3(s.threads), gnode_dmp_batch_backward_lds_bytes(g), st, g->rowptr, g->src,
                           g->rev, a);
        GN_LAUNCH_CHECK();
    } else {
        const dim3 gn((unsigned)B * ng), ge((unsigned)B * eg);
        R::set_step(a, phase_host, 1);
        hipLaunchKernelGGL(k_dmp_tape_start<R>, ge, dim3(256), 0, st, g->src, a, eg, ws.ps);
        for (int t = 1; t + 1 < maxTime; ++t) {
            R::set_step(a, phase_host, t);
            hipLaunchKernelGGL(k_dmp_tape_node<R>, gn, dim3(256), 0, st, g->rowptr, g->rev, a, ng, t, ws.P);
            hipLaunchKernelGGL(k_dmp_tape_edge<R>, ge, dim3(256), 0, st, g->src, g->rev, ws.P, a, eg, t, ws.ps);
        }
        GN_LAUNCH_CHECK();
        for (float* zero : {ws.adj.tb, ws.adj.phb, ws.adj.qb}) GN_HIP(hipMemsetAsync(zero, 0, (size_t)B * std::max<long>(nnz, 1) * 4, st));
        for (float* zero : {ws.adj.pib, ws.adj.prb}) GN_HIP(hipMemsetAsync(zero, 0, (size_t)B * n * 4, st));
        DmpAdjoint A = ws.adj;
        for (int t = maxTime - 1; t >= 1; --t, dmp_adjoint_swap(A)) {
            R::set_step(a, phase_host, t);
            if (t + 1 < maxTime) hipLaunchKernelGGL(k_dmp_grad_edge<R>, ge, dim3(256), 0, st, g->src, a, A, eg, t);
            hipLaunchKernelGGL(k_dmp_grad_node<R>, gn, dim3(256), 0, st, g->rowptr, g->rev, a, A, ng, t);
            GN_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(k_dmp_grad_start_edge<R>, ge, dim3(256), 0, st, g->src, a, A, eg);        // (a holds step 1's tables)
        hipLaunchKernelGGL(k_dmp_grad_start_node<R>, gn, dim3(256), 0, st, g->rowptr, a, A, ng);
        GN_LAUNCH_CHECK();
    }
    if constexpr (kScheduled) GN_HIP(hipStreamSynchronize(st));
    return 0;
}
