// The reverse sweep of DMP with rates that change over time (gnode_dmp_batch_schedule_backward_f32): the gradient of
// sum(grad_out * out) with respect to each phase's weights and recovery probabilities and to the start, where `out` is what
// gnode_dmp_batch_schedule_f32 returned.  It is gnode_dmp.hip's sweep -- the same dmp_rev_* functions of gnode_dmp.h, the same
// adjoints, tape and two forms -- and knows which phase each step's adjoint belongs to.  With p_t = phase[t]:
//   edge pass t   (only when t + 1 < maxTime; the reverse of the two-weight dmp_edge_update)
//                 pb = phi_bar - w^{p_{t+1}} theta_bar          theta_{t+1} = theta_t - w^{p_{t+1}} phi_t
//                 w_bar^{p_{t+1}} -= phi_t theta_bar            the NEXT step's table: theta_{t+1}'s weight
//                 w_bar^{p_t}     -= ((1 - gamma^{p_t}_u) phi_{t-1}) pb
//                 the share of gamma_bar^{p_t}_u is -((1 - w^{p_t}) phi_{t-1}) pb;  phi_bar <- ((1 - w^{p_t})(1 - gamma^{p_t}_u)) pb
//   node pass t   gamma_bar^{p_t}_k += Pi_{t-1}[k] aR + its row's shares;  pi_bar <- gamma^{p_t}_k aR
//   after t = 1   w_bar^{p_1} -= Pi_0[src] theta_bar;  pi0_bar sums phi_bar - w^{p_1} theta_bar over the row
// Ownership: in one pass thread e writes grad_w[p_t][e] and grad_w[p_{t+1}][e] and nothing else of grad_w, thread k writes
// grad_gamma[p_t][k]; passes are separated by a launch boundary or a barrier, and in the one-workgroup form an element has one
// thread for the whole sweep.  So nothing is atomic, the result is deterministic, and a phase no step names keeps the zeros the
// entry wrote.  Where p_t = p_{t+1} the two updates of the one slot happen in gnode_dmp.hip's order, on one register: one phase,
// or several holding equal tables summed over the phases, is gnode_dmp_batch_backward_f32's sweep.
//
// The tape runs the scheduled forward's own arithmetic (dmp_edge_start with step 1's weight, the two-weight dmp_edge_update), so
// it holds the forward's bits; its layout is gnode_dmp.hip's.  The tables are read from memory, never held in LDS, so the forms
// are chosen by gnode_dmp_batch_backward_lds_bytes as there.
#include "gnode_dmp.h"
#include <algorithm>

struct DmpSchedGradArgs {
    const float* w; long w_stride;      // [P][nnz] per sample, sample b at w + b * w_stride
    const float* gamma; long gamma_stride;
    const float* init;                  // [B][n][3]
    const float* out;                   // [B][maxTime][n][3], the forward's
    const float* gout;                  // the same shape
    float *gw, *gg, *gi;                // [B][P][nnz], [B][P][n], [B][n][3]; null: not wanted
    float *th_tape, *ph_tape;           // [B][maxTime - 1][nnz]: theta_1 .. theta_{T-1} and phi_0 .. phi_{T-2}
    const int32_t* phase;               // device int32 [maxTime] (the one-workgroup form reads it)
    int n, maxTime, P; long nnz;
};
struct DmpSchedGradSample {             // sample b's own tables (the tapes are not __restrict__: written and read in one launch)
    const float* __restrict__ w; const float* __restrict__ gamma; const float* __restrict__ s0; const float* __restrict__ out;
    const float* __restrict__ gout;
    float *gw, *gg, *gi, *th_tape, *ph_tape;
    int n, maxTime; long nnz;
    __device__ __forceinline__ float* theta(int t) const { return th_tape + (size_t)(t - 1) * nnz; }    // theta_t, t >= 1
    __device__ __forceinline__ float* phi(int t) const { return ph_tape + (size_t)t * nnz; }            // phi_t, t >= 0
};
__device__ __forceinline__ DmpSchedGradSample dmp_sched_grad_sample(const DmpSchedGradArgs& a, size_t b) {
    const size_t nn = (size_t)a.n, ne = (size_t)a.nnz, np = (size_t)a.P, tape = b * (size_t)(a.maxTime - 1) * ne;
    return {a.w + b * a.w_stride, a.gamma + b * a.gamma_stride, a.init + b * nn * 3, a.out + b * (size_t)a.maxTime * nn * 3,
            a.gout + b * (size_t)a.maxTime * nn * 3, a.gw ? a.gw + b * np * ne : nullptr, a.gg ? a.gg + b * np * nn : nullptr,
            a.gi ? a.gi + b * nn * 3 : nullptr, a.th_tape + tape, a.ph_tape + tape, a.n, a.maxTime, a.nnz};
}
// Where step t's tables lie inside a sample's [P][...] blocks: w = phase[t] * nnz, w_next = phase[t + 1] * nnz (w again where
// t + 1 = maxTime: nothing reads it there), g = phase[t] * n.  Uniform over a launch, or over the workgroup at a step.
struct DmpStepTables { long w, w_next, g; };

// The work of one thread on one element, for both forms.  The tape first: the scheduled forward's own functions.
__device__ __forceinline__ void dmp_sched_tape_start(const DmpSchedGradSample& s, const int* src, float* ps, long w_at, long e) {
    const size_t u = src[e];
    dmp_edge_start(s.s0[u * 3], s.s0[u * 3 + 1], s.w[w_at + e], s.theta(1)[e], s.phi(0)[e], ps[e]);
}
__device__ __forceinline__ void dmp_sched_tape_edge(const DmpSchedGradSample& s, const int* src, const int* rev, const float* P, float* ps,
                                                    int t, const DmpStepTables& at, long e) {
    const size_t u = src[e];
    float ph = s.phi(t - 1)[e];
    dmp_edge_update(P[u], s.theta(t)[rev[e]], s.s0[u * 3], s.w[at.w + e], s.w[at.w_next + e], s.gamma[at.g + u], ph, ps[e], s.theta(t)[e],
                    s.theta(t + 1)[e]);
    s.phi(t)[e] = ph;
}
__device__ __forceinline__ void dmp_sched_grad_edge(const DmpSchedGradSample& s, const DmpAdjoint& A, const int* src, int t,
                                                    const DmpStepTables& at, long e) {
    const int u = src[e];
    const float w_e = s.w[at.w + e], gamma_u = s.gamma[at.g + u], phi_t = s.phi(t)[e], phi_prev = s.phi(t - 1)[e];
    if (at.w == at.w_next) {                                    // one slot: gnode_dmp.hip's dmp_grad_edge
        float w_bar = s.gw ? s.gw[at.w + e] : 0.0f;
        dmp_rev_edge(w_e, gamma_u, phi_t, phi_prev, A.tb[e], A.phb[e], A.qb[e], w_bar, A.q_tot[e], A.gamma_part[e]);
        if (s.gw) s.gw[at.w + e] = w_bar;
        return;
    }
    float w_bar = s.gw ? s.gw[at.w + e] : 0.0f, w_bar_next = s.gw ? s.gw[at.w_next + e] : 0.0f;
    dmp_rev_edge(w_e, s.w[at.w_next + e], gamma_u, phi_t, phi_prev, A.tb[e], A.phb[e], A.qb[e], w_bar, w_bar_next, A.q_tot[e],
                 A.gamma_part[e]);
    if (s.gw) { s.gw[at.w + e] = w_bar; s.gw[at.w_next + e] = w_bar_next; }
}
__device__ __forceinline__ void dmp_sched_grad_node(const DmpSchedGradSample& s, const DmpAdjoint& A, const int* rowptr, const int* rev,
                                                    int t, long g_at, int k) {
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
__device__ __forceinline__ void dmp_sched_grad_start_edge(const DmpSchedGradSample& s, const DmpAdjoint& A, const int* src, long w_at,
                                                          long e) {
    if (s.gw) s.gw[w_at + e] = s.gw[w_at + e] - s.s0[(size_t)src[e] * 3 + 1] * A.tb[e];
}
__device__ __forceinline__ void dmp_sched_grad_start_node(const DmpSchedGradSample& s, const DmpAdjoint& A, const int* rowptr, long w_at,
                                                          int k) {
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

static bool dmp_sched_grad_one_workgroup(gnode_graph_t g) { return gnode_dmp_batch_backward_lds_bytes(g) <= kDmpLdsLimit; }

// One workgroup = one sample: k_dmp_grad_wg with the step's tables chosen at the top of each step.  The phase reads are uniform
// over the workgroup and the barriers sit in uniform control flow (the loops' bounds are kernel arguments); thread `tid` owns
// nodes and edges tid, tid + blockDim.x, ... in every pass, so a gradient slot of any phase has one writer for the whole sweep.
__global__ __launch_bounds__(1024) void k_dmp_sched_grad_wg(const int* __restrict__ rowptr, const int* __restrict__ src,
                                                           const int* __restrict__ rev_g, DmpSchedGradArgs a) {
    extern __shared__ __attribute__((aligned(16))) char dmp_smem[];
    const int n = a.n, nnz = (int)a.nnz, T = a.maxTime, tid = threadIdx.x, nt = blockDim.x;
    const size_t eb = dmp_align16((size_t)nnz * 4), nb = dmp_align16((size_t)n * 4);
    auto edges = [&](int i) { return (float*)(dmp_smem + i * eb); };
    DmpAdjoint A = {edges(0), edges(1), edges(2), edges(3), edges(4), edges(5), (float*)(dmp_smem + 7 * eb),
                          (float*)(dmp_smem + 7 * eb + nb)};
    int* rev = (int*)(dmp_smem + 6 * eb);
    float* ps = A.q_tot; float* P = A.pib;
    const DmpSchedGradSample s = dmp_sched_grad_sample(a, blockIdx.x);
    auto tables = [&](int t) {                                  // (maxTime >= 2: entry 1 exists; t + 1 is read only where it exists)
        const long p = a.phase[t], p_next = t + 1 < T ? a.phase[t + 1] : p;
        return DmpStepTables{p * nnz, p_next * nnz, p * n};
    };
    const long w1 = (long)a.phase[1] * nnz;
    for (int e = tid; e < nnz; e += nt) {
        rev[e] = rev_g[e];
        dmp_sched_tape_start(s, src, ps, w1, e);
    }
    __syncthreads();
    for (int t = 1; t + 1 < T; ++t) {
        const DmpStepTables at = tables(t);
        for (int k = tid; k < n; k += nt) P[k] = dmp_row_product(rev, s.theta(t), rowptr[k], rowptr[k + 1]);
        __syncthreads();
        for (int e = tid; e < nnz; e += nt) dmp_sched_tape_edge(s, src, rev, P, ps, t, at, e);
        __syncthreads();
    }
    for (int e = tid; e < nnz; e += nt) { A.tb[e] = 0.0f; A.phb[e] = 0.0f; A.qb[e] = 0.0f; }
    for (int k = tid; k < n; k += nt) { A.pib[k] = 0.0f; A.prb[k] = 0.0f; }
    __syncthreads();
    for (int t = T - 1; t >= 1; --t, dmp_adjoint_swap(A)) {
        const DmpStepTables at = tables(t);
        if (t + 1 < T)
            for (int e = tid; e < nnz; e += nt) dmp_sched_grad_edge(s, A, src, t, at, e);
        __syncthreads();
        for (int k = tid; k < n; k += nt) dmp_sched_grad_node(s, A, rowptr, rev, t, at.g, k);
        __syncthreads();
    }
    for (int e = tid; e < nnz; e += nt) dmp_sched_grad_start_edge(s, A, src, w1, e);
    for (int k = tid; k < n; k += nt) dmp_sched_grad_start_node(s, A, rowptr, w1, k);
}

// The general form: gnode_dmp.hip's seven kernels with the offsets of the step's tables as arguments, from the host loop.
// `per` blocks of 256 per sample; the adjoint state of sample b is at row b * n and edge slot b * nnz of the workspace arrays.
__device__ __forceinline__ DmpAdjoint dmp_sched_adjoint_of(const DmpAdjoint& A, size_t b, int n, long nnz) {
    const size_t e = b * (size_t)nnz, k = b * (size_t)n;
    return {A.tb + e, A.tb_next + e, A.phb + e, A.qb + e, A.q_tot + e, A.gamma_part + e, A.pib + k, A.prb + k};
}
__global__ __launch_bounds__(256) void k_dmp_sched_tape_start(const int* __restrict__ src, DmpSchedGradArgs a, unsigned per, long w_at,
                                                             float* ps) {
    const size_t b = blockIdx.x / per;
    const long e = (long)(blockIdx.x % per) * 256 + threadIdx.x;
    if (e < a.nnz) dmp_sched_tape_start(dmp_sched_grad_sample(a, b), src, ps + b * (size_t)a.nnz, w_at, e);
}
__global__ __launch_bounds__(256) void k_dmp_sched_tape_node(const int* __restrict__ rowptr, const int* __restrict__ rev, DmpSchedGradArgs a,
                                                            unsigned per, int t, float* __restrict__ P) {
    const size_t b = blockIdx.x / per;
    const int k = (int)(blockIdx.x % per) * 256 + threadIdx.x;
    if (k < a.n) P[b * (size_t)a.n + k] = dmp_row_product(rev, dmp_sched_grad_sample(a, b).theta(t), rowptr[k], rowptr[k + 1]);
}
__global__ __launch_bounds__(256) void k_dmp_sched_tape_edge(const int* __restrict__ src, const int* __restrict__ rev,
                                                            const float* __restrict__ P, DmpSchedGradArgs a, unsigned per, int t,
                                                            DmpStepTables at, float* ps) {
    const size_t b = blockIdx.x / per;
    const long e = (long)(blockIdx.x % per) * 256 + threadIdx.x;
    if (e < a.nnz) dmp_sched_tape_edge(dmp_sched_grad_sample(a, b), src, rev, P + b * (size_t)a.n, ps + b * (size_t)a.nnz, t, at, e);
}
__global__ __launch_bounds__(256) void k_dmp_sched_grad_edge(const int* __restrict__ src, DmpSchedGradArgs a, DmpAdjoint A, unsigned per,
                                                            int t, DmpStepTables at) {
    const size_t b = blockIdx.x / per;
    const long e = (long)(blockIdx.x % per) * 256 + threadIdx.x;
    if (e < a.nnz) dmp_sched_grad_edge(dmp_sched_grad_sample(a, b), dmp_sched_adjoint_of(A, b, a.n, a.nnz), src, t, at, e);
}
__global__ __launch_bounds__(256) void k_dmp_sched_grad_node(const int* __restrict__ rowptr, const int* __restrict__ rev, DmpSchedGradArgs a,
                                                            DmpAdjoint A, unsigned per, int t, long g_at) {
    const size_t b = blockIdx.x / per;
    const int k = (int)(blockIdx.x % per) * 256 + threadIdx.x;
    if (k < a.n) dmp_sched_grad_node(dmp_sched_grad_sample(a, b), dmp_sched_adjoint_of(A, b, a.n, a.nnz), rowptr, rev, t, g_at, k);
}
__global__ __launch_bounds__(256) void k_dmp_sched_grad_start_edge(const int* __restrict__ src, DmpSchedGradArgs a, DmpAdjoint A,
                                                                  unsigned per, long w_at) {
    const size_t b = blockIdx.x / per;
    const long e = (long)(blockIdx.x % per) * 256 + threadIdx.x;
    if (e < a.nnz) dmp_sched_grad_start_edge(dmp_sched_grad_sample(a, b), dmp_sched_adjoint_of(A, b, a.n, a.nnz), src, w_at, e);
}
__global__ __launch_bounds__(256) void k_dmp_sched_grad_start_node(const int* __restrict__ rowptr, DmpSchedGradArgs a, DmpAdjoint A,
                                                                  unsigned per, long w_at) {
    const size_t b = blockIdx.x / per;
    const int k = (int)(blockIdx.x % per) * 256 + threadIdx.x;
    if (k < a.n) dmp_sched_grad_start_node(dmp_sched_grad_sample(a, b), dmp_sched_adjoint_of(A, b, a.n, a.nnz), rowptr, w_at, k);
}

int gn_dmp_schedule_bwd_set_attributes() {       // once per device, from gnode_graph_create
    GN_HIP(hipFuncSetAttribute((const void*)k_dmp_sched_grad_wg, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDmpLdsLimit));
    return 0;
}

// ------------------------------------------------------------------------------------------------ the host side
// The workspace: the device copy of the phase table | the tapes of theta and phi, B * (maxTime - 1) * nnz each; for the general
// form Ps_e, theta_bar x2, phi_bar, q_bar, q_tot, gamma_part over B * nnz edge slots and P, pi_bar, pr_bar over B * n rows.  With
// `base` null only `bytes` means anything.
struct DmpSchedGradWorkspace {
    int32_t* phase;
    float *th_tape, *ph_tape, *ps, *P;
    DmpAdjoint adj;
    size_t bytes;
};
static DmpSchedGradWorkspace dmp_sched_grad_carve(gnode_graph_t g, size_t B, size_t maxTime, bool general, void* base) {
    const size_t edges = (size_t)std::max<int64_t>(g->nnz, 1), tape = gn_align(B * (maxTime - 1) * edges * 4);
    const size_t EB = general ? gn_align(B * edges * 4) : 0, NB = general ? gn_align(B * (size_t)g->info.n * 4) : 0;
    size_t at = 0;
    auto take = [&](size_t bytes) { char* p = base ? (char*)base + at : nullptr; at += bytes; return (float*)p; };
    DmpSchedGradWorkspace w;
    w.phase = (int32_t*)take(gn_align(maxTime * sizeof(int32_t)));
    w.th_tape = take(tape); w.ph_tape = take(tape);
    w.ps = take(EB); w.P = take(NB);
    w.adj.tb = take(EB); w.adj.tb_next = take(EB); w.adj.phb = take(EB); w.adj.qb = take(EB); w.adj.q_tot = take(EB);
    w.adj.gamma_part = take(EB); w.adj.pib = take(NB); w.adj.prb = take(NB);
    w.bytes = at;
    return w;
}
extern "C" size_t gnode_dmp_batch_schedule_backward_workspace_bytes(gnode_graph_t g, int32_t B, int32_t maxTime) {
    return g && B >= 1 && maxTime >= 2 ? dmp_sched_grad_carve(g, (size_t)B, (size_t)maxTime, !dmp_sched_grad_one_workgroup(g), nullptr).bytes
                                       : 0;
}

extern "C" int gnode_dmp_batch_schedule_backward_f32(gnode_graph_t g, const float* weights, int64_t w_stride, const float* gamma,
                                                     int64_t gamma_stride, const int32_t* phase_host, int32_t P, const float* init, int32_t B,
                                                     int32_t maxTime, const float* out, const float* grad_out, float* grad_w,
                                                     float* grad_gamma, float* grad_init, void* workspace, size_t workspace_bytes,
                                                     void* stream) {
    const char* who = "gnode_dmp_batch_schedule_backward_f32";
    GN_CHECK_ARG(g && gamma && init && out && grad_out && workspace && phase_host, "%s: null pointer", who);
    GN_CHECK_ARG(weights || g->nnz == 0, "%s: weights is null", who);          // no edge, no weight: an empty tensor has no address
    GN_CHECK_ARG(maxTime >= 2, "%s: maxTime must be >= 2 (got %d)", who, maxTime);
    GN_CHECK_ARG(B >= 1, "%s: B must be >= 1 (got %d)", who, B);
    GN_CHECK_ARG(P >= 1, "%s: a schedule has at least one phase (P = %d)", who, P);
    const int n = g->info.n;
    const long nnz = (long)g->nnz;
    GN_CHECK_ARG(w_stride == 0 || w_stride == (int64_t)P * nnz, "%s: w_stride must be 0 or P * nnz = %lld (got %lld)", who, (long long)P * nnz,
                 (long long)w_stride);
    GN_CHECK_ARG(gamma_stride == 0 || gamma_stride == (int64_t)P * n, "%s: gamma_stride must be 0 or P * n = %lld (got %lld)", who,
                 (long long)P * n, (long long)gamma_stride);
    for (int t = 1; t < maxTime; ++t)
        GN_CHECK_ARG(phase_host[t] >= 0 && phase_host[t] < P, "%s: phase[%d] = %d is not in [0, %d)", who, t, phase_host[t], P);
    GN_CHECK_ARG(grad_w || grad_gamma || grad_init, "%s: no gradient is asked for", who);
    const unsigned ng = (unsigned)((n + 255) / 256), eg = (unsigned)std::max<long>(1, (nnz + 255) / 256);
    const bool one_wg = dmp_sched_grad_one_workgroup(g);
    const unsigned threads = (unsigned)std::min<long>(1024, std::max<long>(64, (std::max<long>(n, nnz) + 63) / 64 * 64));
    GN_CHECK_ARG(one_wg || (size_t)B * std::max(ng, eg) < ((size_t)1 << 31), "%s: B = %d is too many samples for this graph", who, B);
    const size_t bytes = dmp_sched_grad_carve(g, (size_t)B, (size_t)maxTime, !one_wg, nullptr).bytes;
    if (workspace_bytes < bytes) {
        gnode_set_error("%s: workspace %zu < %zu", who, workspace_bytes, bytes);
        return GNODE_ERR_WORKSPACE;
    }
    GN_CHECK_ARG(g->symmetric, "%s: the sparsity pattern is not symmetric (DMP here serves undirected graphs)", who);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = dmp_check_rate_tables(who, "weights", weights, w_stride ? (size_t)B : 1, (size_t)P, (size_t)nnz, st)) return rc;
    if (int rc = dmp_check_rate_tables(who, "gamma", gamma, gamma_stride ? (size_t)B : 1, (size_t)P, (size_t)n, st)) return rc;
    const DmpSchedGradWorkspace ws = dmp_sched_grad_carve(g, (size_t)B, (size_t)maxTime, !one_wg, workspace);
    // entry 0 is never read; it travels as 0 so that the device copy holds no number out of range
    GN_HIP(hipMemsetAsync(ws.phase, 0, sizeof(int32_t), st));
    GN_HIP(hipMemcpyAsync(ws.phase + 1, phase_host + 1, sizeof(int32_t) * (size_t)(maxTime - 1), hipMemcpyHostToDevice, st));
    GN_HIP(hipStreamSynchronize(st));          // phase_host is done with
    if (grad_w && nnz) GN_HIP(hipMemsetAsync(grad_w, 0, (size_t)B * P * nnz * 4, st));     // the sweep accumulates into them
    if (grad_gamma) GN_HIP(hipMemsetAsync(grad_gamma, 0, (size_t)B * P * n * 4, st));
    if (grad_init) GN_HIP(hipMemsetAsync(grad_init, 0, (size_t)B * n * 12, st));
    const DmpSchedGradArgs a = {weights, (long)w_stride, gamma, (long)gamma_stride, init, out, grad_out, grad_w, grad_gamma, grad_init,
                                ws.th_tape, ws.ph_tape, ws.phase, n, maxTime, P, nnz};
    if (one_wg) {
        hipLaunchKernelGGL(k_dmp_sched_grad_wg, dim3((unsigned)B), dim3(threads), gnode_dmp_batch_backward_lds_bytes(g), st, g->rowptr, g->src,
                           g->rev, a);
        GN_LAUNCH_CHECK();
        GN_HIP(hipStreamSynchronize(st));
        return 0;
    }
    const dim3 gn((unsigned)B * ng), ge((unsigned)B * eg);
    auto tables = [&](int t) {
        const long p = phase_host[t], p_next = t + 1 < maxTime ? phase_host[t + 1] : p;
        return DmpStepTables{p * nnz, p_next * nnz, p * n};
    };
    const long w1 = (long)phase_host[1] * nnz;
    hipLaunchKernelGGL(k_dmp_sched_tape_start, ge, dim3(256), 0, st, g->src, a, eg, w1, ws.ps);
    for (int t = 1; t + 1 < maxTime; ++t) {
        hipLaunchKernelGGL(k_dmp_sched_tape_node, gn, dim3(256), 0, st, g->rowptr, g->rev, a, ng, t, ws.P);
        hipLaunchKernelGGL(k_dmp_sched_tape_edge, ge, dim3(256), 0, st, g->src, g->rev, ws.P, a, eg, t, tables(t), ws.ps);
    }
    GN_LAUNCH_CHECK();
    for (float* zero : {ws.adj.tb, ws.adj.phb, ws.adj.qb}) GN_HIP(hipMemsetAsync(zero, 0, (size_t)B * std::max<long>(nnz, 1) * 4, st));
    for (float* zero : {ws.adj.pib, ws.adj.prb}) GN_HIP(hipMemsetAsync(zero, 0, (size_t)B * n * 4, st));
    DmpAdjoint A = ws.adj;
    for (int t = maxTime - 1; t >= 1; --t, dmp_adjoint_swap(A)) {
        const DmpStepTables at = tables(t);
        if (t + 1 < maxTime) hipLaunchKernelGGL(k_dmp_sched_grad_edge, ge, dim3(256), 0, st, g->src, a, A, eg, t, at);
        hipLaunchKernelGGL(k_dmp_sched_grad_node, gn, dim3(256), 0, st, g->rowptr, g->rev, a, A, ng, t, at.g);
        GN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_dmp_sched_grad_start_edge, ge, dim3(256), 0, st, g->src, a, A, eg, w1);
    hipLaunchKernelGGL(k_dmp_sched_grad_start_node, gn, dim3(256), 0, st, g->rowptr, a, A, ng, w1);
    GN_LAUNCH_CHECK();
    GN_HIP(hipStreamSynchronize(st));
    return 0;
}
