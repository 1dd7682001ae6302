// Dynamic message passing baseline for SIR on MI355X (gfx950) -- SURVEY 8f rank 4.
//
// Restates DMP_SIR of the reference (dmp.py:74-170): messages live on the directed edges e = (src -> tar) of the
// weighted adjacency in COO row-major order (dmp.py:67-72 = the CSR positions of the graph handle);
//   theta_e   <- theta_e - w_e phi_e
//   P_k        = prod_{e: tar(e) = k} theta_e                 (torch_scatter scatter(reduce='mul'), :93-100)
//   Ps_e       = Ps0[src] * P[src] / theta_{rev(e)}           (the cavity product, :96-99)
//   phi_e     <- (1 - w_e)(1 - gamma_src) phi_e - (Ps_e - Ps_e^{prev})
//   marginals  Ps_k = Ps0_k P_k,  Pr_k += gamma_k Pi_k,  Pi_k = 1 - Ps_k - Pr_k       (:124-129, :141-145)
// Undirected graphs only (every shipped graph is `.to_undirected()`, ode_nn.py:402): the edges INTO k are then the
// reverses of row k's edges, so one CSR serves both directions and P_k multiplies theta_{rev(e)} over row k in
// ascending order -- the order the reference's CPU scatter uses.  fp32 like the reference's FloatTensors.
//
// One statement serves the three entries: B samples on one graph, sample b starting from init[b] = (pS, pI, pR) per node with
// weights + b * w_stride and gamma + b * gamma_stride (a stride of 0 shares the table); gnode_dmp_f32 and gnode_dmp_init_f32
// are B = 1.  The recurrence is the four dmp_* functions of gnode_dmp.h and nothing else; the kernels are loops and indexing
// around them, in two forms chosen by dmp_run:
//   general                    four kernels over rows b * n + k and edge slots b * nnz + e of the workspace: two launches per
//                              time step (node pass, edge pass); theta ping-pongs because the edge pass reads its neighbours'
//   one workgroup per sample   the messages and marginals of a sample live in LDS for the whole horizon: one launch
// A sample's numbers do not depend on the form or on B: same expressions, same per-element order.
//
// The second half of the file is the reverse sweep of the same recurrence (gnode_dmp_batch_backward_f32, gnode_dmp_backward_f32):
// the gradients of the marginals with respect to w, gamma and the start, stated once as dmp_rev_* functions and served in the
// same two forms.
#include "gnode_dmp.h"
#include <algorithm>

// ------------------------------------------------------------------------------------------------ the kernels
struct DmpBatchArgs {
    const float* w; long w_stride;
    const float* gamma; long gamma_stride;
    const float* init;                  // [B][n][3]
    float* out;                         // [B][maxTime][n][3]
    int n, maxTime; long nnz;
};
struct DmpSample {                      // sample b's own tables: w[nnz], gamma[n], the start s0[n][3], out[maxTime][n][3]
    const float* __restrict__ w; const float* __restrict__ gamma; const float* __restrict__ s0; float* __restrict__ out;
};
__device__ __forceinline__ DmpSample dmp_sample(const DmpBatchArgs& a, size_t b) {
    return {a.w + b * a.w_stride, a.gamma + b * a.gamma_stride, a.init + b * (size_t)a.n * 3, a.out + b * (size_t)a.maxTime * a.n * 3};
}
__device__ __forceinline__ void dmp_store3(float* __restrict__ row, int k, float ps, float pi, float pr) {
    row[(size_t)k * 3 + 0] = ps; row[(size_t)k * 3 + 1] = pi; row[(size_t)k * 3 + 2] = pr;
}

extern "C" size_t gnode_dmp_batch_lds_bytes(gnode_graph_t g) {
    if (!g) return 0;
    return 5 * dmp_align16((size_t)g->nnz * 4) + 3 * dmp_align16((size_t)g->info.n * 4);      // theta x2, phi, ps, rev | P, Pi, Pr
}
static bool dmp_batch_one_workgroup(gnode_graph_t g) {
#ifdef GN_DMP_BATCH_GENERAL_ONLY        // a measurement build (tools/bench_dmp_batch.py --lib): the general form at every size
    return false;
#else
    return gnode_dmp_batch_lds_bytes(g) <= kDmpLdsLimit;
#endif
}

// One workgroup = one sample, every step.  Thread `tid` owns nodes and edges tid, tid + blockDim.x, ... in both passes; the
// barriers sit in uniform control flow (the step loop's bounds are kernel arguments), so every thread reaches each of them.
__global__ __launch_bounds__(1024) void k_dmp_batch_wg(const int* __restrict__ rowptr, const int* __restrict__ src,
                                                      const int* __restrict__ rev_g, DmpBatchArgs a) {
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
    for (int e = tid; e < nnz; e += nt) {
        const int u = src[e];
        dmp_edge_start(s.s0[(size_t)u * 3], s.s0[(size_t)u * 3 + 1], s.w[e], theta[0][e], phi[e], ps[e]);
        rev[e] = rev_g[e];
    }
    __syncthreads();
    for (int t = 1; t < a.maxTime; ++t) {
        const float* th = theta[(t - 1) & 1];
        float* th_next = theta[t & 1];
        for (int k = tid; k < n; k += nt) {                               // node pass
            const float p = dmp_row_product(rev, th, rowptr[k], rowptr[k + 1]);
            P[k] = p;
            float sk, pi, pr;
            dmp_node_update(p, s.s0[(size_t)k * 3], Pi[k], Pr[k], s.gamma[k], sk, pi, pr);
            Pr[k] = pr; Pi[k] = pi;
            dmp_store3(s.out + (size_t)t * n * 3, k, sk, pi, pr);
        }
        __syncthreads();                                                  // P is complete; theta[cur] is still this step's
        if (t + 1 < a.maxTime)                                            // (the last step's messages have no reader)
            for (int e = tid; e < nnz; e += nt) {                         // edge pass
                const int u = src[e];
                dmp_edge_update(P[u], th[rev[e]], s.s0[(size_t)u * 3], s.w[e], s.gamma[u], phi[e], ps[e], th[e], th_next[e]);
            }
        __syncthreads();                                                  // theta[next] is complete before its node pass
    }
}

// The general form: `per` blocks of 256 per sample, sample b = blockIdx.x / per.  Per-sample state is at row b * n + k and
// edge slot b * nnz + e of the workspace arrays.
__global__ __launch_bounds__(256) void k_dmp_batch_out0(DmpBatchArgs a, unsigned per) {
    const int k = (int)(blockIdx.x % per) * 256 + threadIdx.x;
    if (k >= a.n) return;
    const DmpSample s = dmp_sample(a, blockIdx.x / per);
    dmp_store3(s.out, k, s.s0[(size_t)k * 3], s.s0[(size_t)k * 3 + 1], s.s0[(size_t)k * 3 + 2]);
}

// gnode_dmp_f32's start: the state of a 0/1 seed vector is (1 - seed, seed, 0) (dmp.py's _set_seeds), exact in fp32.  It IS
// output row 0, and the run reads it back from there as its `init`.
__global__ __launch_bounds__(256) void k_dmp_seed_out0(const float* __restrict__ seed, int n, float* __restrict__ out0) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < n) dmp_store3(out0, k, 1.0f - seed[k], seed[k], 0.0f);
}

__global__ __launch_bounds__(256) void k_dmp_batch_init(const int* __restrict__ src, DmpBatchArgs a, unsigned per,
                                                       float* __restrict__ theta, float* __restrict__ phi, float* __restrict__ ps) {
    const size_t b = blockIdx.x / per;
    const long e = (long)(blockIdx.x % per) * 256 + threadIdx.x;
    if (e >= a.nnz) return;
    const DmpSample s = dmp_sample(a, b);
    const size_t slot = b * (size_t)a.nnz + e, u = src[e];
    dmp_edge_start(s.s0[u * 3], s.s0[u * 3 + 1], s.w[e], theta[slot], phi[slot], ps[slot]);
}

__global__ __launch_bounds__(256) void k_dmp_batch_node(const int* __restrict__ rowptr, const int* __restrict__ rev,
                                                       const float* __restrict__ theta, DmpBatchArgs a, unsigned per, int t,
                                                       float* __restrict__ P, float* __restrict__ Pr, float* __restrict__ Pi) {
    const size_t b = blockIdx.x / per;
    const int k = (int)(blockIdx.x % per) * 256 + threadIdx.x;
    if (k >= a.n) return;
    const DmpSample s = dmp_sample(a, b);
    const size_t r = b * (size_t)a.n + k;
    const float p = dmp_row_product(rev, theta + b * (size_t)a.nnz, rowptr[k], rowptr[k + 1]);
    P[r] = p;
    float sk, pi, pr;                                                     // step 1 starts from the state itself
    dmp_node_update(p, s.s0[(size_t)k * 3], t == 1 ? s.s0[(size_t)k * 3 + 1] : Pi[r], t == 1 ? s.s0[(size_t)k * 3 + 2] : Pr[r], s.gamma[k],
                    sk, pi, pr);
    Pr[r] = pr; Pi[r] = pi;
    dmp_store3(s.out + (size_t)t * a.n * 3, k, sk, pi, pr);
}

__global__ __launch_bounds__(256) void k_dmp_batch_edge(const int* __restrict__ src, const int* __restrict__ rev,
                                                       const float* __restrict__ P, const float* __restrict__ theta, DmpBatchArgs a,
                                                       unsigned per, float* __restrict__ phi, float* __restrict__ ps,
                                                       float* __restrict__ theta_next) {
    const size_t b = blockIdx.x / per;
    const long e = (long)(blockIdx.x % per) * 256 + threadIdx.x;
    if (e >= a.nnz) return;
    const DmpSample s = dmp_sample(a, b);
    const size_t base = b * (size_t)a.nnz, slot = base + e;
    const int u = src[e];
    const float w_e = s.w[e];
    dmp_edge_update(P[b * (size_t)a.n + u], theta[base + rev[e]], s.s0[(size_t)u * 3], w_e, s.gamma[u], phi[slot], ps[slot],
                    theta[slot], theta_next[slot]);
}

// ------------------------------------------------------------------------------------------------ the reverse sweep, once
// The gradient of sum(grad_out * out) with respect to w, gamma and the start (gnode_dmp_batch_backward_f32).  Adjoints carried
// from step t + 1 to step t: per edge theta_bar, phi_bar, q_bar (of Ps_e), per node pi_bar, pr_bar; all start at 0.  A step is
// an edge pass (the reverse of dmp_edge_update, absent at t = maxTime - 1, whose messages had no reader) and a node pass (the
// reverse of dmp_node_update and of both products: P_u and the cavity product P_u / theta[rev e], which does not depend on
// theta[rev e]).  The edge pass leaves two numbers per edge for the node pass of its source's row, which sums them in
// ascending position from 0; the node pass writes theta_bar of the reverses of its row's edges into the OTHER theta_bar
// buffer: rev is a permutation, so every slot is written once per step and nothing here is atomic.  Like the recurrence these
// round as written, and the two forms below call them on the sample's own pointers, in global memory or in LDS.  The dmp_rev_*
// functions, DmpRowSums and DmpAdjoint are gnode_dmp.h's: gnode_dmp_schedule_bwd.hip sweeps with them too.

struct DmpGradArgs {
    const float* w; long w_stride;
    const float* gamma; long gamma_stride;
    const float* init;                  // [B][n][3]
    const float* out;                   // [B][maxTime][n][3], the forward's
    const float* gout;                  // the same shape
    float *gw, *gg, *gi;                // [B][nnz], [B][n], [B][n][3]; null: not wanted
    float *th_tape, *ph_tape;           // [B][maxTime - 1][nnz]: theta_1 .. theta_{T-1} and phi_0 .. phi_{T-2}
    int n, maxTime; long nnz;
};
struct DmpGradSample {                  // sample b's own tables (the tapes are not __restrict__: written and read in one launch)
    const float* __restrict__ w; const float* __restrict__ gamma; const float* __restrict__ s0; const float* __restrict__ out;
    const float* __restrict__ gout;
    float *gw, *gg, *gi, *th_tape, *ph_tape;
    int n, maxTime; long nnz;
    __device__ __forceinline__ float* theta(int t) const { return th_tape + (size_t)(t - 1) * nnz; }    // theta_t, t >= 1
    __device__ __forceinline__ float* phi(int t) const { return ph_tape + (size_t)t * nnz; }            // phi_t, t >= 0
};
__device__ __forceinline__ DmpGradSample dmp_grad_sample(const DmpGradArgs& a, size_t b) {
    const size_t nn = (size_t)a.n, ne = (size_t)a.nnz, tape = b * (size_t)(a.maxTime - 1) * ne;
    return {a.w + b * a.w_stride, a.gamma + b * a.gamma_stride, a.init + b * nn * 3, a.out + b * (size_t)a.maxTime * nn * 3,
            a.gout + b * (size_t)a.maxTime * nn * 3, a.gw ? a.gw + b * ne : nullptr, a.gg ? a.gg + b * nn : nullptr,
            a.gi ? a.gi + b * nn * 3 : nullptr, a.th_tape + tape, a.ph_tape + tape, a.n, a.maxTime, a.nnz};
}
// The work of one thread on one element, for both forms.  The tape first: the forward's own functions, theta and phi kept.
__device__ __forceinline__ void dmp_tape_start(const DmpGradSample& s, const int* src, float* ps, long e) {
    const size_t u = src[e];
    dmp_edge_start(s.s0[u * 3], s.s0[u * 3 + 1], s.w[e], s.theta(1)[e], s.phi(0)[e], ps[e]);
}
__device__ __forceinline__ void dmp_tape_edge(const DmpGradSample& s, const int* src, const int* rev, const float* P, float* ps, int t,
                                              long e) {
    const size_t u = src[e];
    float ph = s.phi(t - 1)[e];
    dmp_edge_update(P[u], s.theta(t)[rev[e]], s.s0[u * 3], s.w[e], s.gamma[u], ph, ps[e], s.theta(t)[e], s.theta(t + 1)[e]);
    s.phi(t)[e] = ph;
}
__device__ __forceinline__ void dmp_grad_edge(const DmpGradSample& s, const DmpAdjoint& A, const int* src, int t, long e) {
    const int u = src[e];
    float w_bar = s.gw ? s.gw[e] : 0.0f;
    dmp_rev_edge(s.w[e], s.gamma[u], s.phi(t)[e], s.phi(t - 1)[e], A.tb[e], A.phb[e], A.qb[e], w_bar, A.q_tot[e], A.gamma_part[e]);
    if (s.gw) s.gw[e] = w_bar;
}
__device__ __forceinline__ void dmp_grad_node(const DmpGradSample& s, const DmpAdjoint& A, const int* rowptr, const int* rev, int t,
                                              int k) {
    const int lo = rowptr[k], hi = rowptr[k + 1];
    const bool edge_pass = t + 1 < s.maxTime;                   // (the last step's messages had no reader)
    const float* theta = s.theta(t);
    const float ps0 = s.s0[(size_t)k * 3];
    const float P = dmp_row_product(rev, theta, lo, hi);
    float gamma_bar = s.gg ? s.gg[k] : 0.0f, ps0_bar = s.gi ? s.gi[(size_t)k * 3] : 0.0f, S = 0.0f, P_bar;
    if (edge_pass) {
        const DmpRowSums sums = dmp_rev_row_sums(rev, theta, A.q_tot, A.gamma_part, lo, hi, P, ps0);
        gamma_bar = gamma_bar + sums.gamma;
        ps0_bar = ps0_bar + sums.ps0;
        S = sums.S;
    }
    const float* g = s.gout + ((size_t)t * s.n + k) * 3;
    dmp_rev_node(g[0], g[1], g[2], P, ps0, s.out[((size_t)(t - 1) * s.n + k) * 3 + 1], s.gamma[k], A.pib[k], A.prb[k], gamma_bar, ps0_bar,
                 P_bar);
    if (s.gg) s.gg[k] = gamma_bar;
    if (s.gi) s.gi[(size_t)k * 3] = ps0_bar;
    dmp_rev_theta(rev, theta, edge_pass ? A.q_tot : nullptr, lo, hi, P, ps0, P_bar * P, S, A.tb, A.tb_next);
}
// after step 1: theta_1 = (1 - w Pi_0[src]) + 1e-10, phi_0 = Pi_0[src], Ps_e^{prev} = Ps_0[src], and row 0 of `out` is the start
__device__ __forceinline__ void dmp_grad_start_edge(const DmpGradSample& s, const DmpAdjoint& A, const int* src, long e) {
    if (s.gw) s.gw[e] = s.gw[e] - s.s0[(size_t)src[e] * 3 + 1] * A.tb[e];
}
__device__ __forceinline__ void dmp_grad_start_node(const DmpGradSample& s, const DmpAdjoint& A, const int* rowptr, int k) {
    if (!s.gi) return;
    float pi0_bar = 0.0f, ps0_bar = s.gi[(size_t)k * 3];
    float q_sum = 0.0f;
    for (int e = rowptr[k]; e < rowptr[k + 1]; ++e) {
        pi0_bar = pi0_bar + (A.phb[e] - s.w[e] * A.tb[e]);
        q_sum = q_sum + A.qb[e];
    }
    ps0_bar = ps0_bar + q_sum;
    const float* g = s.gout + (size_t)k * 3;
    s.gi[(size_t)k * 3] = ps0_bar + g[0];
    s.gi[(size_t)k * 3 + 1] = pi0_bar + (A.pib[k] + g[1]);
    s.gi[(size_t)k * 3 + 2] = A.prb[k] + g[2];
}

extern "C" size_t gnode_dmp_batch_backward_lds_bytes(gnode_graph_t g) {
    if (!g) return 0;                   // theta_bar x2, phi_bar, q_bar, q_tot, gamma_part, rev | pi_bar, pr_bar
    return 7 * dmp_align16((size_t)g->nnz * 4) + 2 * dmp_align16((size_t)g->info.n * 4);
}
static bool dmp_grad_one_workgroup(gnode_graph_t g) { return gnode_dmp_batch_backward_lds_bytes(g) <= kDmpLdsLimit; }

// One workgroup = one sample: the forward again with theta and phi kept on the tape (in the workspace; Ps_e and P use the
// room of q_tot and pi_bar meanwhile), then the sweep with the adjoint state in LDS.  Thread `tid` owns nodes and edges tid,
// tid + blockDim.x, ... in every pass, so a gradient slot has one writer; the barriers sit in uniform control flow (the loops'
// bounds are kernel arguments).  What one thread writes to the tape another reads only after a barrier.
__global__ __launch_bounds__(1024) void k_dmp_grad_wg(const int* __restrict__ rowptr, const int* __restrict__ src,
                                                     const int* __restrict__ rev_g, DmpGradArgs a) {
    extern __shared__ __attribute__((aligned(16))) char dmp_smem[];
    const int n = a.n, nnz = (int)a.nnz, T = a.maxTime, tid = threadIdx.x, nt = blockDim.x;
    const size_t eb = dmp_align16((size_t)nnz * 4), nb = dmp_align16((size_t)n * 4);
    auto edges = [&](int i) { return (float*)(dmp_smem + i * eb); };
    DmpAdjoint A = {edges(0), edges(1), edges(2), edges(3), edges(4), edges(5), (float*)(dmp_smem + 7 * eb),
                          (float*)(dmp_smem + 7 * eb + nb)};
    int* rev = (int*)(dmp_smem + 6 * eb);
    float* ps = A.q_tot; float* P = A.pib;
    const DmpGradSample s = dmp_grad_sample(a, blockIdx.x);
    for (int e = tid; e < nnz; e += nt) {
        rev[e] = rev_g[e];
        dmp_tape_start(s, src, ps, e);
    }
    __syncthreads();
    for (int t = 1; t + 1 < T; ++t) {
        for (int k = tid; k < n; k += nt) P[k] = dmp_row_product(rev, s.theta(t), rowptr[k], rowptr[k + 1]);
        __syncthreads();
        for (int e = tid; e < nnz; e += nt) dmp_tape_edge(s, src, rev, P, ps, t, e);
        __syncthreads();
    }
    for (int e = tid; e < nnz; e += nt) { A.tb[e] = 0.0f; A.phb[e] = 0.0f; A.qb[e] = 0.0f; }
    for (int k = tid; k < n; k += nt) { A.pib[k] = 0.0f; A.prb[k] = 0.0f; }
    __syncthreads();
    for (int t = T - 1; t >= 1; --t, dmp_adjoint_swap(A)) {
        if (t + 1 < T)
            for (int e = tid; e < nnz; e += nt) dmp_grad_edge(s, A, src, t, e);
        __syncthreads();
        for (int k = tid; k < n; k += nt) dmp_grad_node(s, A, rowptr, rev, t, k);
        __syncthreads();
    }
    for (int e = tid; e < nnz; e += nt) dmp_grad_start_edge(s, A, src, e);
    for (int k = tid; k < n; k += nt) dmp_grad_start_node(s, A, rowptr, k);
}

// The general form: `per` blocks of 256 per sample; the adjoint state of sample b is at row b * n and edge slot b * nnz of
// the workspace arrays.
__device__ __forceinline__ DmpAdjoint dmp_adjoint_of(const DmpAdjoint& A, size_t b, int n, long nnz) {
    const size_t e = b * (size_t)nnz, k = b * (size_t)n;
    return {A.tb + e, A.tb_next + e, A.phb + e, A.qb + e, A.q_tot + e, A.gamma_part + e, A.pib + k, A.prb + k};
}
__global__ __launch_bounds__(256) void k_dmp_tape_start(const int* __restrict__ src, DmpGradArgs a, unsigned per, float* ps) {
    const size_t b = blockIdx.x / per;
    const long e = (long)(blockIdx.x % per) * 256 + threadIdx.x;
    if (e < a.nnz) dmp_tape_start(dmp_grad_sample(a, b), src, ps + b * (size_t)a.nnz, e);
}
__global__ __launch_bounds__(256) void k_dmp_tape_node(const int* __restrict__ rowptr, const int* __restrict__ rev, DmpGradArgs a,
                                                      unsigned per, int t, float* __restrict__ P) {
    const size_t b = blockIdx.x / per;
    const int k = (int)(blockIdx.x % per) * 256 + threadIdx.x;
    if (k < a.n) P[b * (size_t)a.n + k] = dmp_row_product(rev, dmp_grad_sample(a, b).theta(t), rowptr[k], rowptr[k + 1]);
}
__global__ __launch_bounds__(256) void k_dmp_tape_edge(const int* __restrict__ src, const int* __restrict__ rev, const float* __restrict__ P,
                                                      DmpGradArgs a, unsigned per, int t, float* ps) {
    const size_t b = blockIdx.x / per;
    const long e = (long)(blockIdx.x % per) * 256 + threadIdx.x;
    if (e < a.nnz) dmp_tape_edge(dmp_grad_sample(a, b), src, rev, P + b * (size_t)a.n, ps + b * (size_t)a.nnz, t, e);
}
__global__ __launch_bounds__(256) void k_dmp_grad_edge(const int* __restrict__ src, DmpGradArgs a, DmpAdjoint A, unsigned per, int t) {
    const size_t b = blockIdx.x / per;
    const long e = (long)(blockIdx.x % per) * 256 + threadIdx.x;
    if (e < a.nnz) dmp_grad_edge(dmp_grad_sample(a, b), dmp_adjoint_of(A, b, a.n, a.nnz), src, t, e);
}
__global__ __launch_bounds__(256) void k_dmp_grad_node(const int* __restrict__ rowptr, const int* __restrict__ rev, DmpGradArgs a,
                                                      DmpAdjoint A, unsigned per, int t) {
    const size_t b = blockIdx.x / per;
    const int k = (int)(blockIdx.x % per) * 256 + threadIdx.x;
    if (k < a.n) dmp_grad_node(dmp_grad_sample(a, b), dmp_adjoint_of(A, b, a.n, a.nnz), rowptr, rev, t, k);
}
__global__ __launch_bounds__(256) void k_dmp_grad_start_edge(const int* __restrict__ src, DmpGradArgs a, DmpAdjoint A, unsigned per) {
    const size_t b = blockIdx.x / per;
    const long e = (long)(blockIdx.x % per) * 256 + threadIdx.x;
    if (e < a.nnz) dmp_grad_start_edge(dmp_grad_sample(a, b), dmp_adjoint_of(A, b, a.n, a.nnz), src, e);
}
__global__ __launch_bounds__(256) void k_dmp_grad_start_node(const int* __restrict__ rowptr, DmpGradArgs a, DmpAdjoint A, unsigned per) {
    const size_t b = blockIdx.x / per;
    const int k = (int)(blockIdx.x % per) * 256 + threadIdx.x;
    if (k < a.n) dmp_grad_start_node(dmp_grad_sample(a, b), dmp_adjoint_of(A, b, a.n, a.nnz), rowptr, k);
}

int gn_dmp_set_attributes() {       // once per device, from gnode_graph_create
    GN_HIP(hipFuncSetAttribute((const void*)k_dmp_batch_wg, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDmpLdsLimit));
    GN_HIP(hipFuncSetAttribute((const void*)k_dmp_grad_wg, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDmpLdsLimit));
    return 0;
}

// ------------------------------------------------------------------------------------------------ the host side, once
// The workspace of a call: room no kernel uses any more (src, rev and a status word lay there while every call built them; the
// handle holds them now) -- the size queries are pinned by tests/golden/dmp_parent.json -- then for the general form theta x2,
// phi, ps over B * nnz edge slots and P, Pr, Pi over B * n rows; for the solo entries the 0/1 seed vector after them.  With
// `base` null only `bytes` means anything.
struct DmpWorkspace {
    float *theta[2], *phi, *ps, *P, *Pr, *Pi, *seed;
    size_t bytes;
};
static DmpWorkspace dmp_carve(gnode_graph_t g, size_t B, bool general, bool seed_vector, void* base) {
    const size_t edges = (size_t)std::max<int64_t>(g->nnz, 1), eb = gn_align(edges * 4);
    const size_t EB = general ? gn_align(B * edges * 4) : 0, NB = general ? gn_align(B * (size_t)g->info.n * 4) : 0;
    size_t at = 0;
    auto take = [&](size_t bytes) { char* p = base ? (char*)base + at : nullptr; at += bytes; return (float*)p; };
    DmpWorkspace w;
    take(2 * eb + 256);
    w.theta[0] = take(EB); w.theta[1] = take(EB); w.phi = take(EB); w.ps = take(EB);
    w.P = take(NB); w.Pr = take(NB); w.Pi = take(NB);
    w.seed = take(seed_vector ? gn_align((size_t)g->info.n * 4) : 0);
    w.bytes = at;
    return w;
}
// A solo call is always the general form (dmp_run), and both solo entries ask for the seed vector's room: 6 eb + 4 nb + 256.
extern "C" size_t gnode_dmp_workspace_bytes(gnode_graph_t g) { return g ? dmp_carve(g, 1, true, true, nullptr).bytes : 0; }
extern "C" size_t gnode_dmp_init_workspace_bytes(gnode_graph_t g) { return gnode_dmp_workspace_bytes(g); }   // (the seed vector rests)
extern "C" size_t gnode_dmp_batch_workspace_bytes(gnode_graph_t g, int32_t B) {
    return g && B >= 1 ? dmp_carve(g, (size_t)B, !dmp_batch_one_workgroup(g), false, nullptr).bytes : 0;
}

// What a forward or a backward call settles before it writes anything, in this order: its arguments, the form and its launch
// shape, the workspace's size, the pattern's symmetry.
//   who       the entry's name for the messages        pointers   whether the entry's own pointers are all there
//   wanted    whether some output is asked for         solo       a solo entry: the general form at every size
//   fits      whether the direction's one-workgroup form serves this graph; need(general): its workspace bytes
struct DmpShape {
    int n; long nnz;
    bool one_wg;
    unsigned ng, eg;                    // blocks of 256 per sample over the nodes and over the edges (the general form)
    unsigned threads;                   // of the one workgroup per sample
};
template <class Need>
static int dmp_preamble(const char* who, gnode_graph_t g, const float* weights, long w_stride, const float* gamma, long gamma_stride,
                        bool pointers, const int32_t* seeds_host, int32_t n_seeds, bool wanted, int32_t B, int32_t maxTime, bool solo,
                        bool (*fits)(gnode_graph_t), Need need, size_t workspace_bytes, DmpShape* s) {
    GN_CHECK_ARG(g && gamma && pointers, "%s: null pointer", who);
    GN_CHECK_ARG(weights || g->nnz == 0, "%s: weights is null", who);          // no edge, no weight: an empty tensor has no address
    GN_CHECK_ARG(maxTime >= 2, "%s: maxTime must be >= 2 (got %d)", who, maxTime);
    GN_CHECK_ARG(B >= 1, "%s: B must be >= 1 (got %d)", who, B);
    GN_CHECK_ARG(w_stride == 0 || w_stride == g->nnz, "%s: w_stride must be 0 or nnz = %ld (got %ld)", who, (long)g->nnz, w_stride);
    GN_CHECK_ARG(gamma_stride == 0 || gamma_stride == g->info.n, "%s: gamma_stride must be 0 or n = %d (got %ld)", who, g->info.n, gamma_stride);
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

// B samples.  `solo`: one of the two solo entries, which take the general form at every size and carve the solo workspace.
// init == nullptr: gnode_dmp_f32, whose n_seeds seeds become output row 0, the run's init.
static int dmp_run(const char* who, gnode_graph_t g, const float* weights, long w_stride, const float* gamma, long gamma_stride,
                   const float* init, const int32_t* seeds_host, int32_t n_seeds, int32_t B, int32_t maxTime, float* out, bool solo,
                   void* workspace, size_t workspace_bytes, void* stream) {
    DmpShape s;
    if (int rc = dmp_preamble(who, g, weights, w_stride, gamma, gamma_stride, (init || seeds_host || n_seeds == 0) && out && workspace,
                              seeds_host, n_seeds, true, B, maxTime, solo, dmp_batch_one_workgroup,
                              [&](bool general) { return dmp_carve(g, (size_t)B, general, solo, nullptr).bytes; }, workspace_bytes, &s))
        return rc;
    const int n = s.n;
    const unsigned ng = s.ng, eg = s.eg;
    const DmpWorkspace ws = dmp_carve(g, (size_t)B, !s.one_wg, solo, workspace);
    hipStream_t st = (hipStream_t)stream;
    const float one = 1.0f;
    if (!init) {
        GN_HIP(hipMemsetAsync(ws.seed, 0, (size_t)n * 4, st));
        for (int i = 0; i < n_seeds; ++i) GN_HIP(hipMemcpyAsync(ws.seed + seeds_host[i], &one, 4, hipMemcpyHostToDevice, st));
    }
    // `one` and seeds_host are done with.  For the entries without a seed list nothing waits on the host any more: only the
    // documented contract ("Synchronises `stream`", include/gnode.h) keeps the call there
    GN_HIP(hipStreamSynchronize(st));
    const DmpBatchArgs a = {weights, w_stride, gamma, gamma_stride, init ? init : out, out, n, maxTime, s.nnz};
    if (s.one_wg) {
        hipLaunchKernelGGL(k_dmp_batch_wg, dim3((unsigned)B), dim3(s.threads), gnode_dmp_batch_lds_bytes(g), st, g->rowptr, g->src, g->rev, a);
        GN_LAUNCH_CHECK();
        return 0;
    }
    const dim3 gn((unsigned)B * ng), ge((unsigned)B * eg);
    if (init) hipLaunchKernelGGL(k_dmp_batch_out0, gn, dim3(256), 0, st, a, ng);
    else hipLaunchKernelGGL(k_dmp_seed_out0, gn, dim3(256), 0, st, ws.seed, n, out);
    hipLaunchKernelGGL(k_dmp_batch_init, ge, dim3(256), 0, st, g->src, a, eg, ws.theta[0], ws.phi, ws.ps);
    GN_LAUNCH_CHECK();
    for (int t = 1; t < maxTime; ++t) {
        const int cur = (t - 1) & 1;
        hipLaunchKernelGGL(k_dmp_batch_node, gn, dim3(256), 0, st, g->rowptr, g->rev, ws.theta[cur], a, ng, t, ws.P, ws.Pr, ws.Pi);
        if (t + 1 < maxTime)                 // (the last step's messages have no reader)
            hipLaunchKernelGGL(k_dmp_batch_edge, ge, dim3(256), 0, st, g->src, g->rev, ws.P, ws.theta[cur], a, eg, ws.phi, ws.ps, ws.theta[cur ^ 1]);
        GN_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int gnode_dmp_f32(gnode_graph_t g, const float* weights, const float* gamma, const int32_t* seeds_host,
                             int32_t n_seeds, int32_t maxTime, float* out, void* workspace, size_t workspace_bytes,
                             void* stream) {
    return dmp_run("gnode_dmp_f32", g, weights, 0, gamma, 0, nullptr, seeds_host, n_seeds, 1, maxTime, out, true, workspace, workspace_bytes,
                   stream);
}

extern "C" int gnode_dmp_init_f32(gnode_graph_t g, const float* weights, const float* gamma, const float* init, int32_t maxTime,
                                  float* out, void* workspace, size_t workspace_bytes, void* stream) {
    GN_CHECK_ARG(init, "gnode_dmp_init_f32: null pointer");
    return dmp_run("gnode_dmp_init_f32", g, weights, 0, gamma, 0, init, nullptr, 0, 1, maxTime, out, true, workspace, workspace_bytes, stream);
}

extern "C" int gnode_dmp_batch_f32(gnode_graph_t g, const float* weights, int64_t w_stride, const float* gamma, int64_t gamma_stride,
                                   const float* init, int32_t B, int32_t maxTime, float* out, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    GN_CHECK_ARG(init, "gnode_dmp_batch_f32: null pointer");
    return dmp_run("gnode_dmp_batch_f32", g, weights, (long)w_stride, gamma, (long)gamma_stride, init, nullptr, 0, B, maxTime, out, false,
                   workspace, workspace_bytes, stream);
}

// ------------------------------------------------------------------------------------------------ the reverse sweep's host side
// The workspace of a backward call: the same unused room as dmp_carve's (sizes pinned by tests/golden/edge_tables_parent.json) | the
// tapes of theta and phi, B * (maxTime - 1) * nnz each; for the general form Ps_e, theta_bar x2, phi_bar, q_bar, q_tot, gamma_part
// over B * nnz edge slots and P, pi_bar, pr_bar over B * n rows.
struct DmpGradWorkspace {
    float *th_tape, *ph_tape, *ps, *P;
    DmpAdjoint adj;
    size_t bytes;
};
static DmpGradWorkspace dmp_grad_carve(gnode_graph_t g, size_t B, size_t maxTime, bool general, void* base) {
    const size_t edges = (size_t)std::max<int64_t>(g->nnz, 1), eb = gn_align(edges * 4), tape = gn_align(B * (maxTime - 1) * edges * 4);
    const size_t EB = general ? gn_align(B * edges * 4) : 0, NB = general ? gn_align(B * (size_t)g->info.n * 4) : 0;
    size_t at = 0;
    auto take = [&](size_t bytes) { char* p = base ? (char*)base + at : nullptr; at += bytes; return (float*)p; };
    DmpGradWorkspace w;
    take(2 * eb + 256);
    w.th_tape = take(tape); w.ph_tape = take(tape);
    w.ps = take(EB); w.P = take(NB);
    w.adj.tb = take(EB); w.adj.tb_next = take(EB); w.adj.phb = take(EB); w.adj.qb = take(EB); w.adj.q_tot = take(EB);
    w.adj.gamma_part = take(EB); w.adj.pib = take(NB); w.adj.prb = take(NB);
    w.bytes = at;
    return w;
}
extern "C" size_t gnode_dmp_batch_backward_workspace_bytes(gnode_graph_t g, int32_t B, int32_t maxTime) {
    return g && B >= 1 && maxTime >= 2 ? dmp_grad_carve(g, (size_t)B, (size_t)maxTime, !dmp_grad_one_workgroup(g), nullptr).bytes : 0;
}
extern "C" size_t gnode_dmp_backward_workspace_bytes(gnode_graph_t g, int32_t maxTime) {      // a solo call is the general form
    return g && maxTime >= 2 ? dmp_grad_carve(g, 1, (size_t)maxTime, true, nullptr).bytes : 0;
}

// B samples; `solo`: gnode_dmp_backward_f32, the general form at every size
static int dmp_grad_run(const char* who, gnode_graph_t g, const float* weights, long w_stride, const float* gamma, long gamma_stride,
                        const float* init, int32_t B, int32_t maxTime, const float* out, const float* grad_out, float* grad_w,
                        float* grad_gamma, float* grad_init, bool solo, void* workspace, size_t workspace_bytes, void* stream) {
    DmpShape s;
    if (int rc = dmp_preamble(who, g, weights, w_stride, gamma, gamma_stride, init && out && grad_out && workspace, nullptr, 0,
                              grad_w || grad_gamma || grad_init, B, maxTime, solo, dmp_grad_one_workgroup,
                              [&](bool general) { return dmp_grad_carve(g, (size_t)B, (size_t)maxTime, general, nullptr).bytes; },
                              workspace_bytes, &s))
        return rc;
    const long nnz = s.nnz;
    const int n = s.n;
    const unsigned ng = s.ng, eg = s.eg;
    const DmpGradWorkspace ws = dmp_grad_carve(g, (size_t)B, (size_t)maxTime, !s.one_wg, workspace);
    hipStream_t st = (hipStream_t)stream;
    GN_HIP(hipStreamSynchronize(st));          // nothing waits on the host here: only the documented contract (include/gnode.h) keeps it
    if (grad_w && nnz) GN_HIP(hipMemsetAsync(grad_w, 0, (size_t)B * nnz * 4, st));         // the sweep accumulates into them
    if (grad_gamma) GN_HIP(hipMemsetAsync(grad_gamma, 0, (size_t)B * n * 4, st));
    if (grad_init) GN_HIP(hipMemsetAsync(grad_init, 0, (size_t)B * n * 12, st));
    const DmpGradArgs a = {weights, w_stride, gamma, gamma_stride, init, out, grad_out, grad_w, grad_gamma, grad_init, ws.th_tape, ws.ph_tape,
                           n, maxTime, nnz};
    if (s.one_wg) {
        hipLaunchKernelGGL(k_dmp_grad_wg, dim3((unsigned)B), dim3(s.threads), gnode_dmp_batch_backward_lds_bytes(g), st, g->rowptr, g->src,
                           g->rev, a);
        GN_LAUNCH_CHECK();
        return 0;
    }
    const dim3 gn((unsigned)B * ng), ge((unsigned)B * eg);
    hipLaunchKernelGGL(k_dmp_tape_start, ge, dim3(256), 0, st, g->src, a, eg, ws.ps);
    for (int t = 1; t + 1 < maxTime; ++t) {
        hipLaunchKernelGGL(k_dmp_tape_node, gn, dim3(256), 0, st, g->rowptr, g->rev, a, ng, t, ws.P);
        hipLaunchKernelGGL(k_dmp_tape_edge, ge, dim3(256), 0, st, g->src, g->rev, ws.P, a, eg, t, ws.ps);
    }
    GN_LAUNCH_CHECK();
    for (float* zero : {ws.adj.tb, ws.adj.phb, ws.adj.qb}) GN_HIP(hipMemsetAsync(zero, 0, (size_t)B * std::max<long>(nnz, 1) * 4, st));
    for (float* zero : {ws.adj.pib, ws.adj.prb}) GN_HIP(hipMemsetAsync(zero, 0, (size_t)B * n * 4, st));
    DmpAdjoint A = ws.adj;
    for (int t = maxTime - 1; t >= 1; --t, dmp_adjoint_swap(A)) {
        if (t + 1 < maxTime) hipLaunchKernelGGL(k_dmp_grad_edge, ge, dim3(256), 0, st, g->src, a, A, eg, t);
        hipLaunchKernelGGL(k_dmp_grad_node, gn, dim3(256), 0, st, g->rowptr, g->rev, a, A, ng, t);
        GN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_dmp_grad_start_edge, ge, dim3(256), 0, st, g->src, a, A, eg);
    hipLaunchKernelGGL(k_dmp_grad_start_node, gn, dim3(256), 0, st, g->rowptr, a, A, ng);
    GN_LAUNCH_CHECK();
    return 0;
}

extern "C" int gnode_dmp_batch_backward_f32(gnode_graph_t g, const float* weights, int64_t w_stride, const float* gamma, int64_t gamma_stride,
                                            const float* init, int32_t B, int32_t maxTime, const float* out, const float* grad_out,
                                            float* grad_w, float* grad_gamma, float* grad_init, void* workspace, size_t workspace_bytes,
                                            void* stream) {
    return dmp_grad_run("gnode_dmp_batch_backward_f32", g, weights, (long)w_stride, gamma, (long)gamma_stride, init, B, maxTime, out, grad_out,
                        grad_w, grad_gamma, grad_init, false, workspace, workspace_bytes, stream);
}

extern "C" int gnode_dmp_backward_f32(gnode_graph_t g, const float* weights, const float* gamma, const float* init, int32_t maxTime,
                                      const float* out, const float* grad_out, float* grad_w, float* grad_gamma, float* grad_init,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    return dmp_grad_run("gnode_dmp_backward_f32", g, weights, 0, gamma, 0, init, 1, maxTime, out, grad_out, grad_w, grad_gamma, grad_init, true,
                        workspace, workspace_bytes, stream);
}
