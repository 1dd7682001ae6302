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
// ascending order -- the order the reference's CPU scatter uses.  fp32 like the reference's FloatTensors; two
// launches per time step (node pass, edge pass), theta ping-pongs because the edge pass reads its neighbours'.
#include "gnode_common.h"
#include <algorithm>

__global__ __launch_bounds__(256) void k_dmp_setup(const int* __restrict__ rowptr, const int* __restrict__ col, int n,
                                                  int* __restrict__ src, int* __restrict__ rev, int* __restrict__ bad) {
    const int u = blockIdx.x * 256 + threadIdx.x;
    if (u >= n) return;
    for (int e = rowptr[u]; e < rowptr[u + 1]; ++e) {
        const int v = col[e];
        src[e] = u;
        int lo = rowptr[v], hi = rowptr[v + 1] - 1, found = -1;       // position of u in row v (sorted columns)
        while (lo <= hi) {
            const int mid = (lo + hi) >> 1, c = col[mid];
            if (c == u) { found = mid; break; }
            if (c < u) lo = mid + 1; else hi = mid - 1;
        }
        rev[e] = found;
        if (found < 0) atomicExch(bad, 1);
    }
}

// The initial marginals of node k.  INIT = false: from the 0/1 seed vector (Ps0 = 1 - seed, Pi0 = seed, Pr0 = 0: dmp.py's
// _set_seeds).  INIT = true (gnode_dmp_init_f32): the caller's fp32 [n][3] = (pS, pI, pR), and the message of an edge starts
// from Phi_0 = Pi0[src] -- what 1 - Ps0 is when Pr0 = 0.  The seed instances compile to what they were.
template <bool INIT> __device__ __forceinline__ float dmp_ps0(const float* __restrict__ s0, int k) { return INIT ? s0[(size_t)k * 3] : 1.0f - s0[k]; }
template <bool INIT> __device__ __forceinline__ float dmp_pi0(const float* __restrict__ s0, int k) { return INIT ? s0[(size_t)k * 3 + 1] : s0[k]; }
template <bool INIT> __device__ __forceinline__ float dmp_pr0(const float* __restrict__ s0, int k) { return INIT ? s0[(size_t)k * 3 + 2] : 0.0f; }

// t = 1 (dmp.py:104-121): theta_1 = 1 - w phi_0 + 1e-10, Ps_e^{prev} = Ps0[src]
template <bool INIT>
__global__ __launch_bounds__(256) void k_dmp_init(const int* __restrict__ src, const float* __restrict__ w,
                                                 const float* __restrict__ seed, long nnz, float* __restrict__ theta,
                                                 float* __restrict__ phi, float* __restrict__ ps) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz) return;
    const float ps0 = dmp_ps0<INIT>(seed, src[e]);
    const float ph = INIT ? dmp_pi0<INIT>(seed, src[e]) : 1.0f - ps0;
    theta[e] = (1.0f - w[e] * ph) + 1e-10f;
    phi[e] = ph;
    ps[e] = ps0;
}

// node pass: P_k and the marginals of time step t
template <bool INIT>
__global__ __launch_bounds__(256) void k_dmp_node(const int* __restrict__ rowptr, const int* __restrict__ rev,
                                                 const float* __restrict__ theta, const float* __restrict__ seed,
                                                 const float* __restrict__ gamma, int n, int first, float* __restrict__ P,
                                                 float* __restrict__ Pr, float* __restrict__ Pi, float* __restrict__ out_t) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    float p = 1.0f;
    for (int e = rowptr[k]; e < rowptr[k + 1]; ++e) p = p * theta[rev[e]];
    P[k] = p;
    const float ps0 = dmp_ps0<INIT>(seed, k);
    const float ps = ps0 * p;
    const float pi_prev = first ? dmp_pi0<INIT>(seed, k) : Pi[k];
    const float pr = (first ? dmp_pr0<INIT>(seed, k) : Pr[k]) + gamma[k] * pi_prev;
    const float pi = 1.0f - ps - pr;
    Pr[k] = pr; Pi[k] = pi;
    out_t[(size_t)k * 3 + 0] = ps; out_t[(size_t)k * 3 + 1] = pi; out_t[(size_t)k * 3 + 2] = pr;
}

// edge pass: Ps_e, phi_e of this step, theta of the NEXT step into the other buffer
template <bool INIT>
__global__ __launch_bounds__(256) void k_dmp_edge(const int* __restrict__ src, const int* __restrict__ rev,
                                                 const float* __restrict__ w, const float* __restrict__ gamma,
                                                 const float* __restrict__ seed, const float* __restrict__ P,
                                                 const float* __restrict__ theta, long nnz, float* __restrict__ phi,
                                                 float* __restrict__ ps, float* __restrict__ theta_next) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz) return;
    const int u = src[e];
    const float mul = P[u] / theta[rev[e]];
    const float ps_new = dmp_ps0<INIT>(seed, u) * mul;
    const float ph = (1.0f - w[e]) * (1.0f - gamma[u]) * phi[e] - (ps_new - ps[e]);
    phi[e] = ph;
    ps[e] = ps_new;
    theta_next[e] = theta[e] - w[e] * ph;
}

template <bool INIT>
__global__ __launch_bounds__(256) void k_dmp_out0(const float* __restrict__ seed, int n, float* __restrict__ out0) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    out0[(size_t)k * 3 + 0] = dmp_ps0<INIT>(seed, k); out0[(size_t)k * 3 + 1] = dmp_pi0<INIT>(seed, k); out0[(size_t)k * 3 + 2] = dmp_pr0<INIT>(seed, k);
}

extern "C" size_t gnode_dmp_workspace_bytes(gnode_graph_t g) {
    if (!g) return 0;
    const size_t eb = gn_align((size_t)std::max<int64_t>(g->nnz, 1) * 4), nb = gn_align((size_t)g->info.n * 4);
    return 6 * eb + 4 * nb + 256;          // src, rev, theta x2, phi, ps | seed, P, Pr, Pi | status
}
extern "C" size_t gnode_dmp_init_workspace_bytes(gnode_graph_t g) { return gnode_dmp_workspace_bytes(g); }   // (the seed vector rests)

// INIT = false: the seed list is staged as a 0/1 vector in the workspace.  INIT = true: `init` is the caller's device fp32
// [n][3], read where the seed vector is.  `who`: the entry's name for the messages.
template <bool INIT>
static int dmp_impl(const char* who, gnode_graph_t g, const float* weights, const float* gamma, const int32_t* seeds_host,
                    int32_t n_seeds, const float* init, int32_t maxTime, float* out, void* workspace, size_t workspace_bytes,
                    void* stream) {
    GN_CHECK_ARG(g && gamma && out && workspace && (INIT ? init != nullptr : (seeds_host || n_seeds == 0)), "%s: null pointer", who);
    GN_CHECK_ARG(weights || g->nnz == 0, "%s: weights is null", who);          // no edge, no weight: an empty tensor has no address
    GN_CHECK_ARG(maxTime >= 2, "%s: maxTime must be >= 2 (got %d)", who, maxTime);
    for (int i = 0; i < n_seeds; ++i)
        GN_CHECK_ARG(seeds_host[i] >= 0 && seeds_host[i] < g->info.n, "%s: seed %d out of range", who, seeds_host[i]);
    if (workspace_bytes < gnode_dmp_workspace_bytes(g)) {
        gnode_set_error("%s: workspace %zu < %zu", who, workspace_bytes, gnode_dmp_workspace_bytes(g));
        return GNODE_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const long nnz = g->nnz;
    const int n = g->info.n;
    const size_t eb = gn_align((size_t)std::max<int64_t>(nnz, 1) * 4), nb = gn_align((size_t)n * 4);
    char* ws = (char*)workspace;
    int* src = (int*)ws; int* rev = (int*)(ws + eb);
    float* theta[2] = {(float*)(ws + 2 * eb), (float*)(ws + 3 * eb)};
    float* phi = (float*)(ws + 4 * eb); float* ps = (float*)(ws + 5 * eb);
    float* seed_ws = (float*)(ws + 6 * eb); float* P = (float*)(ws + 6 * eb + nb);
    float* Pr = (float*)(ws + 6 * eb + 2 * nb); float* Pi = (float*)(ws + 6 * eb + 3 * nb);
    int* bad = (int*)(ws + 6 * eb + 4 * nb);
    const float* seed = INIT ? init : seed_ws;
    if (!INIT) GN_HIP(hipMemsetAsync(seed_ws, 0, (size_t)n * 4, st));
    GN_HIP(hipMemsetAsync(bad, 0, 4, st));
    const float one = 1.0f;
    for (int i = 0; i < n_seeds; ++i) GN_HIP(hipMemcpyAsync(seed_ws + seeds_host[i], &one, 4, hipMemcpyHostToDevice, st));
    const unsigned ng = (unsigned)((n + 255) / 256), eg = (unsigned)std::max<long>(1, (nnz + 255) / 256);
    hipLaunchKernelGGL(k_dmp_setup, dim3(ng), dim3(256), 0, st, g->rowptr, g->col, n, src, rev, bad);
    GN_LAUNCH_CHECK();
    int bad_h = 0;
    GN_HIP(hipMemcpyAsync(&bad_h, bad, 4, hipMemcpyDeviceToHost, st));
    GN_HIP(hipStreamSynchronize(st));          // also: `one` and seeds_host are done with
    GN_CHECK_ARG(!bad_h, "%s: the sparsity pattern is not symmetric (DMP here serves undirected graphs)", who);
    const size_t plane = (size_t)n * 3;
    hipLaunchKernelGGL(k_dmp_out0<INIT>, dim3(ng), dim3(256), 0, st, seed, n, out);
    hipLaunchKernelGGL(k_dmp_init<INIT>, dim3(eg), dim3(256), 0, st, src, weights, seed, nnz, theta[0], phi, ps);
    GN_LAUNCH_CHECK();
    for (int t = 1; t < maxTime; ++t) {
        const int cur = (t - 1) & 1;
        hipLaunchKernelGGL(k_dmp_node<INIT>, dim3(ng), dim3(256), 0, st, g->rowptr, rev, theta[cur], seed, gamma, n, t == 1 ? 1 : 0, P, Pr,
                           Pi, out + (size_t)t * plane);
        hipLaunchKernelGGL(k_dmp_edge<INIT>, dim3(eg), dim3(256), 0, st, src, rev, weights, gamma, seed, P, theta[cur], nnz, phi, ps,
                           theta[cur ^ 1]);
        GN_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int gnode_dmp_f32(gnode_graph_t g, const float* weights, const float* gamma, const int32_t* seeds_host,
                             int32_t n_seeds, int32_t maxTime, float* out, void* workspace, size_t workspace_bytes,
                             void* stream) {
    return dmp_impl<false>("gnode_dmp_f32", g, weights, gamma, seeds_host, n_seeds, nullptr, maxTime, out, workspace, workspace_bytes, stream);
}

extern "C" int gnode_dmp_init_f32(gnode_graph_t g, const float* weights, const float* gamma, const float* init, int32_t maxTime,
                                  float* out, void* workspace, size_t workspace_bytes, void* stream) {
    return dmp_impl<true>("gnode_dmp_init_f32", g, weights, gamma, nullptr, 0, init, maxTime, out, workspace, workspace_bytes, stream);
}

// ------------------------------------------------------------------------------------------------ B samples in one call
// gnode_dmp_batch_f32: sample b starts from init[b] with weights + b * w_stride and gamma + b * gamma_stride (a stride of 0
// shares the table).  Every sample's arithmetic is the INIT instances' above, expression for expression, in the same
// per-element order, so sample b's output is gnode_dmp_init_f32's for its inputs bit for bit; `src` / `rev` are built once.
// Two forms, chosen from the graph alone (dmp_batch_one_workgroup):
//   one workgroup per sample   the messages and marginals of a sample live in LDS for the whole horizon: one launch
//   general                    the four kernels over rows r = b * n + k and edge slots b * nnz + e: two launches per step
struct DmpBatchArgs {
    const float* w; long w_stride;
    const float* gamma; long gamma_stride;
    const float* init;                  // [B][n][3]
    float* out;                         // [B][maxTime][n][3]
    int n, maxTime; long nnz;
};

__host__ __device__ static inline size_t dmp_align16(size_t x) { return (x + 15) / 16 * 16; }
static constexpr size_t kDmpLdsLimit = 160 * 1024;      // what a gfx950 workgroup may declare

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
    const size_t b = blockIdx.x, eb = dmp_align16((size_t)nnz * 4), nb = dmp_align16((size_t)n * 4);
    float* theta[2] = {(float*)dmp_smem, (float*)(dmp_smem + eb)};
    float* phi = (float*)(dmp_smem + 2 * eb); float* ps = (float*)(dmp_smem + 3 * eb);
    int* rev = (int*)(dmp_smem + 4 * eb);
    float* P = (float*)(dmp_smem + 5 * eb); float* Pi = (float*)(dmp_smem + 5 * eb + nb); float* Pr = (float*)(dmp_smem + 5 * eb + 2 * nb);
    const float* __restrict__ w = a.w + b * a.w_stride;
    const float* __restrict__ gamma = a.gamma + b * a.gamma_stride;
    const float* __restrict__ s0 = a.init + b * (size_t)n * 3;
    float* __restrict__ out = a.out + b * (size_t)a.maxTime * n * 3;
    for (int k = tid; k < n; k += nt) {                                   // k_dmp_out0; Pi, Pr hold what `first` selects
        const float ps0 = dmp_ps0<true>(s0, k), pi0 = dmp_pi0<true>(s0, k), pr0 = dmp_pr0<true>(s0, k);
        out[(size_t)k * 3 + 0] = ps0; out[(size_t)k * 3 + 1] = pi0; out[(size_t)k * 3 + 2] = pr0;
        Pi[k] = pi0; Pr[k] = pr0;
    }
    for (int e = tid; e < nnz; e += nt) {                                 // k_dmp_init
        const int u = src[e];
        const float ps0 = dmp_ps0<true>(s0, u), ph = dmp_pi0<true>(s0, u);
        theta[0][e] = (1.0f - w[e] * ph) + 1e-10f;
        phi[e] = ph;
        ps[e] = ps0;
        rev[e] = rev_g[e];
    }
    __syncthreads();
    for (int t = 1; t < a.maxTime; ++t) {
        const float* th = theta[(t - 1) & 1];
        float* th_next = theta[t & 1];
        float* __restrict__ out_t = out + (size_t)t * n * 3;
        for (int k = tid; k < n; k += nt) {                               // k_dmp_node
            float p = 1.0f;
            for (int e = rowptr[k]; e < rowptr[k + 1]; ++e) p = p * th[rev[e]];
            P[k] = p;
            const float s = dmp_ps0<true>(s0, k) * p;
            const float pr = Pr[k] + gamma[k] * Pi[k];
            const float pi = 1.0f - s - pr;
            Pr[k] = pr; Pi[k] = pi;
            out_t[(size_t)k * 3 + 0] = s; out_t[(size_t)k * 3 + 1] = pi; out_t[(size_t)k * 3 + 2] = pr;
        }
        __syncthreads();                                                  // P is complete; theta[cur] is still this step's
        if (t + 1 < a.maxTime)                                            // (the last step's messages have no reader)
            for (int e = tid; e < nnz; e += nt) {                         // k_dmp_edge
                const int u = src[e];
                const float mul = P[u] / th[rev[e]];
                const float ps_new = dmp_ps0<true>(s0, u) * mul;
                const float ph = (1.0f - w[e]) * (1.0f - gamma[u]) * phi[e] - (ps_new - ps[e]);
                phi[e] = ph;
                ps[e] = ps_new;
                th_next[e] = th[e] - w[e] * ph;
            }
        __syncthreads();                                                  // theta[next] is complete before its node pass
    }
}

// The general form: `per` blocks of 256 per sample, sample b = blockIdx.x / per.  Per-sample state is at row b * n + k and
// edge slot b * nnz + e of the workspace arrays.
__global__ __launch_bounds__(256) void k_dmp_batch_out0(DmpBatchArgs a, unsigned per) {
    const size_t b = blockIdx.x / per;
    const int k = (int)(blockIdx.x % per) * 256 + threadIdx.x;
    if (k >= a.n) return;
    const float* __restrict__ s0 = a.init + b * (size_t)a.n * 3;
    float* __restrict__ out0 = a.out + b * (size_t)a.maxTime * a.n * 3;
    out0[(size_t)k * 3 + 0] = dmp_ps0<true>(s0, k); out0[(size_t)k * 3 + 1] = dmp_pi0<true>(s0, k); out0[(size_t)k * 3 + 2] = dmp_pr0<true>(s0, k);
}

__global__ __launch_bounds__(256) void k_dmp_batch_init(const int* __restrict__ src, DmpBatchArgs a, unsigned per,
                                                       float* __restrict__ theta, float* __restrict__ phi, float* __restrict__ ps) {
    const size_t b = blockIdx.x / per;
    const long e = (long)(blockIdx.x % per) * 256 + threadIdx.x;
    if (e >= a.nnz) return;
    const float* __restrict__ s0 = a.init + b * (size_t)a.n * 3;
    const size_t slot = b * (size_t)a.nnz + e;
    const float ps0 = dmp_ps0<true>(s0, src[e]);
    const float ph = dmp_pi0<true>(s0, src[e]);
    theta[slot] = (1.0f - a.w[b * a.w_stride + e] * ph) + 1e-10f;
    phi[slot] = ph;
    ps[slot] = ps0;
}

__global__ __launch_bounds__(256) void k_dmp_batch_node(const int* __restrict__ rowptr, const int* __restrict__ rev,
                                                       const float* __restrict__ theta, DmpBatchArgs a, unsigned per, int t,
                                                       float* __restrict__ P, float* __restrict__ Pr, float* __restrict__ Pi) {
    const size_t b = blockIdx.x / per;
    const int k = (int)(blockIdx.x % per) * 256 + threadIdx.x;
    if (k >= a.n) return;
    const float* __restrict__ s0 = a.init + b * (size_t)a.n * 3;
    const float* __restrict__ th = theta + b * (size_t)a.nnz;
    const size_t r = b * (size_t)a.n + k;
    float p = 1.0f;
    for (int e = rowptr[k]; e < rowptr[k + 1]; ++e) p = p * th[rev[e]];
    P[r] = p;
    const float ps0 = dmp_ps0<true>(s0, k);
    const float s = ps0 * p;
    const float pi_prev = t == 1 ? dmp_pi0<true>(s0, k) : Pi[r];
    const float pr = (t == 1 ? dmp_pr0<true>(s0, k) : Pr[r]) + a.gamma[b * a.gamma_stride + k] * pi_prev;
    const float pi = 1.0f - s - pr;
    Pr[r] = pr; Pi[r] = pi;
    float* __restrict__ out_t = a.out + (b * (size_t)a.maxTime + t) * a.n * 3;
    out_t[(size_t)k * 3 + 0] = s; out_t[(size_t)k * 3 + 1] = pi; out_t[(size_t)k * 3 + 2] = pr;
}

__global__ __launch_bounds__(256) void k_dmp_batch_edge(const int* __restrict__ src, const int* __restrict__ rev,
                                                       const float* __restrict__ P, const float* __restrict__ theta, DmpBatchArgs a,
                                                       unsigned per, float* __restrict__ phi, float* __restrict__ ps,
                                                       float* __restrict__ theta_next) {
    const size_t b = blockIdx.x / per;
    const long e = (long)(blockIdx.x % per) * 256 + threadIdx.x;
    if (e >= a.nnz) return;
    const float* __restrict__ s0 = a.init + b * (size_t)a.n * 3;
    const size_t base = b * (size_t)a.nnz, slot = base + e;
    const int u = src[e];
    const float we = a.w[b * a.w_stride + e];
    const float mul = P[b * (size_t)a.n + u] / theta[base + rev[e]];
    const float ps_new = dmp_ps0<true>(s0, u) * mul;
    const float ph = (1.0f - we) * (1.0f - a.gamma[b * a.gamma_stride + u]) * phi[slot] - (ps_new - ps[slot]);
    phi[slot] = ph;
    ps[slot] = ps_new;
    theta_next[slot] = theta[slot] - we * ph;
}

int gn_dmp_set_attributes() {       // once per device, from gnode_graph_create
    GN_HIP(hipFuncSetAttribute((const void*)k_dmp_batch_wg, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDmpLdsLimit));
    return 0;
}

// src, rev | status, and for the general form theta x2, phi, ps over B * nnz slots and P, Pr, Pi over B * n rows
extern "C" size_t gnode_dmp_batch_workspace_bytes(gnode_graph_t g, int32_t B) {
    if (!g || B < 1) return 0;
    const size_t eb = gn_align((size_t)std::max<int64_t>(g->nnz, 1) * 4);
    if (dmp_batch_one_workgroup(g)) return 2 * eb + 256;
    return 2 * eb + 256 + 4 * gn_align((size_t)B * (size_t)std::max<int64_t>(g->nnz, 1) * 4) + 3 * gn_align((size_t)B * (size_t)g->info.n * 4);
}

extern "C" int gnode_dmp_batch_f32(gnode_graph_t g, const float* weights, int64_t w_stride, const float* gamma, int64_t gamma_stride,
                                   const float* init, int32_t B, int32_t maxTime, float* out, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    const char* who = "gnode_dmp_batch_f32";
    GN_CHECK_ARG(g && gamma && init && out && workspace, "%s: null pointer", who);
    GN_CHECK_ARG(weights || g->nnz == 0, "%s: weights is null", who);
    GN_CHECK_ARG(B >= 1, "%s: B must be >= 1 (got %d)", who, B);
    GN_CHECK_ARG(maxTime >= 2, "%s: maxTime must be >= 2 (got %d)", who, maxTime);
    const long nnz = g->nnz;
    const int n = g->info.n;
    GN_CHECK_ARG(w_stride == 0 || w_stride == nnz, "%s: w_stride must be 0 or nnz = %ld (got %lld)", who, nnz, (long long)w_stride);
    GN_CHECK_ARG(gamma_stride == 0 || gamma_stride == n, "%s: gamma_stride must be 0 or n = %d (got %lld)", who, n, (long long)gamma_stride);
    const unsigned ng = (unsigned)((n + 255) / 256), eg = (unsigned)std::max<long>(1, (nnz + 255) / 256);
    const bool one_wg = dmp_batch_one_workgroup(g);
    GN_CHECK_ARG(one_wg || (size_t)B * std::max(ng, eg) < ((size_t)1 << 31), "%s: B = %d is too many samples for this graph", who, B);
    if (workspace_bytes < gnode_dmp_batch_workspace_bytes(g, B)) {
        gnode_set_error("%s: workspace %zu < %zu", who, workspace_bytes, gnode_dmp_batch_workspace_bytes(g, B));
        return GNODE_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t eb = gn_align((size_t)std::max<long>(nnz, 1) * 4);
    char* ws = (char*)workspace;
    int* src = (int*)ws; int* rev = (int*)(ws + eb); int* bad = (int*)(ws + 2 * eb);
    GN_HIP(hipMemsetAsync(bad, 0, 4, st));
    hipLaunchKernelGGL(k_dmp_setup, dim3(ng), dim3(256), 0, st, g->rowptr, g->col, n, src, rev, bad);
    GN_LAUNCH_CHECK();
    int bad_h = 0;
    GN_HIP(hipMemcpyAsync(&bad_h, bad, 4, hipMemcpyDeviceToHost, st));
    GN_HIP(hipStreamSynchronize(st));
    GN_CHECK_ARG(!bad_h, "%s: the sparsity pattern is not symmetric (DMP here serves undirected graphs)", who);
    const DmpBatchArgs a = {weights, (long)w_stride, gamma, (long)gamma_stride, init, out, n, maxTime, nnz};
    if (one_wg) {
        const long most = std::max<long>(n, nnz);
        const unsigned threads = (unsigned)std::min<long>(1024, std::max<long>(64, (most + 63) / 64 * 64));
        hipLaunchKernelGGL(k_dmp_batch_wg, dim3((unsigned)B), dim3(threads), gnode_dmp_batch_lds_bytes(g), st, g->rowptr, src, rev, a);
        GN_LAUNCH_CHECK();
    } else {
        const size_t EB = gn_align((size_t)B * (size_t)std::max<long>(nnz, 1) * 4), NB = gn_align((size_t)B * (size_t)n * 4);
        char* per_sample = ws + 2 * eb + 256;
        float* theta[2] = {(float*)per_sample, (float*)(per_sample + EB)};
        float* phi = (float*)(per_sample + 2 * EB); float* ps = (float*)(per_sample + 3 * EB);
        float* P = (float*)(per_sample + 4 * EB); float* Pr = (float*)(per_sample + 4 * EB + NB); float* Pi = (float*)(per_sample + 4 * EB + 2 * NB);
        const dim3 gn((unsigned)B * ng), ge((unsigned)B * eg);
        hipLaunchKernelGGL(k_dmp_batch_out0, gn, dim3(256), 0, st, a, ng);
        hipLaunchKernelGGL(k_dmp_batch_init, ge, dim3(256), 0, st, src, a, eg, theta[0], phi, ps);
        GN_LAUNCH_CHECK();
        for (int t = 1; t < maxTime; ++t) {
            const int cur = (t - 1) & 1;
            hipLaunchKernelGGL(k_dmp_batch_node, gn, dim3(256), 0, st, g->rowptr, rev, theta[cur], a, ng, t, P, Pr, Pi);
            if (t + 1 < maxTime)                 // (the last step's messages have no reader)
                hipLaunchKernelGGL(k_dmp_batch_edge, ge, dim3(256), 0, st, src, rev, P, theta[cur], a, eg, phi, ps, theta[cur ^ 1]);
            GN_LAUNCH_CHECK();
        }
    }
    return 0;
}
