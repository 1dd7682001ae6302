// DMP with rates that change over time (gnode_dmp_batch_schedule_f32): gnode_dmp_batch_f32's recurrence with P tables of
// weights and recovery probabilities and a phase table that names, per step, which of them governs it.
//
// Step t = 1 .. maxTime-1 leads from state t-1 to state t under tables p = phase[t]:
//   theta_1     = (1 - w^{phase[1]} phi_0) + 1e-10                               dmp_edge_start with step 1's weights
//   node pass t   Pr_t = Pr_{t-1} + gamma^p Pi_{t-1};  Ps_t, Pi_t as ever       dmp_node_update with step t's gamma
//   edge pass t   phi_t = (1 - w^p)(1 - gamma^p_src) phi_{t-1} - (Ps_e(t) - Ps_e(t-1))
//                 theta_{t+1} = theta_t - w^{phase[t+1]} phi_t                   dmp_edge_update with two weights
// phi_t is the probability that the source is infected and has neither transmitted nor recovered up to step t: what happened
// DURING step t, under step t's tables.  theta_{t+1} - theta_t is the probability of a transmission during step t + 1: the next
// step's weight.  The edge pass runs only when t + 1 < maxTime, so phase[t + 1] exists wherever it is read.
//
// A unit of its own, so that gnode_dmp_batch_f32's kernels are the code they were; the arithmetic is gnode_dmp.h's and nothing
// else, so one phase -- or several holding equal tables -- returns gnode_dmp_batch_f32's bits.  The same two forms, chosen by
// the same size (gnode_dmp_batch_lds_bytes: the tables are read from memory, never held in LDS): one workgroup per sample, which
// reads the device copy of the phase table wave-uniformly at every step, and the general form, whose host loop hands each
// launch the offsets of its step's tables.
#include "gnode_dmp.h"
#include <algorithm>

struct DmpSchedArgs {
    const float* w; long w_stride;      // [P][nnz] per sample, sample b at w + b * w_stride
    const float* gamma; long gamma_stride;
    const float* init;                  // [B][n][3]
    float* out;                         // [B][maxTime][n][3]
    const int32_t* phase;               // device int32 [maxTime] (the one-workgroup form reads it)
    int n, maxTime; long nnz;
};
struct DmpSchedSample {                 // sample b's own tables: w[P][nnz], gamma[P][n], the start s0[n][3], out[maxTime][n][3]
    const float* __restrict__ w; const float* __restrict__ gamma; const float* __restrict__ s0; float* __restrict__ out;
};
__device__ __forceinline__ DmpSchedSample dmp_sched_sample(const DmpSchedArgs& a, size_t b) {
    return {a.w + b * a.w_stride, a.gamma + b * a.gamma_stride, a.init + b * (size_t)a.n * 3, a.out + b * (size_t)a.maxTime * a.n * 3};
}
__device__ __forceinline__ void dmp_sched_store3(float* __restrict__ row, int k, float ps, float pi, float pr) {
    row[(size_t)k * 3 + 0] = ps; row[(size_t)k * 3 + 1] = pi; row[(size_t)k * 3 + 2] = pr;
}

static bool dmp_sched_one_workgroup(gnode_graph_t g) {
#ifdef GN_DMP_BATCH_GENERAL_ONLY        // a measurement build: the general form at every size, as gnode_dmp_batch_f32's
    return false;
#else
    return gnode_dmp_batch_lds_bytes(g) <= kDmpLdsLimit;
#endif
}

// One workgroup = one sample, every step: k_dmp_batch_wg with the step's tables chosen at the top of the step.  The phase
// reads are uniform over the workgroup, and the barriers sit in uniform control flow.
__global__ __launch_bounds__(1024) void k_dmp_sched_wg(const int* __restrict__ rowptr, const int* __restrict__ src,
                                                      const int* __restrict__ rev_g, DmpSchedArgs a) {
    extern __shared__ __attribute__((aligned(16))) char dmp_smem[];
    const int n = a.n, nnz = (int)a.nnz, tid = threadIdx.x, nt = blockDim.x;
    const size_t eb = dmp_align16((size_t)nnz * 4), nb = dmp_align16((size_t)n * 4);
    float* theta[2] = {(float*)dmp_smem, (float*)(dmp_smem + eb)};
    float* phi = (float*)(dmp_smem + 2 * eb); float* ps = (float*)(dmp_smem + 3 * eb);
    int* rev = (int*)(dmp_smem + 4 * eb);
    float* P = (float*)(dmp_smem + 5 * eb); float* Pi = (float*)(dmp_smem + 5 * eb + nb); float* Pr = (float*)(dmp_smem + 5 * eb + 2 * nb);
    const DmpSchedSample s = dmp_sched_sample(a, blockIdx.x);
    for (int k = tid; k < n; k += nt) {                                   // output row 0; Pi, Pr hold the start for step 1
        const float ps0 = s.s0[(size_t)k * 3], pi0 = s.s0[(size_t)k * 3 + 1], pr0 = s.s0[(size_t)k * 3 + 2];
        dmp_sched_store3(s.out, k, ps0, pi0, pr0);
        Pi[k] = pi0; Pr[k] = pr0;
    }
    {
        const float* w1 = s.w + (size_t)a.phase[1] * nnz;                 // (maxTime >= 2: entry 1 exists)
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
        const int p = a.phase[t];
        const float* w = s.w + (size_t)p * nnz;
        const float* gam = s.gamma + (size_t)p * n;
        for (int k = tid; k < n; k += nt) {                               // node pass
            const float pk = dmp_row_product(rev, th, rowptr[k], rowptr[k + 1]);
            P[k] = pk;
            float sk, pi, pr;
            dmp_node_update(pk, s.s0[(size_t)k * 3], Pi[k], Pr[k], gam[k], sk, pi, pr);
            Pr[k] = pr; Pi[k] = pi;
            dmp_sched_store3(s.out + (size_t)t * n * 3, k, sk, pi, pr);
        }
        __syncthreads();                                                  // P is complete; theta[cur] is still this step's
        if (t + 1 < a.maxTime) {                                          // (the last step's messages have no reader)
            const float* w_next = s.w + (size_t)a.phase[t + 1] * nnz;
            for (int e = tid; e < nnz; e += nt) {                         // edge pass
                const int u = src[e];
                dmp_edge_update(P[u], th[rev[e]], s.s0[(size_t)u * 3], w[e], w_next[e], gam[u], phi[e], ps[e], th[e], th_next[e]);
            }
        }
        __syncthreads();                                                  // theta[next] is complete before its node pass
    }
}

// The general form: gnode_dmp.hip's four kernels with the offsets of the step's tables inside a sample's [P][...] block as
// arguments (w_at = phase * nnz, g_at = phase * n, from the host loop).
__global__ __launch_bounds__(256) void k_dmp_sched_out0(DmpSchedArgs a, unsigned per) {
    const int k = (int)(blockIdx.x % per) * 256 + threadIdx.x;
    if (k >= a.n) return;
    const DmpSchedSample s = dmp_sched_sample(a, blockIdx.x / per);
    dmp_sched_store3(s.out, k, s.s0[(size_t)k * 3], s.s0[(size_t)k * 3 + 1], s.s0[(size_t)k * 3 + 2]);
}

__global__ __launch_bounds__(256) void k_dmp_sched_init(const int* __restrict__ src, DmpSchedArgs a, unsigned per, long w_at,
                                                       float* __restrict__ theta, float* __restrict__ phi, float* __restrict__ ps) {
    const size_t b = blockIdx.x / per;
    const long e = (long)(blockIdx.x % per) * 256 + threadIdx.x;
    if (e >= a.nnz) return;
    const DmpSchedSample s = dmp_sched_sample(a, b);
    const size_t slot = b * (size_t)a.nnz + e, u = src[e];
    dmp_edge_start(s.s0[u * 3], s.s0[u * 3 + 1], s.w[w_at + e], theta[slot], phi[slot], ps[slot]);
}

__global__ __launch_bounds__(256) void k_dmp_sched_node(const int* __restrict__ rowptr, const int* __restrict__ rev,
                                                       const float* __restrict__ theta, DmpSchedArgs a, unsigned per, int t, long g_at,
                                                       float* __restrict__ P, float* __restrict__ Pr, float* __restrict__ Pi) {
    const size_t b = blockIdx.x / per;
    const int k = (int)(blockIdx.x % per) * 256 + threadIdx.x;
    if (k >= a.n) return;
    const DmpSchedSample s = dmp_sched_sample(a, b);
    const size_t r = b * (size_t)a.n + k;
    const float p = dmp_row_product(rev, theta + b * (size_t)a.nnz, rowptr[k], rowptr[k + 1]);
    P[r] = p;
    float sk, pi, pr;                                                     // step 1 starts from the state itself
    dmp_node_update(p, s.s0[(size_t)k * 3], t == 1 ? s.s0[(size_t)k * 3 + 1] : Pi[r], t == 1 ? s.s0[(size_t)k * 3 + 2] : Pr[r],
                    s.gamma[g_at + k], sk, pi, pr);
    Pr[r] = pr; Pi[r] = pi;
    dmp_sched_store3(s.out + (size_t)t * a.n * 3, k, sk, pi, pr);
}

__global__ __launch_bounds__(256) void k_dmp_sched_edge(const int* __restrict__ src, const int* __restrict__ rev,
                                                       const float* __restrict__ P, const float* __restrict__ theta, DmpSchedArgs a,
                                                       unsigned per, long w_at, long w_next_at, long g_at, float* __restrict__ phi,
                                                       float* __restrict__ ps, float* __restrict__ theta_next) {
    const size_t b = blockIdx.x / per;
    const long e = (long)(blockIdx.x % per) * 256 + threadIdx.x;
    if (e >= a.nnz) return;
    const DmpSchedSample s = dmp_sched_sample(a, b);
    const size_t base = b * (size_t)a.nnz, slot = base + e;
    const int u = src[e];
    dmp_edge_update(P[b * (size_t)a.n + u], theta[base + rev[e]], s.s0[(size_t)u * 3], s.w[w_at + e], s.w[w_next_at + e], s.gamma[g_at + u],
                    phi[slot], ps[slot], theta[slot], theta_next[slot]);
}

int gn_dmp_schedule_set_attributes() {       // once per device, from gnode_graph_create
    GN_HIP(hipFuncSetAttribute((const void*)k_dmp_sched_wg, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDmpLdsLimit));
    return 0;
}

// ------------------------------------------------------------------------------------------------ the host side
// The workspace: the device copy of the phase table, then for the general form theta x2, phi, ps over B * nnz edge slots and
// P, Pr, Pi over B * n rows.  With `base` null only `bytes` means anything.
struct DmpSchedWorkspace {
    int32_t* phase;
    float *theta[2], *phi, *ps, *P, *Pr, *Pi;
    size_t bytes;
};
static DmpSchedWorkspace dmp_sched_carve(gnode_graph_t g, size_t B, size_t maxTime, bool general, void* base) {
    const size_t edges = (size_t)std::max<int64_t>(g->nnz, 1);
    const size_t EB = general ? gn_align(B * edges * 4) : 0, NB = general ? gn_align(B * (size_t)g->info.n * 4) : 0;
    size_t at = 0;
    auto take = [&](size_t bytes) { char* p = base ? (char*)base + at : nullptr; at += bytes; return (float*)p; };
    DmpSchedWorkspace w;
    w.phase = (int32_t*)take(gn_align(maxTime * sizeof(int32_t)));
    w.theta[0] = take(EB); w.theta[1] = take(EB); w.phi = take(EB); w.ps = take(EB);
    w.P = take(NB); w.Pr = take(NB); w.Pi = take(NB);
    w.bytes = at;
    return w;
}
extern "C" size_t gnode_dmp_batch_schedule_workspace_bytes(gnode_graph_t g, int32_t B, int32_t maxTime) {
    return g && B >= 1 && maxTime >= 2 ? dmp_sched_carve(g, (size_t)B, (size_t)maxTime, !dmp_sched_one_workgroup(g), nullptr).bytes : 0;
}

extern "C" int gnode_dmp_batch_schedule_f32(gnode_graph_t g, const float* weights, int64_t w_stride, const float* gamma, int64_t gamma_stride,
                                            const int32_t* phase_host, int32_t P, const float* init, int32_t B, int32_t maxTime, float* out,
                                            void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "gnode_dmp_batch_schedule_f32";
    GN_CHECK_ARG(g && gamma && init && out && workspace && phase_host, "%s: null pointer", who);
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
    const unsigned ng = (unsigned)((n + 255) / 256), eg = (unsigned)std::max<long>(1, (nnz + 255) / 256);
    const bool one_wg = dmp_sched_one_workgroup(g);
    const unsigned threads = (unsigned)std::min<long>(1024, std::max<long>(64, (std::max<long>(n, nnz) + 63) / 64 * 64));
    GN_CHECK_ARG(one_wg || (size_t)B * std::max(ng, eg) < ((size_t)1 << 31), "%s: B = %d is too many samples for this graph", who, B);
    const size_t bytes = dmp_sched_carve(g, (size_t)B, (size_t)maxTime, !one_wg, nullptr).bytes;
    if (workspace_bytes < bytes) {
        gnode_set_error("%s: workspace %zu < %zu", who, workspace_bytes, bytes);
        return GNODE_ERR_WORKSPACE;
    }
    GN_CHECK_ARG(g->symmetric, "%s: the sparsity pattern is not symmetric (DMP here serves undirected graphs)", who);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = dmp_check_rate_tables(who, "weights", weights, w_stride ? (size_t)B : 1, (size_t)P, (size_t)nnz, st)) return rc;
    if (int rc = dmp_check_rate_tables(who, "gamma", gamma, gamma_stride ? (size_t)B : 1, (size_t)P, (size_t)n, st)) return rc;
    const DmpSchedWorkspace ws = dmp_sched_carve(g, (size_t)B, (size_t)maxTime, !one_wg, workspace);
    // entry 0 is never read; it travels as 0 so that the device copy holds no number out of range
    GN_HIP(hipMemsetAsync(ws.phase, 0, sizeof(int32_t), st));
    GN_HIP(hipMemcpyAsync(ws.phase + 1, phase_host + 1, sizeof(int32_t) * (size_t)(maxTime - 1), hipMemcpyHostToDevice, st));
    GN_HIP(hipStreamSynchronize(st));          // phase_host is done with
    const DmpSchedArgs a = {weights, (long)w_stride, gamma, (long)gamma_stride, init, out, ws.phase, n, maxTime, nnz};
    if (one_wg) {
        hipLaunchKernelGGL(k_dmp_sched_wg, dim3((unsigned)B), dim3(threads), gnode_dmp_batch_lds_bytes(g), st, g->rowptr, g->src, g->rev, a);
        GN_LAUNCH_CHECK();
        GN_HIP(hipStreamSynchronize(st));
        return 0;
    }
    const dim3 gn((unsigned)B * ng), ge((unsigned)B * eg);
    auto w_at = [&](int t) { return (long)phase_host[t] * nnz; };
    auto g_at = [&](int t) { return (long)phase_host[t] * n; };
    hipLaunchKernelGGL(k_dmp_sched_out0, gn, dim3(256), 0, st, a, ng);
    hipLaunchKernelGGL(k_dmp_sched_init, ge, dim3(256), 0, st, g->src, a, eg, w_at(1), ws.theta[0], ws.phi, ws.ps);
    GN_LAUNCH_CHECK();
    for (int t = 1; t < maxTime; ++t) {
        const int cur = (t - 1) & 1;
        hipLaunchKernelGGL(k_dmp_sched_node, gn, dim3(256), 0, st, g->rowptr, g->rev, ws.theta[cur], a, ng, t, g_at(t), ws.P, ws.Pr, ws.Pi);
        if (t + 1 < maxTime)                 // (the last step's messages have no reader)
            hipLaunchKernelGGL(k_dmp_sched_edge, ge, dim3(256), 0, st, g->src, g->rev, ws.P, ws.theta[cur], a, eg, w_at(t), w_at(t + 1), g_at(t),
                               ws.phi, ws.ps, ws.theta[cur ^ 1]);
        GN_LAUNCH_CHECK();
    }
    GN_HIP(hipStreamSynchronize(st));
    return 0;
}
