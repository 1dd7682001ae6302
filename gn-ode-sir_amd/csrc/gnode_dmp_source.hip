// Source inference from one snapshot (Lokhov, Mezard, Ohta, Zdeborova 2014): the DMP recurrence of gnode_dmp.h from every
// candidate source, scored by the mean-field likelihood of the observed states -- gnode_dmp_source_scores_f32.
//
// C candidates on one graph.  Candidate c's sample is DMP from the one-hot seed state (1 - [k == cand_c], [k == cand_c], 0),
// which the kernels synthesise from the candidate id wherever gnode_dmp.hip reads a start: no [C][n][3] state exists, and an id
// outside the graph matches no node.  The weights [nnz] and gamma [n] are shared by the candidates.  No marginal goes to
// global memory: at every step t = 0 .. maxTime - 1 (row 0 is the start itself) the node pass, which holds Ps, Pi, Pr of node k
// in registers, forms for obs[k] in {0, 1, 2}
//   log((double)min(max(p, floor), 1.0f)),      p = Ps / Pi / Pr by obs[k]
// and any other obs[k] contributes nothing (so no device value indexes anything).  The clamp is fp32: Pi = 1 - Ps - Pr can
// round below 0, Ps can exceed 1 by the 1e-10 offset, and a node outside the t-ball of the candidate has probability exactly 0.
//   scores[c][t] = sum_k term_k       in fp64, in a fixed order and without atomics:
// a thread sums its own nodes in ascending k, a wave adds its 64 lanes in a fixed tree, and the waves' sums are added in
// ascending wave order; in the general form one partial per block of 256 goes to the workspace at [c][t][block], and a last
// kernel adds a row's partials in ascending block order.  Two forms, chosen from the graph alone like gnode_dmp_batch_f32's:
//   one workgroup per candidate   the messages and marginals of the sample live in LDS for the whole horizon: one launch
//   general                       rows c * n + k and edge slots c * nnz + e of the workspace: two launches per time step,
//                                 one for row 0 and the messages' start each, and the final add
// A candidate's row does not depend on C or on its position in the call: same expressions, same per-element order, and the
// reduction tree is a function of the graph alone.
#include "gnode_dmp.h"
#include <algorithm>

struct DmpSourceArgs {
    const float* w; const float* gamma;         // [nnz], [n]
    const int32_t* cand;                        // [C]
    const int32_t* obs;                         // [n]
    float floor;
    double* scores;                             // [C][maxTime]
    int n, maxTime; long nnz;
};

// (dmp_source_state and dmp_source_term, which gnode_dmp_source_batch.hip shares, are in gnode_dmp.h)
static constexpr size_t kDmpSourceRedBytes = 2 * 16 * sizeof(double);       // the waves' sums of a step, two steps' worth

extern "C" size_t gnode_dmp_source_lds_bytes(gnode_graph_t g) {
    return g ? gnode_dmp_batch_lds_bytes(g) + kDmpSourceRedBytes : 0;         // the forward's arrays | the fp64 reduction scratch
}
static bool dmp_source_one_workgroup(gnode_graph_t g) { return gnode_dmp_source_lds_bytes(g) <= kDmpLdsLimit; }

// One workgroup = one candidate, every step: k_dmp_batch_wg with the start synthesised and the output rows replaced by their
// scores.  Thread `tid` owns nodes and edges tid, tid + blockDim.x, ... in both passes; blockDim.x is a multiple of 64.  The
// barriers sit in uniform control flow (the step loop's bounds are kernel arguments), so every thread reaches each of them.
// Step t's wave sums go to red[t & 1]: thread 0 adds them after the barrier that follows the node pass while the other waves
// go on, and the same half is next written two barriers later.
__global__ __launch_bounds__(1024) void k_dmp_source_wg(const int* __restrict__ rowptr, const int* __restrict__ src,
                                                       const int* __restrict__ rev_g, DmpSourceArgs a) {
    extern __shared__ __attribute__((aligned(16))) char dmp_smem[];
    const int n = a.n, nnz = (int)a.nnz, tid = threadIdx.x, nt = blockDim.x, wave = tid >> 6, lane = tid & 63, waves = nt >> 6;
    const size_t eb = dmp_align16((size_t)nnz * 4), nb = dmp_align16((size_t)n * 4);
    float* theta[2] = {(float*)dmp_smem, (float*)(dmp_smem + eb)};
    float* phi = (float*)(dmp_smem + 2 * eb); float* ps = (float*)(dmp_smem + 3 * eb);
    int* rev = (int*)(dmp_smem + 4 * eb);
    float* P = (float*)(dmp_smem + 5 * eb); float* Pi = (float*)(dmp_smem + 5 * eb + nb); float* Pr = (float*)(dmp_smem + 5 * eb + 2 * nb);
    double* red = (double*)(dmp_smem + 5 * eb + 3 * nb);
    const int cand = a.cand[blockIdx.x];
    double* score = a.scores + (size_t)blockIdx.x * a.maxTime;
    double acc = 0.0;
    for (int k = tid; k < n; k += nt) {                                   // row 0; Pi, Pr hold the start for step 1
        float ps0, pi0;
        dmp_source_state(k, cand, ps0, pi0);
        Pi[k] = pi0; Pr[k] = 0.0f;
        acc = acc + dmp_source_term(a.obs[k], ps0, pi0, 0.0f, a.floor);
    }
    acc = dmp_wave_sum(acc);
    if (lane == 0) red[wave] = acc;
    for (int e = tid; e < nnz; e += nt) {
        float ps0, pi0;
        dmp_source_state(src[e], cand, ps0, pi0);
        dmp_edge_start(ps0, pi0, a.w[e], theta[0][e], phi[e], ps[e]);
        rev[e] = rev_g[e];
    }
    __syncthreads();
    if (tid == 0) score[0] = dmp_sum_in_order(red, waves);
    for (int t = 1; t < a.maxTime; ++t) {
        const float* th = theta[(t - 1) & 1];
        float* th_next = theta[t & 1];
        double* red_t = red + (t & 1) * 16;
        acc = 0.0;
        for (int k = tid; k < n; k += nt) {                               // node pass
            const float p = dmp_row_product(rev, th, rowptr[k], rowptr[k + 1]);
            P[k] = p;
            float ps0, pi0, sk, pi, pr;
            dmp_source_state(k, cand, ps0, pi0);
            dmp_node_update(p, ps0, Pi[k], Pr[k], a.gamma[k], sk, pi, pr);
            Pr[k] = pr; Pi[k] = pi;
            acc = acc + dmp_source_term(a.obs[k], sk, pi, pr, a.floor);
        }
        acc = dmp_wave_sum(acc);
        if (lane == 0) red_t[wave] = acc;
        __syncthreads();                                                  // P and the wave sums are complete; theta[cur] is still this step's
        if (tid == 0) score[t] = dmp_sum_in_order(red_t, waves);
        if (t + 1 < a.maxTime)                                            // (the last step's messages have no reader)
            for (int e = tid; e < nnz; e += nt) {                         // edge pass
                const int u = src[e];
                float ps0, pi0;
                dmp_source_state(u, cand, ps0, pi0);
                dmp_edge_update(P[u], th[rev[e]], ps0, a.w[e], a.gamma[u], phi[e], ps[e], th[e], th_next[e]);
            }
        __syncthreads();                                                  // theta[next] is complete before its node pass
    }
}

// The general form: `per` blocks of 256 per candidate, candidate c = blockIdx.x / per.  Per-candidate state is at row c * n + k
// and edge slot c * nnz + e of the workspace arrays.  The messages' start and the edge pass, which read no observation, are
// k_dmp_source_init and k_dmp_source_edge of gnode_dmp.h, shared with gnode_dmp_source_batch.hip.
//
// Step t of every candidate's nodes and the block's partial of scores[c][t]; t = 0 is the start itself (theta is not read).  No
// thread leaves before the barrier: one past the last node contributes 0.
__global__ __launch_bounds__(256) void k_dmp_source_node(const int* __restrict__ rowptr, const int* __restrict__ rev,
                                                        const float* __restrict__ theta, DmpSourceArgs a, unsigned per, int t,
                                                        float* __restrict__ P, float* __restrict__ Pr, float* __restrict__ Pi,
                                                        double* __restrict__ partial) {
    __shared__ double red[4];
    const size_t c = blockIdx.x / per;
    const unsigned blk = blockIdx.x % per;
    const int k = (int)blk * 256 + threadIdx.x;
    double term = 0.0;
    if (k < a.n) {
        float ps0, pi0, sk, pi, pr;
        dmp_source_state(k, a.cand[c], ps0, pi0);
        if (t == 0) {
            sk = ps0; pi = pi0; pr = 0.0f;
        } else {
            const size_t r = c * (size_t)a.n + k;
            const float p = dmp_row_product(rev, theta + c * (size_t)a.nnz, rowptr[k], rowptr[k + 1]);
            P[r] = p;                                                     // step 1 starts from the state itself
            dmp_node_update(p, ps0, t == 1 ? pi0 : Pi[r], t == 1 ? 0.0f : Pr[r], a.gamma[k], sk, pi, pr);
            Pr[r] = pr; Pi[r] = pi;
        }
        term = dmp_source_term(a.obs[k], sk, pi, pr, a.floor);
    }
    term = dmp_wave_sum(term);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = term;
    __syncthreads();
    if (threadIdx.x == 0) partial[(c * (size_t)a.maxTime + t) * per + blk] = dmp_sum_in_order(red, 4);
}

// scores[i] = the `per` partials of row i = c * maxTime + t, in ascending block order
__global__ __launch_bounds__(256) void k_dmp_source_add(const double* __restrict__ partial, unsigned per, size_t rows,
                                                       double* __restrict__ scores) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < rows; i += (size_t)gridDim.x * 256)
        scores[i] = dmp_sum_in_order(partial + i * per, (int)per);
}

int gn_dmp_source_set_attributes() {        // once per device, from gnode_graph_create
    GN_HIP(hipFuncSetAttribute((const void*)k_dmp_source_wg, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDmpLdsLimit));
    return 0;
}

// ------------------------------------------------------------------------------------------------ the host side
// The workspace of a call.  The one-workgroup form keeps everything in LDS and uses none of it: one aligned unit, so that the
// query is not 0 for a call that is served.  The general form: theta x2, phi, ps over C * nnz edge slots, P, Pr, Pi over C * n
// rows, the partials [C][maxTime][blocks per candidate] in fp64.  With `base` null only `bytes` means anything.
struct DmpSourceWorkspace {
    float *theta[2], *phi, *ps, *P, *Pr, *Pi;
    double* partial;
    size_t bytes;
};
static DmpSourceWorkspace dmp_source_carve(gnode_graph_t g, size_t C, size_t maxTime, bool general, void* base) {
    const size_t edges = (size_t)std::max<int64_t>(g->nnz, 1), n = (size_t)g->info.n, ng = (n + 255) / 256;
    const size_t EB = general ? gn_align(C * edges * 4) : 0, NB = general ? gn_align(C * n * 4) : 0;
    size_t at = 0;
    auto take = [&](size_t bytes) { char* p = base ? (char*)base + at : nullptr; at += bytes; return p; };
    DmpSourceWorkspace w;
    w.theta[0] = (float*)take(EB); w.theta[1] = (float*)take(EB); w.phi = (float*)take(EB); w.ps = (float*)take(EB);
    w.P = (float*)take(NB); w.Pr = (float*)take(NB); w.Pi = (float*)take(NB);
    w.partial = (double*)take(general ? gn_align(C * maxTime * ng * 8) : 256);
    w.bytes = at;
    return w;
}
extern "C" size_t gnode_dmp_source_workspace_bytes(gnode_graph_t g, int32_t C, int32_t maxTime) {
    return g && C >= 1 && maxTime >= 2 ? dmp_source_carve(g, (size_t)C, (size_t)maxTime, !dmp_source_one_workgroup(g), nullptr).bytes : 0;
}

// What the call settles before it writes anything, in dmp_preamble's order (gnode_dmp.hip): its arguments, the form and its
// launch shape, the workspace's size, the pattern's symmetry.
extern "C" int gnode_dmp_source_scores_f32(gnode_graph_t g, const float* weights, const float* gamma, const int32_t* candidates, int32_t C,
                                           const int32_t* obs, float floor, int32_t maxTime, double* scores, void* workspace,
                                           size_t workspace_bytes, void* stream) {
    const char* who = "gnode_dmp_source_scores_f32";
    GN_CHECK_ARG(g && gamma && candidates && obs && scores && workspace, "%s: null pointer", who);
    GN_CHECK_ARG(weights || g->nnz == 0, "%s: weights is null", who);          // no edge, no weight: an empty tensor has no address
    GN_CHECK_ARG(maxTime >= 2, "%s: maxTime must be >= 2 (got %d)", who, maxTime);
    GN_CHECK_ARG(C >= 1, "%s: C must be >= 1 (got %d)", who, C);
    GN_CHECK_ARG(floor > 0.0f && floor <= 1.0f, "%s: floor must be in (0, 1] (got %g)", who, (double)floor);      // (a NaN fails it)
    const int n = g->info.n;
    const long nnz = g->nnz;
    const unsigned ng = (unsigned)((n + 255) / 256), eg = (unsigned)std::max<long>(1, (nnz + 255) / 256);
    const bool one_wg = dmp_source_one_workgroup(g);
    const unsigned threads = (unsigned)std::min<long>(1024, std::max<long>(64, (std::max<long>(n, nnz) + 63) / 64 * 64));
    GN_CHECK_ARG(one_wg || (size_t)C * std::max(ng, eg) < ((size_t)1 << 31), "%s: C = %d is too many candidates for this graph", who, C);
    const size_t bytes = dmp_source_carve(g, (size_t)C, (size_t)maxTime, !one_wg, nullptr).bytes;
    if (workspace_bytes < bytes) {
        gnode_set_error("%s: workspace %zu < %zu", who, workspace_bytes, bytes);
        return GNODE_ERR_WORKSPACE;
    }
    GN_CHECK_ARG(g->symmetric, "%s: the sparsity pattern is not symmetric (DMP here serves undirected graphs)", who);
    const DmpSourceWorkspace ws = dmp_source_carve(g, (size_t)C, (size_t)maxTime, !one_wg, workspace);
    hipStream_t st = (hipStream_t)stream;
    GN_HIP(hipStreamSynchronize(st));          // nothing waits on the host here: only the documented contract (include/gnode.h) keeps it
    const DmpSourceArgs a = {weights, gamma, candidates, obs, floor, scores, n, maxTime, nnz};
    if (one_wg) {
        hipLaunchKernelGGL(k_dmp_source_wg, dim3((unsigned)C), dim3(threads), gnode_dmp_source_lds_bytes(g), st, g->rowptr, g->src, g->rev, a);
        GN_LAUNCH_CHECK();
        return 0;
    }
    const dim3 gn((unsigned)C * ng), ge((unsigned)C * eg);
    hipLaunchKernelGGL(k_dmp_source_node, gn, dim3(256), 0, st, g->rowptr, g->rev, ws.theta[0], a, ng, 0, ws.P, ws.Pr, ws.Pi, ws.partial);
    hipLaunchKernelGGL(k_dmp_source_init<DmpSourceArgs>, ge, dim3(256), 0, st, g->src, a, eg, ws.theta[0], ws.phi, ws.ps);
    GN_LAUNCH_CHECK();
    for (int t = 1; t < maxTime; ++t) {
        const int cur = (t - 1) & 1;
        hipLaunchKernelGGL(k_dmp_source_node, gn, dim3(256), 0, st, g->rowptr, g->rev, ws.theta[cur], a, ng, t, ws.P, ws.Pr, ws.Pi, ws.partial);
        if (t + 1 < maxTime)                 // (the last step's messages have no reader)
            hipLaunchKernelGGL(k_dmp_source_edge<DmpSourceArgs>, ge, dim3(256), 0, st, g->src, g->rev, ws.P, ws.theta[cur], a, eg, ws.phi, ws.ps,
                               ws.theta[cur ^ 1]);
        GN_LAUNCH_CHECK();
    }
    const size_t rows = (size_t)C * maxTime;
    hipLaunchKernelGGL(k_dmp_source_add, dim3((unsigned)std::min<size_t>((rows + 255) / 256, 65536)), dim3(256), 0, st, ws.partial, ng, rows,
                       scores);
    GN_LAUNCH_CHECK();
    return 0;
}
