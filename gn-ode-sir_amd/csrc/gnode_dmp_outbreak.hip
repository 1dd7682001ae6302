// Whom to immunise and where to seed (Lokhov, Saad 2017): the DMP recurrence of gnode_dmp.h from every candidate intervention on
// one outbreak, kept only as the expected size of each compartment over time -- gnode_dmp_outbreak_sizes_f32.
//
// C candidates on one graph.  Candidate c's sample is DMP from the shared base start init[n][3] = (pS, pI, pR) per node with
// the triple of node cand[c] replaced: action 0 (seed) makes it (0, 1, 0), action 1 (immunise) makes it (0, 0, 1).  The
// kernels synthesise that start wherever gnode_dmp.hip reads one: no [C][n][3] state exists, and an id outside the graph
// (-1 by convention) matches no node and gives the base start itself.  The weights [nnz] and gamma [n] are shared by the
// candidates.  The recurrence is called as gnode_dmp.hip calls it for an `init` start (Pr_0 from the triple, phi_0 = Pi_0), so
// the fp32 marginals are gnode_dmp_batch_f32's bit for bit -- but none goes to global memory: at every step
// t = 0 .. maxTime - 1 (row 0 is the start itself) the node pass, which holds Ps, Pi, Pr of node k in registers, forms
//   sizes[c][t][j] = sum_k (double)value[k] * (double)P^k_j(t),      j = 0 / 1 / 2 for S / I / R; value == null: 1 for every k
// (the product of two floats is exact in a double) in fp64, in a fixed order and without atomics, as gnode_dmp_source.hip does:
// a thread sums its own nodes in ascending k, a wave adds its 64 lanes in a fixed tree, and the waves' sums are added in
// ascending wave order; in the general form one partial per block of 256 goes to the workspace at [c][t][j][block], and a last
// kernel adds a row's partials in ascending block order.  Two forms, chosen from the graph alone like gnode_dmp_batch_f32's:
//   one workgroup per candidate   the messages and marginals of the sample live in LDS for the whole horizon: one launch
//   general                       rows c * n + k and edge slots c * nnz + e of the workspace: two launches per time step,
//                                 one for row 0 and the messages' start each, and the final add
// A candidate's rows do not depend on C or on its position in the call: same expressions, same per-element order, and the
// reduction tree is a function of the graph alone.
#include "gnode_dmp.h"
#include <algorithm>

struct DmpOutbreakArgs {
    const float* w; const float* gamma;         // [nnz], [n]
    const float* init;                          // [n][3], the base start
    const int32_t* cand;                        // [C]
    const float* value;                         // [n] or null
    int action;                                 // 0 seed, 1 immunise
    double* sizes;                              // [C][maxTime][3]
    int n, maxTime; long nnz;
};

// the start of node k in the sample of candidate `cand`: the base triple, or the action's where k is the candidate
__device__ __forceinline__ void dmp_outbreak_state(const DmpOutbreakArgs& a, int k, int cand, float& ps0, float& pi0, float& pr0) {
    const bool hit = k == cand;
    const float seeded = a.action == 0 ? 1.0f : 0.0f;
    ps0 = hit ? 0.0f : a.init[(size_t)k * 3];
    pi0 = hit ? seeded : a.init[(size_t)k * 3 + 1];
    pr0 = hit ? 1.0f - seeded : a.init[(size_t)k * 3 + 2];
}
// ... and its Ps_0 alone, which is all that the steps after the first read of it: 0 under either action
__device__ __forceinline__ float dmp_outbreak_ps0(const DmpOutbreakArgs& a, int k, int cand) {
    return k == cand ? 0.0f : a.init[(size_t)k * 3];
}

struct DmpSums { double s, i, r; };
__device__ __forceinline__ void dmp_outbreak_add(const DmpOutbreakArgs& a, int k, float ps, float pi, float pr, DmpSums& acc) {
    const double v = a.value ? (double)a.value[k] : 1.0;
    acc.s = acc.s + v * (double)ps;
    acc.i = acc.i + v * (double)pi;
    acc.r = acc.r + v * (double)pr;
}
// the waves' sums of one step: red[j * 16 + wave].  Every lane of the wave is active where this is called.
__device__ __forceinline__ void dmp_outbreak_wave_sums(DmpSums acc, int lane, int wave, double* red) {
    const double s = dmp_wave_sum(acc.s), i = dmp_wave_sum(acc.i), r = dmp_wave_sum(acc.r);
    if (lane == 0) { red[wave] = s; red[16 + wave] = i; red[32 + wave] = r; }
}

static constexpr size_t kDmpOutbreakRedBytes = 2 * 3 * 16 * sizeof(double);     // the waves' three sums of a step, two steps' worth

extern "C" size_t gnode_dmp_outbreak_lds_bytes(gnode_graph_t g) {
    return g ? gnode_dmp_batch_lds_bytes(g) + kDmpOutbreakRedBytes : 0;          // the forward's arrays | the fp64 reduction scratch
}
static bool dmp_outbreak_one_workgroup(gnode_graph_t g) { return gnode_dmp_outbreak_lds_bytes(g) <= kDmpLdsLimit; }

// One workgroup = one candidate, every step: k_dmp_batch_wg with the start synthesised and the output rows replaced by their
// sums.  Thread `tid` owns nodes and edges tid, tid + blockDim.x, ... in both passes; blockDim.x is a multiple of 64 and at
// most 1024 (16 waves).  The barriers sit in uniform control flow (the step loop's bounds are kernel arguments), so every
// thread reaches each of them.  Step t's wave sums go to half t & 1 of `red`: threads 0, 1, 2 add one compartment's each after
// the barrier that follows the node pass while the other waves go on, and the same half is next written two barriers later.
__global__ __launch_bounds__(1024) void k_dmp_outbreak_wg(const int* __restrict__ rowptr, const int* __restrict__ src,
                                                         const int* __restrict__ rev_g, DmpOutbreakArgs a) {
    extern __shared__ __attribute__((aligned(16))) char dmp_smem[];
    const int n = a.n, nnz = (int)a.nnz, tid = threadIdx.x, nt = blockDim.x, wave = tid >> 6, lane = tid & 63, waves = nt >> 6;
    const size_t eb = dmp_align16((size_t)nnz * 4), nb = dmp_align16((size_t)n * 4);
    float* theta[2] = {(float*)dmp_smem, (float*)(dmp_smem + eb)};
    float* phi = (float*)(dmp_smem + 2 * eb); float* ps = (float*)(dmp_smem + 3 * eb);
    int* rev = (int*)(dmp_smem + 4 * eb);
    float* P = (float*)(dmp_smem + 5 * eb); float* Pi = (float*)(dmp_smem + 5 * eb + nb); float* Pr = (float*)(dmp_smem + 5 * eb + 2 * nb);
    double* red = (double*)(dmp_smem + 5 * eb + 3 * nb);
    const int cand = a.cand[blockIdx.x];
    double* size = a.sizes + (size_t)blockIdx.x * a.maxTime * 3;
    DmpSums acc = {0.0, 0.0, 0.0};
    for (int k = tid; k < n; k += nt) {                                   // row 0; Pi, Pr hold the start for step 1
        float ps0, pi0, pr0;
        dmp_outbreak_state(a, k, cand, ps0, pi0, pr0);
        Pi[k] = pi0; Pr[k] = pr0;
        dmp_outbreak_add(a, k, ps0, pi0, pr0, acc);
    }
    dmp_outbreak_wave_sums(acc, lane, wave, red);
    for (int e = tid; e < nnz; e += nt) {
        float ps0, pi0, pr0;
        dmp_outbreak_state(a, src[e], cand, ps0, pi0, pr0);
        dmp_edge_start(ps0, pi0, a.w[e], theta[0][e], phi[e], ps[e]);
        rev[e] = rev_g[e];
    }
    __syncthreads();
    if (tid < 3) size[tid] = dmp_sum_in_order(red + tid * 16, waves);
    for (int t = 1; t < a.maxTime; ++t) {
        const float* th = theta[(t - 1) & 1];
        float* th_next = theta[t & 1];
        double* red_t = red + (t & 1) * 48;
        acc = {0.0, 0.0, 0.0};
        for (int k = tid; k < n; k += nt) {                               // node pass
            const float p = dmp_row_product(rev, th, rowptr[k], rowptr[k + 1]);
            P[k] = p;
            float sk, pi, pr;
            dmp_node_update(p, dmp_outbreak_ps0(a, k, cand), Pi[k], Pr[k], a.gamma[k], sk, pi, pr);
            Pr[k] = pr; Pi[k] = pi;
            dmp_outbreak_add(a, k, sk, pi, pr, acc);
        }
        dmp_outbreak_wave_sums(acc, lane, wave, red_t);
        __syncthreads();                                                  // P and the wave sums are complete; theta[cur] is still this step's
        if (tid < 3) size[(size_t)t * 3 + tid] = dmp_sum_in_order(red_t + tid * 16, waves);
        if (t + 1 < a.maxTime)                                            // (the last step's messages have no reader)
            for (int e = tid; e < nnz; e += nt) {                         // edge pass
                const int u = src[e];
                dmp_edge_update(P[u], th[rev[e]], dmp_outbreak_ps0(a, u, cand), a.w[e], a.gamma[u], phi[e], ps[e], th[e], th_next[e]);
            }
        __syncthreads();                                                  // theta[next] is complete before its node pass
    }
}

// The general form: `per` blocks of 256 per candidate, candidate c = blockIdx.x / per.  Per-candidate state is at row c * n + k
// and edge slot c * nnz + e of the workspace arrays.
__global__ __launch_bounds__(256) void k_dmp_outbreak_init(const int* __restrict__ src, DmpOutbreakArgs a, unsigned per,
                                                          float* __restrict__ theta, float* __restrict__ phi, float* __restrict__ ps) {
    const size_t c = blockIdx.x / per;
    const long e = (long)(blockIdx.x % per) * 256 + threadIdx.x;
    if (e >= a.nnz) return;
    const size_t slot = c * (size_t)a.nnz + e;
    float ps0, pi0, pr0;
    dmp_outbreak_state(a, src[e], a.cand[c], ps0, pi0, pr0);
    dmp_edge_start(ps0, pi0, a.w[e], theta[slot], phi[slot], ps[slot]);
}

// Step t of every candidate's nodes and the block's partials of sizes[c][t][.]; t = 0 is the start itself (theta is not read).
// No thread leaves before the barrier: one past the last node contributes 0.
__global__ __launch_bounds__(256) void k_dmp_outbreak_node(const int* __restrict__ rowptr, const int* __restrict__ rev,
                                                          const float* __restrict__ theta, DmpOutbreakArgs a, unsigned per, int t,
                                                          float* __restrict__ P, float* __restrict__ Pr, float* __restrict__ Pi,
                                                          double* __restrict__ partial) {
    __shared__ double red[48];
    const size_t c = blockIdx.x / per;
    const unsigned blk = blockIdx.x % per;
    const int k = (int)blk * 256 + threadIdx.x;
    DmpSums acc = {0.0, 0.0, 0.0};
    if (k < a.n) {
        float ps0, pi0, pr0, sk, pi, pr;
        dmp_outbreak_state(a, k, a.cand[c], ps0, pi0, pr0);
        if (t == 0) {
            sk = ps0; pi = pi0; pr = pr0;
        } else {
            const size_t r = c * (size_t)a.n + k;
            const float p = dmp_row_product(rev, theta + c * (size_t)a.nnz, rowptr[k], rowptr[k + 1]);
            P[r] = p;                                                     // step 1 starts from the state itself
            dmp_node_update(p, ps0, t == 1 ? pi0 : Pi[r], t == 1 ? pr0 : Pr[r], a.gamma[k], sk, pi, pr);
            Pr[r] = pr; Pi[r] = pi;
        }
        dmp_outbreak_add(a, k, sk, pi, pr, acc);
    }
    dmp_outbreak_wave_sums(acc, threadIdx.x & 63, threadIdx.x >> 6, red);
    __syncthreads();
    if (threadIdx.x < 3)
        partial[((c * (size_t)a.maxTime + t) * 3 + threadIdx.x) * per + blk] = dmp_sum_in_order(red + threadIdx.x * 16, 4);
}

__global__ __launch_bounds__(256) void k_dmp_outbreak_edge(const int* __restrict__ src, const int* __restrict__ rev,
                                                          const float* __restrict__ P, const float* __restrict__ theta, DmpOutbreakArgs a,
                                                          unsigned per, float* __restrict__ phi, float* __restrict__ ps,
                                                          float* __restrict__ theta_next) {
    const size_t c = blockIdx.x / per;
    const long e = (long)(blockIdx.x % per) * 256 + threadIdx.x;
    if (e >= a.nnz) return;
    const size_t base = c * (size_t)a.nnz, slot = base + e;
    const int u = src[e];
    dmp_edge_update(P[c * (size_t)a.n + u], theta[base + rev[e]], dmp_outbreak_ps0(a, u, a.cand[c]), a.w[e], a.gamma[u], phi[slot], ps[slot],
                    theta[slot], theta_next[slot]);
}

// sizes[i] = the `per` partials of row i = (c * maxTime + t) * 3 + j, in ascending block order
__global__ __launch_bounds__(256) void k_dmp_outbreak_add(const double* __restrict__ partial, unsigned per, size_t rows,
                                                         double* __restrict__ sizes) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < rows; i += (size_t)gridDim.x * 256)
        sizes[i] = dmp_sum_in_order(partial + i * per, (int)per);
}

int gn_dmp_outbreak_set_attributes() {      // once per device, from gnode_graph_create
    GN_HIP(hipFuncSetAttribute((const void*)k_dmp_outbreak_wg, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDmpLdsLimit));
    return 0;
}

// ------------------------------------------------------------------------------------------------ the host side
// The workspace of a call.  The one-workgroup form keeps everything in LDS and uses none of it: one aligned unit, so that the
// query is not 0 for a call that is served.  The general form: theta x2, phi, ps over C * nnz edge slots, P, Pr, Pi over C * n
// rows, the partials [C][maxTime][3][blocks per candidate] in fp64.  With `base` null only `bytes` means anything.
struct DmpOutbreakWorkspace {
    float *theta[2], *phi, *ps, *P, *Pr, *Pi;
    double* partial;
    size_t bytes;
};
static DmpOutbreakWorkspace dmp_outbreak_carve(gnode_graph_t g, size_t C, size_t maxTime, bool general, void* base) {
    const size_t edges = (size_t)std::max<int64_t>(g->nnz, 1), n = (size_t)g->info.n, ng = (n + 255) / 256;
    const size_t EB = general ? gn_align(C * edges * 4) : 0, NB = general ? gn_align(C * n * 4) : 0;
    size_t at = 0;
    auto take = [&](size_t bytes) { char* p = base ? (char*)base + at : nullptr; at += bytes; return p; };
    DmpOutbreakWorkspace w;
    w.theta[0] = (float*)take(EB); w.theta[1] = (float*)take(EB); w.phi = (float*)take(EB); w.ps = (float*)take(EB);
    w.P = (float*)take(NB); w.Pr = (float*)take(NB); w.Pi = (float*)take(NB);
    w.partial = (double*)take(general ? gn_align(C * maxTime * 3 * ng * 8) : 256);
    w.bytes = at;
    return w;
}
extern "C" size_t gnode_dmp_outbreak_workspace_bytes(gnode_graph_t g, int32_t C, int32_t maxTime) {
    return g && C >= 1 && maxTime >= 2 ? dmp_outbreak_carve(g, (size_t)C, (size_t)maxTime, !dmp_outbreak_one_workgroup(g), nullptr).bytes : 0;
}

// What the call settles before it writes anything, in gnode_dmp_source_scores_f32's order: its arguments, the form and its
// launch shape, the workspace's size, the pattern's symmetry.  Nothing here waits on the host: the call only enqueues work.
extern "C" int gnode_dmp_outbreak_sizes_f32(gnode_graph_t g, const float* weights, const float* gamma, const float* init,
                                            const int32_t* candidates, int32_t C, int32_t action, const float* value, int32_t maxTime,
                                            double* sizes, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "gnode_dmp_outbreak_sizes_f32";
    GN_CHECK_ARG(g && gamma && init && candidates && sizes && workspace, "%s: null pointer", who);
    GN_CHECK_ARG(weights || g->nnz == 0, "%s: weights is null", who);          // no edge, no weight: an empty tensor has no address
    GN_CHECK_ARG(maxTime >= 2, "%s: maxTime must be >= 2 (got %d)", who, maxTime);
    GN_CHECK_ARG(C >= 1, "%s: C must be >= 1 (got %d)", who, C);
    GN_CHECK_ARG(action == 0 || action == 1, "%s: action must be 0 (seed) or 1 (immunise) (got %d)", who, action);
    const int n = g->info.n;
    const long nnz = g->nnz;
    const unsigned ng = (unsigned)((n + 255) / 256), eg = (unsigned)std::max<long>(1, (nnz + 255) / 256);
    const bool one_wg = dmp_outbreak_one_workgroup(g);
    const unsigned threads = (unsigned)std::min<long>(1024, std::max<long>(64, (std::max<long>(n, nnz) + 63) / 64 * 64));
    GN_CHECK_ARG(one_wg || (size_t)C * std::max(ng, eg) < ((size_t)1 << 31), "%s: C = %d is too many candidates for this graph", who, C);
    const size_t bytes = dmp_outbreak_carve(g, (size_t)C, (size_t)maxTime, !one_wg, nullptr).bytes;
    if (workspace_bytes < bytes) {
        gnode_set_error("%s: workspace %zu < %zu", who, workspace_bytes, bytes);
        return GNODE_ERR_WORKSPACE;
    }
    GN_CHECK_ARG(g->symmetric, "%s: the sparsity pattern is not symmetric (DMP here serves undirected graphs)", who);
    const DmpOutbreakWorkspace ws = dmp_outbreak_carve(g, (size_t)C, (size_t)maxTime, !one_wg, workspace);
    hipStream_t st = (hipStream_t)stream;
    const DmpOutbreakArgs a = {weights, gamma, init, candidates, value, action, sizes, n, maxTime, nnz};
    if (one_wg) {
        hipLaunchKernelGGL(k_dmp_outbreak_wg, dim3((unsigned)C), dim3(threads), gnode_dmp_outbreak_lds_bytes(g), st, g->rowptr, g->src, g->rev, a);
        GN_LAUNCH_CHECK();
        return 0;
    }
    const dim3 gn((unsigned)C * ng), ge((unsigned)C * eg);
    hipLaunchKernelGGL(k_dmp_outbreak_node, gn, dim3(256), 0, st, g->rowptr, g->rev, ws.theta[0], a, ng, 0, ws.P, ws.Pr, ws.Pi, ws.partial);
    hipLaunchKernelGGL(k_dmp_outbreak_init, ge, dim3(256), 0, st, g->src, a, eg, ws.theta[0], ws.phi, ws.ps);
    GN_LAUNCH_CHECK();
    for (int t = 1; t < maxTime; ++t) {
        const int cur = (t - 1) & 1;
        hipLaunchKernelGGL(k_dmp_outbreak_node, gn, dim3(256), 0, st, g->rowptr, g->rev, ws.theta[cur], a, ng, t, ws.P, ws.Pr, ws.Pi, ws.partial);
        if (t + 1 < maxTime)                 // (the last step's messages have no reader)
            hipLaunchKernelGGL(k_dmp_outbreak_edge, ge, dim3(256), 0, st, g->src, g->rev, ws.P, ws.theta[cur], a, eg, ws.phi, ws.ps, ws.theta[cur ^ 1]);
        GN_LAUNCH_CHECK();
    }
    const size_t rows = (size_t)C * maxTime * 3;
    hipLaunchKernelGGL(k_dmp_outbreak_add, dim3((unsigned)std::min<size_t>((rows + 255) / 256, 65536)), dim3(256), 0, st, ws.partial, ng, rows,
                       sizes);
    GN_LAUNCH_CHECK();
    return 0;
}
