// Source inference from time-stamped evidence in one DMP pass -- gnode_dmp_source_events_scores_f32.
//
// gnode_dmp_source_batch.hip scores O snapshots: rows of STATES at one common step.  Outbreak data is events -- the step at which
// a node was infected, the step at which it recovered -- and DMP gives those too: node k becomes infected AT step t with
// probability Ps_k(t-1) - Ps_k(t) and recovers AT step t with probability Pr_k(t) - Pr_k(t-1).  The node pass holds both
// differences in registers: Pr(t-1) is the pr_prev its update reads, Ps(t-1) is ps0 * P_old[k] on the product it is about to
// overwrite (ps0 itself at t = 1, where no product exists yet), and before the start Ps(-1) = 1, Pr(-1) = 0.  So a row code may
// be 3 ("infected at this step") or 4 ("recovered at this step") next to 0 / 1 / 2; per node and step the FIVE possible terms
// are computed once (dmp_source_event_logs) and every row selects one of them, or 0.0 (dmp_source_event_pick).  The contract:
//   scores[r * score_stride + c * maxTime + t]; a row whose codes are all outside 3 / 4 is bit for bit
//   gnode_dmp_source_batch_scores_f32's row, and so gnode_dmp_source_scores_f32's table for that row alone.
// Everything that makes that so is that unit's: the form is chosen by the solo entry's predicate, the launch shapes are the solo
// entry's, the tile and the workspace are the batch entry's, and every row's sum is taken in the solo kernels' order (a thread
// adds its own nodes in ascending k, dmp_wave_sum adds the lanes, dmp_sum_in_order adds the waves and, in the general form, the
// per-block partials).  Nothing is atomic and no row value indexes anything.  The kernels are that unit's two with the previous
// step's Ps and Pr kept for the two differences; the start of the messages and the edge pass read no row (gnode_dmp.h).
#include "gnode_dmp.h"
#include <algorithm>

static constexpr int kDmpSourceEventsTile = 16;     // rows per workgroup / per barrier, as gnode_dmp_source_batch.hip: registers in DESIGN 4.11

struct DmpSourceEventsArgs {
    const float* w; const float* gamma;         // [nnz], [n]
    const int32_t* cand;                        // [C]
    const int8_t* rows;                         // [R][n]
    float floor;
    double* scores;                             // [r * stride + c * maxTime + t]
    long stride;
    int n, maxTime, R; long nnz;
};

static bool dmp_source_events_one_workgroup(gnode_graph_t g) { return gnode_dmp_source_lds_bytes(g) <= kDmpLdsLimit; }   // the solo entry's
static constexpr size_t kDmpSourceEventsRedBytes = 2 * 16 * sizeof(double);        // per row of a tile: the solo kernel's scratch
// the tile of the one-workgroup form on this graph: what the LDS left by the sample's arrays holds, at most the compiled one
static int dmp_source_events_wg_tile(gnode_graph_t g) {
    const size_t room = (kDmpLdsLimit - gnode_dmp_batch_lds_bytes(g)) / kDmpSourceEventsRedBytes;     // >= 1 in this form
    return (int)std::min<size_t>(room, (size_t)kDmpSourceEventsTile);
}
extern "C" int gnode_dmp_source_events_tile(gnode_graph_t g) {
    return !g ? 0 : dmp_source_events_one_workgroup(g) ? dmp_source_events_wg_tile(g) : kDmpSourceEventsTile;
}

// One workgroup = one candidate and `tile` <= W consecutive rows, every step: k_dmp_source_batch_wg with the five terms.  Block b
// serves candidate b / tiles and the rows from (b % tiles) * tile on, `wt` of them; acc[] is indexed by unrolled constants only,
// and the `w < wt` tests are uniform over the workgroup.  red holds [2][tile][16] doubles: step t's wave sums of row w at
// red[(t & 1) * tile * 16 + w * 16 + wave], read by thread w after the barrier that follows the node pass and next written two
// barriers later.  P[k] is read before it is written: it still holds step t - 1's product, and Pr[k] step t - 1's Pr.
template <int W>
__global__ __launch_bounds__(1024) void k_dmp_source_events_wg(const int* __restrict__ rowptr, const int* __restrict__ src,
                                                              const int* __restrict__ rev_g, DmpSourceEventsArgs a, int tile,
                                                              unsigned tiles) {
    extern __shared__ __attribute__((aligned(16))) char dmp_smem[];
    const int n = a.n, nnz = (int)a.nnz, tid = threadIdx.x, nt = blockDim.x, wave = tid >> 6, lane = tid & 63, waves = nt >> 6;
    const size_t eb = dmp_align16((size_t)nnz * 4), nb = dmp_align16((size_t)n * 4);
    float* theta[2] = {(float*)dmp_smem, (float*)(dmp_smem + eb)};
    float* phi = (float*)(dmp_smem + 2 * eb); float* ps = (float*)(dmp_smem + 3 * eb);
    int* rev = (int*)(dmp_smem + 4 * eb);
    float* P = (float*)(dmp_smem + 5 * eb); float* Pi = (float*)(dmp_smem + 5 * eb + nb); float* Pr = (float*)(dmp_smem + 5 * eb + 2 * nb);
    double* red = (double*)(dmp_smem + 5 * eb + 3 * nb);
    const unsigned c = blockIdx.x / tiles;
    const int r0 = (int)(blockIdx.x % tiles) * tile, wt = min(tile, a.R - r0);
    const int cand = a.cand[c];
    const int8_t* rows = a.rows + (size_t)r0 * n;                         // the tile's rows: rows[w * n + k], w < wt
    double* score = a.scores + (size_t)c * a.maxTime + (size_t)(r0 + tid) * a.stride;      // thread w < wt writes row r0 + w
    double acc[W];
#pragma unroll
    for (int w = 0; w < W; ++w) acc[w] = 0.0;
    for (int k = tid; k < n; k += nt) {                                   // row 0; Pi, Pr hold the start for step 1
        float ps0, pi0;
        dmp_source_state(k, cand, ps0, pi0);
        Pi[k] = pi0; Pr[k] = 0.0f;
        const DmpSourceEventLogs l = dmp_source_event_logs(ps0, pi0, 0.0f, 1.0f, 0.0f, a.floor);      // before the start: all susceptible
#pragma unroll
        for (int w = 0; w < W; ++w)
            if (w < wt) acc[w] = acc[w] + dmp_source_event_pick(rows[(size_t)w * n + k], l);
    }
#pragma unroll
    for (int w = 0; w < W; ++w)
        if (w < wt) {
            const double s = dmp_wave_sum(acc[w]);
            if (lane == 0) red[w * 16 + wave] = s;
        }
    for (int e = tid; e < nnz; e += nt) {
        float ps0, pi0;
        dmp_source_state(src[e], cand, ps0, pi0);
        dmp_edge_start(ps0, pi0, a.w[e], theta[0][e], phi[e], ps[e]);
        rev[e] = rev_g[e];
    }
    __syncthreads();
    if (tid < wt) score[0] = dmp_sum_in_order(red + tid * 16, waves);
    for (int t = 1; t < a.maxTime; ++t) {
        const float* th = theta[(t - 1) & 1];
        float* th_next = theta[t & 1];
        double* red_t = red + (size_t)(t & 1) * tile * 16;
#pragma unroll
        for (int w = 0; w < W; ++w) acc[w] = 0.0;
        for (int k = tid; k < n; k += nt) {                               // node pass
            const float p = dmp_row_product(rev, th, rowptr[k], rowptr[k + 1]);
            float ps0, pi0, sk, pi, pr;
            dmp_source_state(k, cand, ps0, pi0);
            const float ps_prev = t == 1 ? ps0 : ps0 * P[k], pr_prev = Pr[k];       // (no product exists before step 1)
            P[k] = p;
            dmp_node_update(p, ps0, Pi[k], pr_prev, a.gamma[k], sk, pi, pr);
            Pr[k] = pr; Pi[k] = pi;
            const DmpSourceEventLogs l = dmp_source_event_logs(sk, pi, pr, ps_prev, pr_prev, a.floor);
#pragma unroll
            for (int w = 0; w < W; ++w)
                if (w < wt) acc[w] = acc[w] + dmp_source_event_pick(rows[(size_t)w * n + k], l);
        }
#pragma unroll
        for (int w = 0; w < W; ++w)
            if (w < wt) {
                const double s = dmp_wave_sum(acc[w]);
                if (lane == 0) red_t[w * 16 + wave] = s;
            }
        __syncthreads();                                                  // P and the wave sums are complete; theta[cur] is still this step's
        if (tid < wt) score[t] = dmp_sum_in_order(red_t + tid * 16, waves);
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

// The general form: `per` blocks of 256 per candidate, candidate c = blockIdx.x / per; per-candidate state at row c * n + k and
// edge slot c * nnz + e of the workspace arrays.  Step t of every candidate's nodes, once, and the block's partial of
// scores[r][c][t] for EVERY row r; t = 0 is the start itself (theta, P, Pr, Pi are not read), and step 1 starts from the state,
// so the workspace is never read before it is written.  No thread leaves before the barriers: one past the last node
// contributes 0 to every sum.  The rows go in groups of G: group j's wave sums at red[j & 1], one barrier, then thread w < wt adds
// the four of row r0 + w; the same half is next written after the barrier of group j + 1, which those threads reach after reading.
template <int G>
__global__ __launch_bounds__(256) void k_dmp_source_events_node(const int* __restrict__ rowptr, const int* __restrict__ rev,
                                                               const float* __restrict__ theta, DmpSourceEventsArgs a, unsigned per, int t,
                                                               float* __restrict__ P, float* __restrict__ Pr, float* __restrict__ Pi,
                                                               double* __restrict__ partial) {
    __shared__ double red[2][G][4];
    const size_t c = blockIdx.x / per;
    const unsigned blk = blockIdx.x % per;
    const int tid = threadIdx.x, k = (int)blk * 256 + tid;
    const bool live = k < a.n;
    DmpSourceEventLogs l = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (live) {
        float ps0, pi0, sk, pi, pr, ps_prev, pr_prev;
        dmp_source_state(k, a.cand[c], ps0, pi0);
        if (t == 0) {
            sk = ps0; pi = pi0; pr = 0.0f;
            ps_prev = 1.0f; pr_prev = 0.0f;                               // before the start: all susceptible
        } else {
            const size_t r = c * (size_t)a.n + k;
            const float p = dmp_row_product(rev, theta + c * (size_t)a.nnz, rowptr[k], rowptr[k + 1]);
            ps_prev = t == 1 ? ps0 : ps0 * P[r];                          // step 1 starts from the state itself: no product yet
            pr_prev = t == 1 ? 0.0f : Pr[r];
            P[r] = p;
            dmp_node_update(p, ps0, t == 1 ? pi0 : Pi[r], pr_prev, a.gamma[k], sk, pi, pr);
            Pr[r] = pr; Pi[r] = pi;
        }
        l = dmp_source_event_logs(sk, pi, pr, ps_prev, pr_prev, a.floor);
    }
    double* out = partial + (c * (size_t)a.maxTime + t) * a.R * per + blk;           // row r at out[r * per]
    const int8_t* rows = a.rows + (live ? k : 0);                                     // row r at rows[r * n], where live
    for (int r0 = 0, j = 0; r0 < a.R; r0 += G, ++j) {
        const int wt = min(G, a.R - r0);
        double(*red_j)[4] = red[j & 1];
        for (int w = 0; w < wt; ++w) {
            double term = live ? dmp_source_event_pick(rows[(size_t)(r0 + w) * a.n], l) : 0.0;
            term = dmp_wave_sum(term);
            if ((tid & 63) == 0) red_j[w][tid >> 6] = term;
        }
        __syncthreads();
        if (tid < wt) out[(size_t)(r0 + tid) * per] = dmp_sum_in_order(red_j[tid], 4);
    }
}

// scores[r][c][t] = the `per` partials of line i = (c * maxTime + t) * R + r, in ascending block order
__global__ __launch_bounds__(256) void k_dmp_source_events_add(const double* __restrict__ partial, unsigned per, size_t lines, int R,
                                                              long stride, double* __restrict__ scores) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < lines; i += (size_t)gridDim.x * 256)
        scores[(i % R) * (size_t)stride + i / R] = dmp_sum_in_order(partial + i * per, (int)per);
}

int gn_dmp_source_events_set_attributes() {       // once per device, from gnode_graph_create
    GN_HIP(hipFuncSetAttribute((const void*)k_dmp_source_events_wg<kDmpSourceEventsTile>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)kDmpLdsLimit));
    return 0;
}

// ------------------------------------------------------------------------------------------------ the host side
// The workspace of a call, gnode_dmp_source_batch.hip's.  The one-workgroup form uses none: one aligned unit, so that the query
// is not 0 for a call that is served.  The general form: theta x2, phi, ps over C * nnz edge slots, P, Pr, Pi over C * n rows,
// and the partials [C][maxTime][R][blocks per candidate] in fp64.  With `base` null only `bytes` means anything.
struct DmpSourceEventsWorkspace {
    float *theta[2], *phi, *ps, *P, *Pr, *Pi;
    double* partial;
    size_t bytes;
};
static DmpSourceEventsWorkspace dmp_source_events_carve(gnode_graph_t g, size_t C, size_t R, size_t maxTime, bool general, void* base) {
    const size_t edges = (size_t)std::max<int64_t>(g->nnz, 1), n = (size_t)g->info.n, ng = (n + 255) / 256;
    const size_t EB = general ? gn_align(C * edges * 4) : 0, NB = general ? gn_align(C * n * 4) : 0;
    size_t at = 0;
    auto take = [&](size_t bytes) { char* p = base ? (char*)base + at : nullptr; at += bytes; return p; };
    DmpSourceEventsWorkspace w;
    w.theta[0] = (float*)take(EB); w.theta[1] = (float*)take(EB); w.phi = (float*)take(EB); w.ps = (float*)take(EB);
    w.P = (float*)take(NB); w.Pr = (float*)take(NB); w.Pi = (float*)take(NB);
    w.partial = (double*)take(general ? gn_align(C * maxTime * R * ng * 8) : 256);
    w.bytes = at;
    return w;
}
extern "C" size_t gnode_dmp_source_events_workspace_bytes(gnode_graph_t g, int32_t C, int32_t R, int32_t maxTime) {
    return g && C >= 1 && R >= 1 && maxTime >= 2
               ? dmp_source_events_carve(g, (size_t)C, (size_t)R, (size_t)maxTime, !dmp_source_events_one_workgroup(g), nullptr).bytes
               : 0;
}

// What the call settles before it writes anything, in gnode_dmp_source_batch_scores_f32's order: its arguments, the form and
// its launch shape, the workspace's size, the pattern's symmetry.
extern "C" int gnode_dmp_source_events_scores_f32(gnode_graph_t g, const float* weights, const float* gamma, const int32_t* candidates,
                                                  int32_t C, const int8_t* rows, int32_t R, float floor, int32_t maxTime, double* scores,
                                                  int64_t score_stride, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "gnode_dmp_source_events_scores_f32";
    GN_CHECK_ARG(g && gamma && candidates && rows && scores && workspace, "%s: null pointer", who);
    GN_CHECK_ARG(weights || g->nnz == 0, "%s: weights is null", who);          // no edge, no weight: an empty tensor has no address
    GN_CHECK_ARG(maxTime >= 2, "%s: maxTime must be >= 2 (got %d)", who, maxTime);
    GN_CHECK_ARG(C >= 1, "%s: C must be >= 1 (got %d)", who, C);
    GN_CHECK_ARG(R >= 1, "%s: R must be >= 1 (got %d)", who, R);
    GN_CHECK_ARG(floor > 0.0f && floor <= 1.0f, "%s: floor must be in (0, 1] (got %g)", who, (double)floor);      // (a NaN fails it)
    GN_CHECK_ARG(score_stride >= (int64_t)C * maxTime, "%s: score_stride %lld < C * maxTime = %lld", who, (long long)score_stride,
                 (long long)C * maxTime);
    const int n = g->info.n;
    const long nnz = g->nnz;
    const unsigned ng = (unsigned)((n + 255) / 256), eg = (unsigned)std::max<long>(1, (nnz + 255) / 256);
    const bool one_wg = dmp_source_events_one_workgroup(g);
    const unsigned threads = (unsigned)std::min<long>(1024, std::max<long>(64, (std::max<long>(n, nnz) + 63) / 64 * 64));
    const int tile = one_wg ? dmp_source_events_wg_tile(g) : kDmpSourceEventsTile;
    const unsigned tiles = (unsigned)((R + tile - 1) / tile);
    GN_CHECK_ARG((size_t)C * (one_wg ? tiles : std::max(ng, eg)) < ((size_t)1 << 31), "%s: C = %d is too many candidates for this graph%s",
                 who, C, one_wg ? " and R" : "");
    const size_t bytes = dmp_source_events_carve(g, (size_t)C, (size_t)R, (size_t)maxTime, !one_wg, nullptr).bytes;
    if (workspace_bytes < bytes) {
        gnode_set_error("%s: workspace %zu < %zu", who, workspace_bytes, bytes);
        return GNODE_ERR_WORKSPACE;
    }
    GN_CHECK_ARG(g->symmetric, "%s: the sparsity pattern is not symmetric (DMP here serves undirected graphs)", who);
    const DmpSourceEventsWorkspace ws = dmp_source_events_carve(g, (size_t)C, (size_t)R, (size_t)maxTime, !one_wg, workspace);
    hipStream_t st = (hipStream_t)stream;
    GN_HIP(hipStreamSynchronize(st));          // nothing waits on the host here: only the documented contract (include/gnode.h) keeps it
    const DmpSourceEventsArgs a = {weights, gamma, candidates, rows, floor, scores, (long)score_stride, n, maxTime, R, nnz};
    if (one_wg) {
        const size_t lds = gnode_dmp_batch_lds_bytes(g) + (size_t)tile * kDmpSourceEventsRedBytes;
        hipLaunchKernelGGL(k_dmp_source_events_wg<kDmpSourceEventsTile>, dim3((unsigned)C * tiles), dim3(threads), lds, st, g->rowptr, g->src,
                           g->rev, a, tile, tiles);
        GN_LAUNCH_CHECK();
        return 0;
    }
    const dim3 gn((unsigned)C * ng), ge((unsigned)C * eg);
    auto node = k_dmp_source_events_node<kDmpSourceEventsTile>;
    hipLaunchKernelGGL(node, gn, dim3(256), 0, st, g->rowptr, g->rev, ws.theta[0], a, ng, 0, ws.P, ws.Pr, ws.Pi, ws.partial);
    hipLaunchKernelGGL(k_dmp_source_init<DmpSourceEventsArgs>, ge, dim3(256), 0, st, g->src, a, eg, ws.theta[0], ws.phi, ws.ps);
    GN_LAUNCH_CHECK();
    for (int t = 1; t < maxTime; ++t) {
        const int cur = (t - 1) & 1;
        hipLaunchKernelGGL(node, gn, dim3(256), 0, st, g->rowptr, g->rev, ws.theta[cur], a, ng, t, ws.P, ws.Pr, ws.Pi, ws.partial);
        if (t + 1 < maxTime)                 // (the last step's messages have no reader)
            hipLaunchKernelGGL(k_dmp_source_edge<DmpSourceEventsArgs>, ge, dim3(256), 0, st, g->src, g->rev, ws.P, ws.theta[cur], a, eg, ws.phi,
                               ws.ps, ws.theta[cur ^ 1]);
        GN_LAUNCH_CHECK();
    }
    const size_t lines = (size_t)C * maxTime * R;
    hipLaunchKernelGGL(k_dmp_source_events_add, dim3((unsigned)std::min<size_t>((lines + 255) / 256, 65536)), dim3(256), 0, st, ws.partial, ng,
                       lines, R, (long)score_stride, scores);
    GN_LAUNCH_CHECK();
    return 0;
}
