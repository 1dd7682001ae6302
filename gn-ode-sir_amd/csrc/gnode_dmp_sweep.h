// The candidate sweep, stated once for gnode_dmp_source.hip, gnode_dmp_source_batch.hip, gnode_dmp_source_events.hip and
// gnode_dmp_outbreak.hip, and for the last two under a rate schedule (gnode_dmp_source_events_schedule.hip,
// gnode_dmp_outbreak_schedule.hip): the DMP recurrence of gnode_dmp.h from C synthesised starts on one graph, with no marginal
// written to memory and only fixed-order fp64 sums of what the node pass holds in registers.
//
// C candidates; candidate c's sample starts from a state that the kernels synthesise from the candidate id wherever
// gnode_dmp.hip reads a start: no [C][n][3] state exists.  The weights [nnz] and gamma [n] are shared by the candidates.  At
// every step t = 0 .. maxTime - 1 (row 0 is the start itself) the node pass holds Ps, Pi, Pr of node k in registers and adds
// the node's term to each of S sums per candidate and step, in fp64, in a fixed order and without atomics: a thread adds its
// own nodes in ascending k, dmp_wave_sum adds a wave's 64 lanes in a fixed tree, dmp_sum_in_order adds the waves' sums in
// ascending wave order and, in the general form, the per-block partials in ascending block order.  Two forms, chosen from the
// graph alone like gnode_dmp_batch_f32's (dmp_sweep_tile):
//   one workgroup per candidate and tile of sums
//                 the messages and marginals of the sample live in LDS for the whole horizon, with 2 * 16 doubles per sum of the
//                 tile behind them: one launch.  A reader with kTiled has the recurrence of a candidate run ceil(S / tile)
//                 times; on a graph whose LDS leaves less room than W sums the tile narrows, down to 1, and the form stays.
//   general       rows c * n + k and edge slots c * nnz + e of the workspace, `per` blocks of 256 per candidate: two launches
//                 per time step, one for row 0 and the messages' start each, and the final add of the partials
//                 [c][t][s][block].  The recurrence of a candidate runs once whatever S is.
// A candidate's sums do not depend on C, on S or on its position in the call: same expressions, same per-element order, and the
// reduction tree is a function of the graph alone.
//
// What varies between the entries is a READER, a type of static members that the kernels and the host side take as a template
// argument:
//   Args          the kernels' argument struct: DmpSweepArgs, which dmp_sweep_run fills, and behind it the entry's own
//   W, kTiled     W sums a thread accumulates at once (indexed by unrolled constants only: they stay in registers).  kTiled:
//                 S = a.S is the call's and goes in tiles of at most W; else S = W
//   start, ps0    the synthesised start (Ps_0, Pi_0, Pr_0) of node k for candidate id `cand`, and its Ps_0 alone
//   Terms, terms  what the node pass keeps of (ps, pi, pr) and of the previous step's (ps_prev, pr_prev), which are (1, 0) at row
//                 0: once per node and step.  A reader that ignores ps_prev leaves no trace of its load.
//   pick          node k's term of sum s0 + w from its Terms; s0 is uniform (a tile's or a group's first sum), w small
//   out           where the finished sum s of row ct = c * maxTime + t goes
//   Rates         the tables that govern a step, see below: DmpConstantRates, or DmpScheduledRates under a rate schedule
//
// RATES.  The kernels never read a.w or a.gamma themselves: R::Rates::of(a, c) gives sample c's view, whose w(a, t) and
// gamma(a, t) are the tables of step t = 1 .. maxTime - 1.  The reads follow gnode_dmp_schedule.hip's table: dmp_edge_start
// reads w(1); the node pass of step t reads gamma(t); the edge pass of step t reads w(t), gamma(t) and, for theta_{t+1}, w(t + 1)
// -- the two-weight dmp_edge_update of gnode_dmp.h -- and runs only when t + 1 < maxTime, so step t + 1 exists wherever it is
// read.  DmpConstantRates returns a.w and a.gamma whatever t is: the two weights are one load and the instances are what they
// were before the policy existed.  DmpScheduledRates (DmpScheduled<R> makes the reader) reads tables w[P][nnz], gamma[P][n] shared
// by the samples, a phase row [L] and one SHIFT per sample: step t of sample c is governed by phase[shift[c] + t], a schedule
// stated in calendar steps met by a run that starts shift[c] steps into it.  c is uniform over a block in both forms, so the
// shift and phase reads are uniform loads and the barriers stay in uniform control flow.  The tables stay in memory, never in
// LDS: the form and the tile are dmp_sweep_tile<R>(g)'s whatever the rates are.
#pragma once
#include "gnode_dmp.h"
#include <algorithm>
#include <string>
#include <type_traits>

struct DmpSweepArgs {
    const float* w; const float* gamma;         // [nnz], [n]
    const int32_t* cand;                        // [C]
    int n, maxTime; long nnz;
    int S, tile; unsigned tiles;                // of a kTiled reader: its sums, and how the one-workgroup form tiles them
};
static constexpr size_t kDmpSweepRedBytes = 2 * 16 * sizeof(double);        // per sum of a tile: the waves' sums of a step, two steps' worth

// the start of source inference: one-hot at the candidate, Pr_0 = 0; an id outside the graph matches no node
struct DmpOneHotStart {
    static __device__ __forceinline__ void start(const DmpSweepArgs&, int k, int cand, float& ps0, float& pi0, float& pr0) {
        dmp_source_state(k, cand, ps0, pi0);
        pr0 = 0.0f;
    }
    static __device__ __forceinline__ float ps0(const DmpSweepArgs& a, int k, int cand) {
        float ps0, pi0, pr0;
        start(a, k, cand, ps0, pi0, pr0);
        return ps0;
    }
};

// constant rates: one table of each kind for every sample and step
struct DmpConstantRates {
    template <class A> static __device__ __forceinline__ DmpConstantRates of(const A&, size_t) { return {}; }
    template <class A> __device__ __forceinline__ const float* w(const A& a, int) const { return a.w; }
    template <class A> __device__ __forceinline__ const float* gamma(const A& a, int) const { return a.gamma; }
    template <class A> static __host__ __device__ __forceinline__ int edge_step(const A&) { return 0; }      // (no table depends on it)
    template <class A> static void set_edge_step(A&, int) {}
};
// a rate schedule: a.w is [P][nnz], a.gamma [P][n]; `steps` is the sample's window of the phase row, steps[t] = phase[shift + t]
struct DmpScheduledRates {
    const int32_t* steps;
    template <class A> static __device__ __forceinline__ DmpScheduledRates of(const A& a, size_t c) { return {a.phase + a.shift[c]}; }
    template <class A> __device__ __forceinline__ const float* w(const A& a, int t) const { return a.w + (size_t)steps[t] * (size_t)a.nnz; }
    template <class A> __device__ __forceinline__ const float* gamma(const A& a, int t) const { return a.gamma + (size_t)steps[t] * (size_t)a.n; }
    // k_dmp_sweep_edge has no step among its arguments (under constant rates it needs none): the host loop of the general form
    // writes the step into the arguments of each edge launch
    template <class A> static __device__ __forceinline__ int edge_step(const A& a) { return a.edge_step; }
    template <class A> static void set_edge_step(A& a, int t) { a.edge_step = t; }
};
// reader R under a schedule: R's start, terms and sums, with the phase row and the shifts behind R's arguments
template <class R>
struct DmpScheduled : R {
    struct Args : R::Args {
        const int32_t* phase;                   // device [L], entries in [0, P)
        const int32_t* shift;                   // device [C], shift[c] + maxTime <= L
        int edge_step;                          // the general form's edge launch: its step (DmpScheduledRates::edge_step)
    };
    using Rates = DmpScheduledRates;
};

template <class R> __device__ __forceinline__ int dmp_sweep_sums(const typename R::Args& a) { return R::kTiled ? a.S : R::W; }

// The waves' sums of one step: sum w's at red[w * 16 + wave].  Every lane of the wave is active where this is called.  With a
// constant wt (a reader that is not kTiled) all sums are taken before lane 0 stores any, so that their independent shuffle chains
// overlap; where `w < wt` is a branch they cannot, and each sum is stored where it is taken, which keeps fewer values live.
template <class R>
__device__ __forceinline__ void dmp_sweep_wave_sums(double (&acc)[R::W], int wt, int lane, int wave, double* red) {
    if constexpr (R::kTiled) {
#pragma unroll
        for (int w = 0; w < R::W; ++w)
            if (w < wt) {
                const double s = dmp_wave_sum(acc[w]);
                if (lane == 0) red[w * 16 + wave] = s;
            }
    } else {
#pragma unroll
        for (int w = 0; w < R::W; ++w) acc[w] = dmp_wave_sum(acc[w]);
        if (lane == 0) {
#pragma unroll
            for (int w = 0; w < R::W; ++w) red[w * 16 + wave] = acc[w];
        }
    }
}

// One workgroup = one candidate and `tile` <= W consecutive sums, every step: k_dmp_batch_wg with the start synthesised and the
// output rows replaced by their sums.  Block b serves candidate b / tiles and the sums from (b % tiles) * tile on, `wt` of them.
// Thread `tid` owns nodes and edges tid, tid + blockDim.x, ... in both passes; blockDim.x is a multiple of 64 and at most 1024
// (16 waves).  The barriers sit in uniform control flow (the step loop's bounds are kernel arguments), so every thread reaches
// each of them.  acc[] is indexed by unrolled constants only, and the `w < wt` tests are uniform over the workgroup.  red holds
// [2][tile][16] doubles: step t's wave sums of sum w at red[(t & 1) * tile * 16 + w * 16 + wave], read by thread w after the
// barrier that follows the node pass while the other waves go on, and next written two barriers later.  P[k] and Pr[k] are read
// before they are written: they still hold step t - 1's product and Pr.
template <class R>
__global__ __launch_bounds__(1024) void k_dmp_sweep_wg(const int* __restrict__ rowptr, const int* __restrict__ src,
                                                      const int* __restrict__ rev_g, typename R::Args a) {
    extern __shared__ __attribute__((aligned(16))) char dmp_smem[];
    const int n = a.n, nnz = (int)a.nnz, tid = threadIdx.x, nt = blockDim.x, wave = tid >> 6, lane = tid & 63, waves = nt >> 6;
    const DmpLds L = dmp_lds(dmp_smem, n, nnz);
    double* red = (double*)L.rest;
    const int tile = R::kTiled ? a.tile : R::W;
    const unsigned tiles = R::kTiled ? a.tiles : 1u;
    const unsigned c = blockIdx.x / tiles;
    const int first = (int)(blockIdx.x % tiles) * tile, wt = min(tile, dmp_sweep_sums<R>(a) - first);
    const int cand = a.cand[c];
    const typename R::Rates rates = R::Rates::of(a, c);
    const size_t ct0 = (size_t)c * a.maxTime;
    double acc[R::W];
#pragma unroll
    for (int w = 0; w < R::W; ++w) acc[w] = 0.0;
    for (int k = tid; k < n; k += nt) {                                   // row 0; Pi, Pr hold the start for step 1
        float ps0, pi0, pr0;
        R::start(a, k, cand, ps0, pi0, pr0);
        L.Pi[k] = pi0; L.Pr[k] = pr0;
        const typename R::Terms l = R::terms(a, k, ps0, pi0, pr0, 1.0f, 0.0f);        // before the start: all susceptible
#pragma unroll
        for (int w = 0; w < R::W; ++w)
            if (w < wt) acc[w] = acc[w] + R::pick(a, l, k, first, w);
    }
    dmp_sweep_wave_sums<R>(acc, wt, lane, wave, red);
    {
        const float* w1 = rates.w(a, 1);                                  // (maxTime >= 2: step 1 exists)
        for (int e = tid; e < nnz; e += nt) {
            float ps0, pi0, pr0;
            R::start(a, src[e], cand, ps0, pi0, pr0);
            dmp_edge_start(ps0, pi0, w1[e], L.theta0[e], L.phi[e], L.ps[e]);
            L.rev[e] = rev_g[e];
        }
    }
    __syncthreads();
    if (tid < wt) *R::out(a, ct0, first + tid) = dmp_sum_in_order(red + tid * 16, waves);
    for (int t = 1; t < a.maxTime; ++t) {
        const float* th = L.theta((t - 1) & 1);
        float* th_next = L.theta(t & 1);
        double* red_t = red + (size_t)(t & 1) * tile * 16;
        const float* gam = rates.gamma(a, t);
#pragma unroll
        for (int w = 0; w < R::W; ++w) acc[w] = 0.0;
        for (int k = tid; k < n; k += nt) {                               // node pass
            const float p = dmp_row_product(L.rev, th, rowptr[k], rowptr[k + 1]);
            const float ps0 = R::ps0(a, k, cand);
            const float ps_prev = t == 1 ? ps0 : ps0 * L.P[k], pr_prev = L.Pr[k];       // (no product exists before step 1)
            L.P[k] = p;
            float sk, pi, pr;
            dmp_node_update(p, ps0, L.Pi[k], pr_prev, gam[k], sk, pi, pr);
            L.Pr[k] = pr; L.Pi[k] = pi;
            const typename R::Terms l = R::terms(a, k, sk, pi, pr, ps_prev, pr_prev);
#pragma unroll
            for (int w = 0; w < R::W; ++w)
                if (w < wt) acc[w] = acc[w] + R::pick(a, l, k, first, w);
        }
        dmp_sweep_wave_sums<R>(acc, wt, lane, wave, red_t);
        __syncthreads();                                                  // P and the wave sums are complete; theta[cur] is still this step's
        if (tid < wt) *R::out(a, ct0 + t, first + tid) = dmp_sum_in_order(red_t + tid * 16, waves);
        if (t + 1 < a.maxTime) {                                          // (the last step's messages have no reader)
            const float* w = rates.w(a, t);
            const float* w_next = rates.w(a, t + 1);
            for (int e = tid; e < nnz; e += nt) {                         // edge pass
                const int u = src[e];
                dmp_edge_update(L.P[u], th[L.rev[e]], R::ps0(a, u, cand), w[e], w_next[e], gam[u], L.phi[e], L.ps[e], th[e], th_next[e]);
            }
        }
        __syncthreads();                                                  // theta[next] is complete before its node pass
    }
}

// The general form: `per` blocks of 256 per candidate, candidate c = blockIdx.x / per; per-candidate state at row c * n + k and
// edge slot c * nnz + e of the workspace arrays.  The messages' start:
template <class R>
__global__ __launch_bounds__(256) void k_dmp_sweep_init(const int* __restrict__ src, typename R::Args a, unsigned per,
                                                       float* __restrict__ theta, float* __restrict__ phi, float* __restrict__ ps) {
    const size_t c = blockIdx.x / per;
    const long e = (long)(blockIdx.x % per) * 256 + threadIdx.x;
    if (e >= a.nnz) return;
    const size_t slot = c * (size_t)a.nnz + e;
    float ps0, pi0, pr0;
    R::start(a, src[e], a.cand[c], ps0, pi0, pr0);
    dmp_edge_start(ps0, pi0, R::Rates::of(a, c).w(a, 1)[e], theta[slot], phi[slot], ps[slot]);
}

// Step t of every candidate's nodes, once, and the block's partial of EVERY sum s of (c, t); t = 0 is the start itself (theta,
// P, Pr, Pi are not read), and step 1 starts from the state, so the workspace is never read before it is written.  No thread
// leaves before the barriers: one past the last node contributes 0 to every sum.  The sums go in groups of W: group j's wave
// sums at red[j & 1], one barrier, then thread w < wt adds the four of sum s0 + w; the same half is next written after the
// barrier of group j + 1, which those threads reach after reading.
template <class R>
__global__ __launch_bounds__(256) void k_dmp_sweep_node(const int* __restrict__ rowptr, const int* __restrict__ rev,
                                                       const float* __restrict__ theta, typename R::Args a, unsigned per, int t,
                                                       float* __restrict__ P, float* __restrict__ Pr, float* __restrict__ Pi,
                                                       double* __restrict__ partial) {
    __shared__ double red[2][R::W][4];
    const size_t c = blockIdx.x / per;
    const unsigned blk = blockIdx.x % per;
    const int tid = threadIdx.x, k = (int)blk * 256 + tid, S = dmp_sweep_sums<R>(a);
    const bool live = k < a.n;
    typename R::Terms l{};
    if (live) {
        float ps0, pi0, pr0, sk, pi, pr, ps_prev, pr_prev;
        R::start(a, k, a.cand[c], ps0, pi0, pr0);
        if (t == 0) {
            sk = ps0; pi = pi0; pr = pr0;
            ps_prev = 1.0f; pr_prev = 0.0f;                               // before the start: all susceptible
        } else {
            const size_t r = c * (size_t)a.n + k;
            const float p = dmp_row_product(rev, theta + c * (size_t)a.nnz, rowptr[k], rowptr[k + 1]);
            ps_prev = t == 1 ? ps0 : ps0 * P[r];                          // step 1 starts from the state itself: no product yet
            pr_prev = t == 1 ? pr0 : Pr[r];
            P[r] = p;
            dmp_node_update(p, ps0, t == 1 ? pi0 : Pi[r], pr_prev, R::Rates::of(a, c).gamma(a, t)[k], sk, pi, pr);
            Pr[r] = pr; Pi[r] = pi;
        }
        l = R::terms(a, k, sk, pi, pr, ps_prev, pr_prev);
    }
    double* out = partial + (c * (size_t)a.maxTime + t) * S * per + blk;             // sum s at out[s * per]
    for (int s0 = 0, j = 0; s0 < S; s0 += R::W, ++j) {
        const int wt = min(R::W, S - s0);
        double(*red_j)[4] = red[j & 1];
        for (int w = 0; w < wt; ++w) {
            double term = live ? R::pick(a, l, k, s0, w) : 0.0;
            term = dmp_wave_sum(term);
            if ((tid & 63) == 0) red_j[w][tid >> 6] = term;
        }
        __syncthreads();
        if (tid < wt) out[(size_t)(s0 + tid) * per] = dmp_sum_in_order(red_j[tid], 4);
    }
}

// the edge pass of step t
template <class R>
__global__ __launch_bounds__(256) void k_dmp_sweep_edge(const int* __restrict__ src, const int* __restrict__ rev,
                                                       const float* __restrict__ P, const float* __restrict__ theta, typename R::Args a,
                                                       unsigned per, float* __restrict__ phi, float* __restrict__ ps,
                                                       float* __restrict__ theta_next) {
    const size_t c = blockIdx.x / per;
    const long e = (long)(blockIdx.x % per) * 256 + threadIdx.x;
    if (e >= a.nnz) return;
    const size_t base = c * (size_t)a.nnz, slot = base + e;
    const int u = src[e];
    const typename R::Rates rates = R::Rates::of(a, c);
    const int t = R::Rates::edge_step(a);
    dmp_edge_update(P[c * (size_t)a.n + u], theta[base + rev[e]], R::ps0(a, u, a.cand[c]), rates.w(a, t)[e], rates.w(a, t + 1)[e],
                    rates.gamma(a, t)[u], phi[slot], ps[slot], theta[slot], theta_next[slot]);
}

// sum s of row ct = the `per` partials of line i = ct * S + s, in ascending block order
template <class R>
__global__ __launch_bounds__(256) void k_dmp_sweep_add(const double* __restrict__ partial, unsigned per, size_t lines, typename R::Args a) {
    const size_t S = (size_t)dmp_sweep_sums<R>(a);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < lines; i += (size_t)gridDim.x * 256)
        *R::out(a, i / S, i % S) = dmp_sum_in_order(partial + i * per, (int)per);
}

// ------------------------------------------------------------------------------------------------ the host side
// The one-workgroup form's tile on this graph: what the LDS left by the sample's arrays holds, at most W; 0 where it holds less
// than the reader can do with (one sum if kTiled, else all W), and the general form serves.
template <class R> static int dmp_sweep_tile(gnode_graph_t g) {
    const size_t arrays = gnode_dmp_batch_lds_bytes(g);
    const size_t room = arrays < kDmpLdsLimit ? (kDmpLdsLimit - arrays) / kDmpSweepRedBytes : 0;
    return room >= (size_t)(R::kTiled ? 1 : R::W) ? (int)std::min<size_t>(room, (size_t)R::W) : 0;
}
// the LDS of the one-workgroup form with a full tile: the forward's arrays | the fp64 reduction scratch
template <class R> static size_t dmp_sweep_lds_bytes(gnode_graph_t g) { return g ? gnode_dmp_batch_lds_bytes(g) + R::W * kDmpSweepRedBytes : 0; }

template <class R> static int dmp_sweep_set_attributes() {       // once per device, from gnode_graph_create
    GN_HIP(hipFuncSetAttribute((const void*)k_dmp_sweep_wg<R>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kDmpLdsLimit));
    return 0;
}

// The workspace of a call.  The one-workgroup form keeps everything in LDS and uses none of it: one aligned unit, so that the
// query is not 0 for a call that is served.  The general form: theta x2, phi, ps over C * nnz edge slots, P, Pr, Pi over C * n
// rows, the partials [lines = C * maxTime * S][blocks per candidate] in fp64.  With `base` null only `bytes` means anything.
struct DmpSweepWorkspace {
    float *theta[2], *phi, *ps, *P, *Pr, *Pi;
    double* partial;
    size_t bytes;
};
static inline DmpSweepWorkspace dmp_sweep_carve(gnode_graph_t g, size_t C, size_t lines, bool general, void* base) {
    const size_t edges = (size_t)std::max<int64_t>(g->nnz, 1), n = (size_t)g->info.n, ng = (n + 255) / 256;
    const size_t EB = general ? gn_align(C * edges * 4) : 0, NB = general ? gn_align(C * n * 4) : 0;
    size_t at = 0;
    auto take = [&](size_t bytes) { char* p = base ? (char*)base + at : nullptr; at += bytes; return p; };
    DmpSweepWorkspace w;
    w.theta[0] = (float*)take(EB); w.theta[1] = (float*)take(EB); w.phi = (float*)take(EB); w.ps = (float*)take(EB);
    w.P = (float*)take(NB); w.Pr = (float*)take(NB); w.Pi = (float*)take(NB);
    w.partial = (double*)take(general ? gn_align(lines * ng * 8) : 256);
    w.bytes = at;
    return w;
}
template <class R> static size_t dmp_sweep_workspace_bytes(gnode_graph_t g, int32_t C, int32_t maxTime, int32_t S) {
    return g && C >= 1 && S >= 1 && maxTime >= 2 ? dmp_sweep_carve(g, (size_t)C, (size_t)C * maxTime * S, dmp_sweep_tile<R>(g) == 0, nullptr).bytes : 0;
}

// What a call settles before it writes anything, in dmp_preamble's order (gnode_dmp.hip): its arguments -- these, then the
// entry's own --, the form and its launch shape, the workspace's size, the pattern's symmetry.  `pointers`: none of the entry's
// other pointers is null.
static inline int dmp_sweep_arguments(const char* who, gnode_graph_t g, bool pointers, const float* weights, int32_t maxTime, int32_t C) {
    GN_CHECK_ARG(g && pointers, "%s: null pointer", who);
    GN_CHECK_ARG(weights || g->nnz == 0, "%s: weights is null", who);          // no edge, no weight: an empty tensor has no address
    GN_CHECK_ARG(maxTime >= 2, "%s: maxTime must be >= 2 (got %d)", who, maxTime);
    GN_CHECK_ARG(C >= 1, "%s: C must be >= 1 (got %d)", who, C);
    return 0;
}

// A rate schedule as an entry receives it (a DmpScheduled<R> call): P tables of each kind on the device, the phase row [L] and
// the shifts [C] on the host; shifts_host null means 0 for every sample.  Its device copies lead the workspace -- phase [L],
// then shift [C], each rounded up to gn_align's unit -- and dmp_sweep_carve's regions follow.
struct DmpSweepSchedule {
    const int32_t* phase_host; int32_t P, L;
    const int32_t* shifts_host;
};
static inline size_t dmp_sweep_schedule_bytes(size_t C, size_t L) { return gn_align(L * sizeof(int32_t)) + gn_align(C * sizeof(int32_t)); }
// the entry's own checks of a schedule, after dmp_sweep_arguments and whatever else the entry checks of its arguments
static inline int dmp_sweep_schedule_arguments(const char* who, const DmpSweepSchedule& s, int32_t maxTime, int32_t C) {
    GN_CHECK_ARG(s.phase_host, "%s: null pointer", who);
    GN_CHECK_ARG(s.P >= 1, "%s: a schedule has at least one phase (P = %d)", who, s.P);
    GN_CHECK_ARG(s.L >= maxTime, "%s: the phase row names L = %d steps, the call has maxTime = %d", who, s.L, maxTime);
    for (int i = 1; i < s.L; ++i)              // (entry 0 is never read: shift >= 0 and t >= 1)
        GN_CHECK_ARG(s.phase_host[i] >= 0 && s.phase_host[i] < s.P, "%s: phase[%d] = %d is not in [0, %d)", who, i, s.phase_host[i], s.P);
    if (s.shifts_host)
        for (int c = 0; c < C; ++c)
            GN_CHECK_ARG(s.shifts_host[c] >= 0 && (int64_t)s.shifts_host[c] + maxTime <= s.L,
                         "%s: shifts[%d] = %d is not in [0, L - maxTime = %d]", who, c, s.shifts_host[c], s.L - maxTime);
    return 0;
}
template <class R> static size_t dmp_sweep_schedule_workspace_bytes(gnode_graph_t g, int32_t C, int32_t maxTime, int32_t S, int32_t L) {
    const size_t sweep = dmp_sweep_workspace_bytes<R>(g, C, maxTime, S);
    return sweep && L >= maxTime ? dmp_sweep_schedule_bytes((size_t)C, (size_t)L) + sweep : 0;
}

// ... and the launches.  `a`: the entry's own members are set, its DmpSweepArgs is filled here.  `and_what` completes the
// refusal of a grid that C and a kTiled reader's S make too large.  `wait_first`: the entry's documented contract
// (include/gnode.h) has it synchronise the stream before it enqueues; nothing here waits on the host otherwise.  `schedule`
// (checked by dmp_sweep_schedule_arguments), for a DmpScheduled<R> and for nothing else: weights and gamma are its P tables,
// which are read back and validated once every other refusal is past (dmp_check_rate_tables names the phase and the position);
// then the phase row and the shifts are staged at the head of the workspace and the stream is synchronised once, so that the
// host arrays are done with when the call returns.
template <class R>
static int dmp_sweep_run(const char* who, const char* and_what, gnode_graph_t g, const float* weights, const float* gamma,
                         const int32_t* candidates, int32_t C, int32_t maxTime, int32_t S, typename R::Args a, bool wait_first,
                         void* workspace, size_t workspace_bytes, void* stream, const DmpSweepSchedule* schedule = nullptr) {
    constexpr bool kScheduled = std::is_same<typename R::Rates, DmpScheduledRates>::value;
    const int n = g->info.n;
    const long nnz = g->nnz;
    const unsigned ng = (unsigned)((n + 255) / 256), eg = (unsigned)std::max<long>(1, (nnz + 255) / 256);
    const int wg_tile = dmp_sweep_tile<R>(g);
    const bool one_wg = wg_tile > 0;
    const unsigned threads = (unsigned)std::min<long>(1024, std::max<long>(64, (std::max<long>(n, nnz) + 63) / 64 * 64));
    const int tile = one_wg ? wg_tile : R::W;
    const unsigned tiles = (unsigned)((S + tile - 1) / tile);
    GN_CHECK_ARG((size_t)C * (one_wg ? tiles : std::max(ng, eg)) < ((size_t)1 << 31), "%s: C = %d is too many candidates for this graph%s",
                 who, C, one_wg ? and_what : "");
    const size_t lines = (size_t)C * maxTime * S;
    const size_t head = kScheduled ? dmp_sweep_schedule_bytes((size_t)C, (size_t)schedule->L) : 0;
    const size_t bytes = head + dmp_sweep_carve(g, (size_t)C, lines, !one_wg, nullptr).bytes;
    if (workspace_bytes < bytes) {
        gnode_set_error("%s: workspace %zu < %zu", who, workspace_bytes, bytes);
        return GNODE_ERR_WORKSPACE;
    }
    GN_CHECK_ARG(g->symmetric, "%s: the sparsity pattern is not symmetric (DMP here serves undirected graphs)", who);
    const DmpSweepWorkspace ws = dmp_sweep_carve(g, (size_t)C, lines, !one_wg, (char*)workspace + head);
    hipStream_t st = (hipStream_t)stream;
    if (wait_first) GN_HIP(hipStreamSynchronize(st));
    static_cast<DmpSweepArgs&>(a) = {weights, gamma, candidates, n, maxTime, nnz, S, tile, tiles};
    if constexpr (kScheduled) {
        const size_t P = (size_t)schedule->P, L = (size_t)schedule->L;
        if (int rc = dmp_check_rate_tables(who, "weights", weights, 1, P, (size_t)nnz, st)) return rc;
        if (int rc = dmp_check_rate_tables(who, "gamma", gamma, 1, P, (size_t)n, st)) return rc;
        int32_t* phase = (int32_t*)workspace;
        int32_t* shift = (int32_t*)((char*)workspace + gn_align(L * sizeof(int32_t)));
        // entry 0 is never read; it travels as 0 so that the device copy holds no number out of range (L >= maxTime >= 2)
        GN_HIP(hipMemsetAsync(phase, 0, sizeof(int32_t), st));
        if (L > 1) GN_HIP(hipMemcpyAsync(phase + 1, schedule->phase_host + 1, sizeof(int32_t) * (L - 1), hipMemcpyHostToDevice, st));
        if (schedule->shifts_host)
            GN_HIP(hipMemcpyAsync(shift, schedule->shifts_host, sizeof(int32_t) * (size_t)C, hipMemcpyHostToDevice, st));
        else
            GN_HIP(hipMemsetAsync(shift, 0, sizeof(int32_t) * (size_t)C, st));
        GN_HIP(hipStreamSynchronize(st));          // phase_host and shifts_host are done with
        a.phase = phase; a.shift = shift; a.edge_step = 0;
    }
    if (one_wg) {
        const size_t lds = gnode_dmp_batch_lds_bytes(g) + (size_t)tile * kDmpSweepRedBytes;
        hipLaunchKernelGGL(k_dmp_sweep_wg<R>, dim3((unsigned)C * tiles), dim3(threads), lds, st, g->rowptr, g->src, g->rev, a);
        GN_LAUNCH_CHECK();
        return 0;
    }
    const dim3 gn((unsigned)C * ng), ge((unsigned)C * eg);
    hipLaunchKernelGGL(k_dmp_sweep_node<R>, gn, dim3(256), 0, st, g->rowptr, g->rev, ws.theta[0], a, ng, 0, ws.P, ws.Pr, ws.Pi, ws.partial);
    hipLaunchKernelGGL(k_dmp_sweep_init<R>, ge, dim3(256), 0, st, g->src, a, eg, ws.theta[0], ws.phi, ws.ps);
    GN_LAUNCH_CHECK();
    for (int t = 1; t < maxTime; ++t) {
        const int cur = (t - 1) & 1;
        hipLaunchKernelGGL(k_dmp_sweep_node<R>, gn, dim3(256), 0, st, g->rowptr, g->rev, ws.theta[cur], a, ng, t, ws.P, ws.Pr, ws.Pi, ws.partial);
        R::Rates::set_edge_step(a, t);
        if (t + 1 < maxTime)                 // (the last step's messages have no reader)
            hipLaunchKernelGGL(k_dmp_sweep_edge<R>, ge, dim3(256), 0, st, g->src, g->rev, ws.P, ws.theta[cur], a, eg, ws.phi, ws.ps,
                               ws.theta[cur ^ 1]);
        GN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_dmp_sweep_add<R>, dim3((unsigned)std::min<size_t>((lines + 255) / 256, 65536)), dim3(256), 0, st, ws.partial, ng, lines, a);
    GN_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------------ rows of codes
// gnode_dmp_source_batch.hip and gnode_dmp_source_events.hip score `count` rows [count][n] (int8) of codes per node in one pass:
// per node and step the possible terms are computed once (T::logs), and every row selects one of them by its code, or 0.0
// (T::pick) -- selected and never indexed, so no row value indexes anything.  They differ in T alone: T::Logs, T::logs of
// (ps, pi, pr, ps_prev, pr_prev, floor), T::pick of (code, logs).  scores[r * stride + c * maxTime + t].
static constexpr int kDmpRowsTile = 16;         // rows per workgroup / per barrier: register counts in DESIGN 4.10, 4.11

struct DmpRowsArgs : DmpSweepArgs {
    const int8_t* rows;                         // [S][n]
    float floor;
    double* scores;                             // [r * stride + c * maxTime + t]
    long stride;
};
template <class T>
struct DmpRowsReader : DmpOneHotStart {
    using Args = DmpRowsArgs;
    using Rates = DmpConstantRates;
    using Terms = typename T::Logs;
    static constexpr int W = kDmpRowsTile;
    static constexpr bool kTiled = true;
    static __device__ __forceinline__ Terms terms(const Args& a, int, float ps, float pi, float pr, float ps_prev, float pr_prev) {
        return T::logs(ps, pi, pr, ps_prev, pr_prev, a.floor);
    }
    static __device__ __forceinline__ double pick(const Args& a, const Terms& l, int k, int r0, int w) {
        return T::pick((a.rows + (size_t)r0 * a.n)[(size_t)w * a.n + k], l);
    }
    static __device__ __forceinline__ double* out(const Args& a, size_t ct, size_t r) { return a.scores + r * (size_t)a.stride + ct; }
};
// the tile that serves this graph: the one-workgroup form's, or the general form's groups
template <class T> static int dmp_rows_tile(gnode_graph_t g) {
    const int tile = g ? dmp_sweep_tile<DmpRowsReader<T>>(g) : 0;
    return !g ? 0 : tile ? tile : kDmpRowsTile;
}
// the entry; `count_name` is what its header calls the number of rows ("O", "R").  Under a rate schedule R is
// DmpScheduled<DmpRowsReader<T>> and `schedule` is the call's.
template <class T, class R = DmpRowsReader<T>>
static int dmp_rows_scores(const char* who, const char* count_name, gnode_graph_t g, const float* weights, const float* gamma,
                           const int32_t* candidates, int32_t C, const int8_t* rows, int32_t count, float floor, int32_t maxTime,
                           double* scores, int64_t score_stride, void* workspace, size_t workspace_bytes, void* stream,
                           const DmpSweepSchedule* schedule = nullptr) {
    if (int e = dmp_sweep_arguments(who, g, gamma && candidates && rows && scores && workspace, weights, maxTime, C)) return e;
    GN_CHECK_ARG(count >= 1, "%s: %s must be >= 1 (got %d)", who, count_name, count);
    GN_CHECK_ARG(floor > 0.0f && floor <= 1.0f, "%s: floor must be in (0, 1] (got %g)", who, (double)floor);      // (a NaN fails it)
    GN_CHECK_ARG(score_stride >= (int64_t)C * maxTime, "%s: score_stride %lld < C * maxTime = %lld", who, (long long)score_stride,
                 (long long)C * maxTime);
    if (schedule)
        if (int e = dmp_sweep_schedule_arguments(who, *schedule, maxTime, C)) return e;
    const std::string and_what = std::string(" and ") + count_name;
    typename R::Args a = {};
    static_cast<DmpRowsArgs&>(a) = {{}, rows, floor, scores, (long)score_stride};
    return dmp_sweep_run<R>(who, and_what.c_str(), g, weights, gamma, candidates, C, maxTime, count, a, true, workspace, workspace_bytes,
                            stream, schedule);
}

// the five terms of gnode_dmp_source_events.hip and gnode_dmp_source_events_schedule.hip: the three states and the two events
struct DmpEventTerms {
    using Logs = DmpSourceEventLogs;
    static __device__ __forceinline__ Logs logs(float ps, float pi, float pr, float ps_prev, float pr_prev, float floor) {
        return dmp_source_event_logs(ps, pi, pr, ps_prev, pr_prev, floor);
    }
    static __device__ __forceinline__ double pick(int o, const Logs& l) { return dmp_source_event_pick(o, l); }
};

// ------------------------------------------------------------------------------------------------ outbreak sizes
// The reader of gnode_dmp_outbreak.hip and gnode_dmp_outbreak_schedule.hip: the base start with the candidate's triple replaced,
// and the three value-weighted sums.
struct DmpOutbreakArgs : DmpSweepArgs {
    const float* init;                          // [n][3], the base start
    const float* value;                         // [n] or null
    int action;                                 // 0 seed, 1 immunise
    double* sizes;                              // [C][maxTime][3]
};
struct DmpOutbreakReader {
    using Args = DmpOutbreakArgs;
    using Rates = DmpConstantRates;
    struct Terms { double s, i, r; };
    static constexpr int W = 3;
    static constexpr bool kTiled = false;
    // the start of node k in the sample of candidate `cand`: the base triple, or the action's where k is the candidate
    static __device__ __forceinline__ void start(const Args& a, int k, int cand, float& ps0, float& pi0, float& pr0) {
        const bool hit = k == cand;
        const float seeded = a.action == 0 ? 1.0f : 0.0f;
        ps0 = hit ? 0.0f : a.init[(size_t)k * 3];
        pi0 = hit ? seeded : a.init[(size_t)k * 3 + 1];
        pr0 = hit ? 1.0f - seeded : a.init[(size_t)k * 3 + 2];
    }
    // ... and its Ps_0 alone, which is all that the steps after the first read of it: 0 under either action
    static __device__ __forceinline__ float ps0(const Args& a, int k, int cand) { return k == cand ? 0.0f : a.init[(size_t)k * 3]; }
    static __device__ __forceinline__ Terms terms(const Args& a, int k, float ps, float pi, float pr, float, float) {
        const double v = a.value ? (double)a.value[k] : 1.0;
        return {v * (double)ps, v * (double)pi, v * (double)pr};
    }
    static __device__ __forceinline__ double pick(const Args&, const Terms& l, int, int j0, int w) {
        return j0 + w == 0 ? l.s : j0 + w == 1 ? l.i : l.r;
    }
    static __device__ __forceinline__ double* out(const Args& a, size_t ct, size_t j) { return a.sizes + (ct * 3 + j); }
};
// the entry.  Under a rate schedule R is DmpScheduled<DmpOutbreakReader> and `schedule` is the call's.
template <class R>
static int dmp_outbreak_sizes(const char* who, gnode_graph_t g, const float* weights, const float* gamma, const float* init,
                              const int32_t* candidates, int32_t C, int32_t action, const float* value, int32_t maxTime, double* sizes,
                              void* workspace, size_t workspace_bytes, void* stream, const DmpSweepSchedule* schedule = nullptr) {
    if (int e = dmp_sweep_arguments(who, g, gamma && init && candidates && sizes && workspace, weights, maxTime, C)) return e;
    GN_CHECK_ARG(action == 0 || action == 1, "%s: action must be 0 (seed) or 1 (immunise) (got %d)", who, action);
    if (schedule)
        if (int e = dmp_sweep_schedule_arguments(who, *schedule, maxTime, C)) return e;
    typename R::Args a = {};
    static_cast<DmpOutbreakArgs&>(a) = {{}, init, value, action, sizes};
    return dmp_sweep_run<R>(who, "", g, weights, gamma, candidates, C, maxTime, 3, a, false, workspace, workspace_bytes, stream, schedule);
}
