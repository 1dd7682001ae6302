// Monte-Carlo SIR label generator for MI355X (gfx950).
//
// Restates sir_torch (reference ode_nn.py:30-88): `sims` independent discrete-time
// SIR trajectories; per step every (infected u -> susceptible v) directed edge
// fires with probability beta and every infected node recovers with probability
// gamma, both decided on the pre-step state (:60-78); per-(t, node) membership
// counts are accumulated (:80-82) with row 0 ASSIGNED (:55-56).
//
// The reference runs ~20 torch launches and >= 4 host syncs per (sim, step) and tests EVERY directed edge
// against the infected set each step (`isin` over all 2E rows, ode_nn.py:61).  Here one workgroup owns one
// trajectory and keeps its FRONTIER -- the list of currently infected nodes -- next to an "ever infected" bitmap in
// LDS; a step walks only the CSR rows of the listed nodes (one 16-lane group per node, very long rows by the whole
// workgroup), draws the recovery coin of each listed node, and builds the next list in the same pass: work per
// step is the frontier's out-degree, not nnz (k_sir_frontier).  Only the two EVENTS a node can have (infection
// step, recovery step) reach memory, as integer atomics; a final pass turns the event histograms into the S/I/R
// counts by a prefix sum over time.  Coins are Philox4x32-10 keyed (CSR position | node, step, trajectory, kind),
// so which edges are visited, in which order, by which lane, or on which GPU cannot change a count: all arithmetic
// is integer, results are bit-exact against the edge-scan statement of the same model (oracle: sir_philox; the
// edge-parallel kernel k_sir_philox below remains for graphs whose lists do not fit and as the in-library
// cross-check of the tests).
//
// Per-node rates (gnode_sir_mc_philox_nodes, the NODES instances): the entry (u -> v) fires against the threshold of
// its TARGET v (the GN-ODE's convention: row v's dS_v = -beta_v (A Z_I)_v Z_S,v) and node u recovers against its own.
// Same coins, same 64-bit compare: constant arrays give the scalar call's counts.
//
// Per-edge probabilities (gnode_sir_mc_philox_edges, the EDGES instances): the entry at CSR position p, in row u with
// col[p] = v, fires against the threshold of w[p], the probability that u infects v (source = row, target = column:
// gnode_dmp_f32's convention for its weights).  The pattern stays symmetric; a directed contact is a zero on the reverse
// entry.  Recovery is per node.  w[p] = beta[col[p]] gives the per-node call's counts, one constant the scalar call's.
//
// Initial-state distributions (gnode_sir_mc_philox_init, the INIT instances): they take uint64 [2][n] -- thr(pS) and thr(pR)
// per node -- and each trajectory DRAWS its start, one coin per node (kind 2, step 0; sir_init_draw below), in place of the
// seed phase; the step loops do not know which form ran.  Row 0 of the counts is then accumulated like every other row
// (k_sir_finalize<ACC0>).  Separate instances, not a run-time test in the shared ones: that form was measured and cost the
// seed-list call 2 % at fb-social size, so the seed-list instances are the code they were before.
//
// Rates that change over time (gnode_sir_mc_philox_schedule, the SCHED instances, EDGES only): P staged tables of per-edge and
// per-node thresholds and an int32 [T] phase table; step `it` reads table phase[it], a wave-uniform choice of two pointers at
// the top of the step (sir_step_thr).  The coins do not know the schedule, so one phase gives the per-edge call's counts.
// Separate instances again: the other forms' step pointers are their kernel arguments, and they compile to what they were
// (DESIGN 4.12).
//
// The candidate sweep (gnode_sir_mc_philox_sweep and its _scores, _timed and _posterior forms; INIT and SCHED instances only): one
// launch runs C x sims jobs, job (c, s) being trajectory s from the drawn start with candidate c's node overridden and the phase
// row read from the candidate's shift on.  What a job puts out -- sums per (candidate, step, compartment), binned similarities
// with snapshots, binned agreement with timed records, per-node counts of the trajectories that match them, or those counts by
// the number of records missed -- is the kernel's
// output policy, its type parameter OUT and its last two arguments (the jobs, the policy): gnode_sir_sweep.h states the six
// policies, the hooks the two step kernels call at every event, every closed step and the end of a job, and the host half of
// each output.  An instance that is not a sweep takes the empty policy and compiles to what it was; a sweep has no histogram,
// no events and no curves.
#include "gnode_common.h"
#include "gnode_sir_plan.h"
#include "gnode_sir_sweep.h"
#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

enum : uint8_t { ST_S = 0, ST_I = 1, ST_R = 2 };

// --------------------------------------------------------------------------- Philox4x32-10
// FOUR consecutive items (CSR positions for infection coins, node ids for recovery coins) share one block: the coin of item
// pos is word (pos & 3) of philox(ctr = (pos >> 2, step, trajectory, kind), key).  Round 2 drew one block per coin and kept
// one word of four: 40 quarter-rate 32-bit multiplies per coin, the kernel's main cost (oracle: philox_coin).
__device__ __forceinline__ void philox_block(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&o)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}
__device__ __forceinline__ uint32_t philox_coin(uint32_t pos, uint32_t it, uint32_t sim, uint32_t kind, uint32_t k0, uint32_t k1) {
    uint32_t w[4];
    philox_block(pos >> 2, it, sim, kind, k0, k1, w);
    const uint32_t j = pos & 3u;
    return j == 0 ? w[0] : j == 1 ? w[1] : j == 2 ? w[2] : w[3];
}

// --------------------------------------------------------------------------- coin thresholds
// A coin fires iff (64-bit) word < thr, thr = floor(p * 2^32) in [0, 2^32].  Scalar instances carry the two thresholds
// as kernel arguments; the NODES instances read thr[v] from two uint64 [n] arrays in memory (staged by the host, L2
// resident).  uint64 because 2^32 + 1 thresholds do not fit 32 bits and p = 1 must always fire: stored whole, the test
// is the scalar one, with nothing to decode.  The EDGES instances (which are NODES instances: recovery stays per node) read
// the infection threshold at the entry's CSR position instead, thr[e], from a uint64 [nnz] array staged the same way.
template <bool NODES> using SirThr = std::conditional_t<NODES, const unsigned long long*, unsigned long long>;
__device__ __forceinline__ unsigned long long sir_thr(unsigned long long t, int) { return t; }
__device__ __forceinline__ unsigned long long sir_thr(const unsigned long long* t, int v) { return t[v]; }

// --------------------------------------------------------------------------- drawn initial state
// Node v of trajectory `sim` starts in S iff coin < thr(pS), else in R iff coin >= 2^32 - thr(pR), else in I; coin = word
// (v & 3) of philox(ctr = (v >> 2, step 0, sim, kind 2)): four consecutive nodes share a block, as the recovery coins do.
// A one-hot row never depends on the coin (thresholds 0 and 2^32).  A thread takes the block of nodes 4q .. 4q + 3: two
// nibbles, bit j = node 4q + j -- `inf` (starts in I) and `rec` (starts in R).
__device__ __forceinline__ void sir_init_draw(const unsigned long long* __restrict__ init_thr, int n, int q, uint32_t sim,
                                              uint32_t k0, uint32_t k1, uint32_t& inf, uint32_t& rec) {
    uint32_t w[4];
    philox_block((uint32_t)q, 0u, sim, 2u, k0, k1, w);
    inf = 0; rec = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int v = 4 * q + j;
        if (v < n) {
            const unsigned long long c = w[j];
            if (c >= init_thr[v]) {
                if (c >= 4294967296ull - init_thr[(size_t)n + v]) rec |= 1u << j; else inf |= 1u << j;
            }
        }
    }
}

// --------------------------------------------------------------------------- per-trajectory output
// TRAJ instances (gnode_sir_mc_philox_traj) also keep what the histograms fold away.  events: int16 [2][sims][n], the step
// at which node v of the call's s-th trajectory was infected (plane 0; 0 for seeds) and recovered (plane 1), over a -1
// background laid by k_fill_i16: one 2-byte store next to every histogram atomic.  curves: uint32 [sims][T][3], the
// trajectory's totals (S_t, I_t, R_t); row 0 is the true initial state, and the rows after an early end of the epidemic
// repeat the final state.  Either pointer may be null (a kernel argument: tested wave-uniformly).  The other instances
// take an empty struct and compile to what they were.
template <bool TRAJ> struct SirTraj {};
template <> struct SirTraj<true> { int16_t* events; uint32_t* curves; };

// INIT instances (gnode_sir_mc_philox_init) take the start thresholds, uint64 [2][n]; the others take an empty struct, as
// with SirTraj, and compile to what they were: the drawn start is no part of a seed-list instance.
template <bool INIT> struct SirInit {};
template <> struct SirInit<true> { const unsigned long long* thr; };

// SCHED instances (gnode_sir_mc_philox_schedule) take the phase table, int32 [T] in memory: step `it` reads its thresholds from
// table phase[it] of P staged ones, thr_beta + phase[it] * nnz and thr_gamma + phase[it] * n -- a wave-uniform choice of two
// pointers at the top of the step, behind which every read of a threshold sees that step's table.  EDGES instances only.  The
// others take an empty struct, as with SirTraj and SirInit, and their step's pointers ARE the kernel's arguments.
template <bool SCHED> struct SirSched {};
template <> struct SirSched<true> { const int32_t* phase; };
template <bool NODES, bool SCHED>
__device__ __forceinline__ SirThr<NODES> sir_step_thr(SirThr<NODES> base, const SirSched<SCHED>& sc, int it, size_t len) {
    if constexpr (SCHED) return base + (size_t)sc.phase[it] * len; else return base;
}

// one event of the [2][T][n] histograms: the SWEEP instances have none
template <bool SWEEP> __device__ __forceinline__ void sir_hist_add(uint32_t* h) { if constexpr (!SWEEP) atomicAdd(h, 1u); }
// the start of nodes 4q .. 4q + 3 (sir_init_draw), with the candidate's bit overridden in the SWEEP instances; node < 0: nobody
template <bool SWEEP>
__device__ __forceinline__ void sir_start_quad(const unsigned long long* __restrict__ init_thr, int n, int q, uint32_t sim, uint32_t k0,
                                               uint32_t k1, int node, int action, uint32_t& inf, uint32_t& rec) {
    sir_init_draw(init_thr, n, q, sim, k0, k1, inf, rec);
    if constexpr (SWEEP) {
        if ((node >> 2) == q) {                    // (node = -1: quad -1, never a thread's)
            const uint32_t bit = 1u << (node & 3);
            if (action == 0) { inf |= bit; rec &= ~bit; } else { rec |= bit; inf &= ~bit; }
        }
    }
}

__device__ __forceinline__ void sir_curve_row(uint32_t* __restrict__ curves, long s, int T, int row, int n, int n_ever, int n_rec) {
    uint32_t* r = curves + ((size_t)s * T + row) * 3;
    r[0] = (uint32_t)(n - n_ever); r[1] = (uint32_t)(n_ever - n_rec); r[2] = (uint32_t)n_rec;
}
// the schedule as job (c, s) reads it: from shifts[c] on in the SWEEP instances, as it is in the others
template <bool SWEEP, bool SCHED, class JOBS>
__device__ __forceinline__ SirSched<SCHED> sir_job_sched(const SirSched<SCHED>& sc, const JOBS& jobs, int c) {
    if constexpr (SWEEP) { SirSched<SCHED> o = sc; o.phase += jobs.shifts[c]; return o; } else return sc;
}

// p[0 .. count) = val.  p is 2-byte aligned only (a caller's view): 16-byte stores over the aligned body, the < 8 elements
// in front of it and behind it by the first workgroup.
__global__ __launch_bounds__(256) void k_fill_i16(int16_t* __restrict__ p, size_t count, int16_t val) {
    const size_t to_align = ((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 1;
    const size_t head = to_align < count ? to_align : count;
    const size_t nvec = (count - head) >> 3;
    uint4* pv = reinterpret_cast<uint4*>(p + head);
    const uint32_t w = (uint32_t)(uint16_t)val * 0x10001u;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (size_t)gridDim.x * 256) pv[i] = make_uint4(w, w, w, w);
    if (blockIdx.x == 0 && threadIdx.x < 8) {
        const size_t t0 = head + nvec * 8;
        if (threadIdx.x < head) p[threadIdx.x] = val;
        if (t0 + threadIdx.x < count) p[t0 + threadIdx.x] = val;
    }
}

// --------------------------------------------------------------------------- production kernel
// hist: uint32 [2][T][n]: [0] = infection events (t = 0 for seeds), [1] = recovery events.
#ifndef GN_SIR_UNROLL
#define GN_SIR_UNROLL 8
#endif
template <bool STATE_IN_LDS, bool NODES, bool TRAJ, bool EDGES = false, bool INIT = false, bool SCHED = false, class OUT = SirNoSweep>
__global__ __launch_bounds__(1024) void k_sir_philox(const int* __restrict__ src, const int* __restrict__ dst, long nnz,
                                                    int n, const int* __restrict__ seeds, int n_seeds,
                                                    SirThr<NODES> thr_beta, SirThr<NODES> thr_gamma,
                                                    long sims, long sim_offset, int T, uint32_t k0, uint32_t k1,
                                                    uint32_t* __restrict__ hist, uint8_t* __restrict__ gstate, SirTraj<TRAJ> tr,
                                                    SirInit<INIT> in, SirSched<SCHED> sc_call, typename OUT::Jobs sw, OUT outp) {
    static_assert(NODES || !EDGES, "per-edge infection thresholds come with per-node recovery thresholds");
    static_assert(EDGES || !SCHED, "a schedule switches per-edge tables");
    static_assert(!OUT::SWEEP || (INIT && SCHED && !TRAJ), "the sweep overrides a drawn start and shifts a schedule; its output is its policy's");
    constexpr bool SWEEP = OUT::SWEEP, TALLY = TRAJ || OUT::ROWS;   // TALLY: the trajectory's totals are kept in tcnt
    extern __shared__ uint8_t smem[];
    uint8_t* state = STATE_IN_LDS ? smem : gstate + (size_t)blockIdx.x * 2 * n;
    uint8_t* flag = state + n;
    uint32_t* hinf = hist;
    uint32_t* hrec = hist + (size_t)T * n;
    const int nthr = blockDim.x;                  // 256 for small graphs, 1024 when the LDS state allows one workgroup per CU
    // TRAJ: the scan has no counters of its own -- [0] ever infected, [1] recovered, of the trajectory in hand (static LDS:
    // the dynamic size is what the host's occupancy choice is computed from)
    __shared__ int tcnt[2];
    __shared__ int olds[OUT::LDS_INTS ? OUT::LDS_INTS : 1];      // the output policy's; a policy without LDS never names it
    const auto state_of = [&](int v) -> int { return (int)state[v]; };
    int16_t* ev_inf = nullptr; int16_t* ev_rec = nullptr; uint32_t* curves = nullptr;
    if constexpr (TRAJ) { ev_inf = tr.events; if (tr.events) ev_rec = tr.events + (size_t)sims * n; curves = tr.curves; }
    long jobs = sims;                             // (SWEEP) C * sims of them, the candidates interleaved
    if constexpr (SWEEP) jobs = sims * sw.C;
    for (long job = blockIdx.x; job < jobs; job += gridDim.x) {
        long s = job; int cj = 0, cnode = -1, cact = 0;                 // (SWEEP) the candidate, its node and action
        if constexpr (SWEEP) { sir_sweep_job(job, sw.C, sims, cj, s); cnode = sw.cand[cj]; if (cnode >= n) cnode = -1; cact = sw.action; }
        typename OUT::Job jb;
        const SirSched<SCHED> sc = sir_job_sched<SWEEP>(sc_call, sw, cj);
        const uint32_t sim = (uint32_t)(sim_offset + s);
        for (int v = threadIdx.x; v < n; v += nthr) { state[v] = ST_S; flag[v] = 0; }
        if (TALLY && threadIdx.x < 2) tcnt[threadIdx.x] = 0;
        outp.reset(olds, T, (int)threadIdx.x, nthr);
        __syncthreads();
        if constexpr (INIT) {
            // drawn start: a node that starts in I or R has left S at step 0 (one infection event), one that starts in R
            // has recovered at step 0 as well
            int n_out = 0, n_gone = 0;
            for (int q = threadIdx.x; 4 * q < n; q += nthr) {
                uint32_t inf, rec;
                sir_start_quad<SWEEP>(in.thr, n, q, sim, k0, k1, cnode, cact, inf, rec);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int v = 4 * q + j;
                    if (!(((inf | rec) >> j) & 1u)) continue;
                    const bool r = (rec >> j) & 1u;
                    state[v] = r ? ST_R : ST_I;
                    sir_hist_add<SWEEP>(&hinf[v]); outp.template event<0>(olds, T, v, 0);
                    if (r) { sir_hist_add<SWEEP>(&hrec[v]); outp.template event<1>(olds, T, v, 0); }
                    if (TRAJ && ev_inf) { ev_inf[(size_t)s * n + v] = 0; if (r) ev_rec[(size_t)s * n + v] = 0; }
                }
                n_out += __popc(inf | rec); n_gone += __popc(rec);
            }
            if (TALLY && n_out) atomicAdd(&tcnt[0], n_out);
            if (TALLY && n_gone) atomicAdd(&tcnt[1], n_gone);
        } else {
            for (int j = threadIdx.x; j < n_seeds; j += nthr) state[seeds[j]] = ST_I;   // duplicates: same value
        }
        __syncthreads();
        for (int j = threadIdx.x; j < n_seeds; j += nthr) {
            // one infection event at t=0 per distinct seed node
            const int v = seeds[j];
            bool first = true;
            for (int q = 0; q < j; ++q) first = first && (seeds[q] != v);
            if (first) {
                sir_hist_add<SWEEP>(&hinf[v]);
                if (TRAJ) atomicAdd(&tcnt[0], 1);
                if (TRAJ && ev_inf) ev_inf[(size_t)s * n + v] = 0;
            }
        }
        int rows_done = 1;                          // (TRAJ, SWEEP) rows of `curves` / of the sums written so far
        const bool rows = OUT::ROWS || (TRAJ && curves);
        int t_end = outp.steps(T);
        if constexpr (OUT::CLOSES) if (!outp.closed(jb, olds, sw, cj, 0, n, (int)threadIdx.x, nthr, state_of)) t_end = 0;   // (the start is step 0, closed by the barrier above)
        if (rows) {
            __syncthreads();
            if constexpr (SWEEP) outp.row(jb, olds, sw, cj, T, 0, n, tcnt[0], tcnt[1], (int)threadIdx.x); else
            if (threadIdx.x == 0) sir_curve_row(curves, s, T, 0, n, tcnt[0], INIT ? tcnt[1] : 0);
        }
        for (int it = 1; it < t_end; ++it) {
            const SirThr<NODES> tb_step = sir_step_thr<NODES>(thr_beta, sc, it, (size_t)nnz), tg_step = sir_step_thr<NODES>(thr_gamma, sc, it, (size_t)n);
            // GN_SIR_UNROLL source ids in flight per thread: the scan is a chain of (global id load -> LDS state read)
            // pairs, latency-bound when issued one at a time.  Wiki-vote-size graph, 10 000 sims x T = 20: 38.8 ms at 1,
            // 25.9 ms at 4, 23.6 ms at 8.  Tried on top, no gain: 16-bit ids (23.4 ms: not bound by the id bytes); four
            // consecutive edges per lane sharing one Philox block (32.5 ms: a wave then spans ~9 rows instead of ~2 and
            // runs mostly half-empty).
#define GN_EDGE(ON, E)                                                                                        \
                if (ON) {                                                                                     \
                    const int v = dst[E];                                                                     \
                    if (state[v] == ST_S &&                                                                   \
                        (unsigned long long)philox_coin((uint32_t)(E), (uint32_t)it, sim, 0u, k0, k1) < sir_thr(tb_step, EDGES ? (int)(E) : v)) \
                        flag[v] = 1;                                                                          \
                }
            long e = threadIdx.x;
            for (; e + (long)(GN_SIR_UNROLL - 1) * nthr < nnz; e += (long)GN_SIR_UNROLL * nthr) {
                int u[GN_SIR_UNROLL]; bool inf[GN_SIR_UNROLL];
#pragma unroll
                for (int q = 0; q < GN_SIR_UNROLL; ++q) u[q] = src[e + (long)q * nthr];
#pragma unroll
                for (int q = 0; q < GN_SIR_UNROLL; ++q) inf[q] = state[u[q]] == ST_I;
#pragma unroll
                for (int q = 0; q < GN_SIR_UNROLL; ++q) GN_EDGE(inf[q], e + (long)q * nthr)
            }
            for (; e < nnz; e += nthr) {
                const bool i0 = state[src[e]] == ST_I;
                GN_EDGE(i0, e)
            }
#undef GN_EDGE
            for (int u = threadIdx.x; u < n; u += nthr)
                if (state[u] == ST_I &&
                    (unsigned long long)philox_coin((uint32_t)u, (uint32_t)it, sim, 1u, k0, k1) < sir_thr(tg_step, u))
                    flag[u] = 2;
            __syncthreads();
            int any = 0, n_new = 0, n_gone = 0;
            for (int v = threadIdx.x; v < n; v += nthr) {
                const uint8_t f = flag[v];
                if (f == 1) {
                    state[v] = ST_I; sir_hist_add<SWEEP>(&hinf[(size_t)it * n + v]); outp.template event<0>(olds, T, v, it);
                    if (TALLY) ++n_new;
                    if (TRAJ && ev_inf) ev_inf[(size_t)s * n + v] = (int16_t)it;
                } else if (f == 2) {
                    state[v] = ST_R; sir_hist_add<SWEEP>(&hrec[(size_t)it * n + v]); outp.template event<1>(olds, T, v, it);
                    if (TALLY) ++n_gone;
                    if (TRAJ && ev_inf) ev_rec[(size_t)s * n + v] = (int16_t)it;
                }
                flag[v] = 0;
                any |= (state[v] == ST_I);
            }
            if (TALLY && n_new) atomicAdd(&tcnt[0], n_new);
            if (TALLY && n_gone) atomicAdd(&tcnt[1], n_gone);
            const int alive = __syncthreads_or(any);
            if (rows) {                             // (the counters rest until the next step's barrier)
                if constexpr (SWEEP) outp.row(jb, olds, sw, cj, T, it, n, tcnt[0], tcnt[1], (int)threadIdx.x); else
                if (threadIdx.x == 0) sir_curve_row(curves, s, T, it, n, tcnt[0], tcnt[1]);
                rows_done = it + 1;
            }
            // (the next step writes flag[] alone until its own barrier: the state rests)
            if constexpr (OUT::CLOSES) if (!outp.closed(jb, olds, sw, cj, it, n, (int)threadIdx.x, nthr, state_of)) break;
            if (!alive) break;                      // epidemic over: no further events in this trajectory
        }
        if constexpr (SWEEP) {                      // (every event lies behind a barrier)
            outp.finish(jb, olds, sw, cj, s, sims, T, rows_done, n, OUT::ROWS ? tcnt[0] : 0, OUT::ROWS ? tcnt[1] : 0, (int)threadIdx.x, nthr, state_of);
        } else if (rows) {                          // the rows after an early end repeat the final state
            const int n_ever = tcnt[0], n_rec = tcnt[1];
            for (int r = rows_done + threadIdx.x; r < T; r += nthr) sir_curve_row(curves, s, T, r, n, n_ever, n_rec);
        }
        __syncthreads();
    }
}

// --------------------------------------------------------------------------- frontier-driven kernel
// LDS: ever-infected bitmap (n bits) and, when they fit (uint16 ids: n up to 11 232 for a graph without rows longer than
// GN_SIR_BIGROW, frontier_lists_in_lds), the node lists: current / next frontier and the rows too long for
// one lane group.  Larger graphs keep the three lists in the caller's workspace (int32 ids, one set per workgroup).
// GN_SIR_BIGROW (gnode_common.h): rows longer than this are walked by the whole workgroup
// COUNT: the profiling instantiation (gnode_sir_mc_philox_counted) also tallies Philox blocks, coins and CSR entries read.
// NODES: per-node thresholds.  A target's threshold is read only where a coin is drawn -- in `drain`, for the (position,
// target) pairs that passed the ever-infected test -- and the read is issued ahead of the coin's Philox rounds.
// EDGES (with NODES): the infection threshold is read at the queued CSR position instead of the queued target -- the queue
// already carries both, for every path into it (lane-group rows and the whole-workgroup walk of hub rows alike).  `spent`
// and the recovery-only phase ask only whether a target is susceptible, so both stay sufficient next to w = 0 entries: a row
// whose susceptible targets all sit behind zeros keeps being walked.  There is no COUNT && EDGES instance.
// TRAJ: per-trajectory events and curves (SirTraj above); there is no COUNT && TRAJ instance.
// OUT: the candidate sweep's output policy (gnode_sir_sweep.h): jobs instead of trajectories, its output instead of histograms.
template <typename IdT, bool LISTS_IN_LDS, bool COUNT, bool NODES, bool TRAJ, bool EDGES = false, bool INIT = false, bool SCHED = false,
          class OUT = SirNoSweep>
__global__ __launch_bounds__(1024) void k_sir_frontier(const int* __restrict__ rowptr, const int* __restrict__ col, int n,
                                                      const int* __restrict__ seeds, int n_seeds,
                                                      SirThr<NODES> thr_beta, SirThr<NODES> thr_gamma,
                                                      long sims, long sim_offset, int T, uint32_t k0, uint32_t k1,
                                                      uint32_t* __restrict__ hist, int32_t* __restrict__ glists,
                                                      unsigned long long* __restrict__ stats, SirTraj<TRAJ> tr, SirInit<INIT> in,
                                                      SirSched<SCHED> sc_call, typename OUT::Jobs sw, OUT outp) {
    constexpr bool SWEEP = OUT::SWEEP;
    static_assert(!SWEEP || (INIT && SCHED && !TRAJ), "the sweep overrides a drawn start and shifts a schedule; its output is its policy's");
    static_assert(!(COUNT && INIT), "the counting instantiation starts from a seed list");
    static_assert(EDGES || !SCHED, "a schedule switches per-edge tables");
    static_assert(!(COUNT && TRAJ), "the counting instantiation has no per-trajectory output");
    static_assert(!(COUNT && EDGES) && (NODES || !EDGES), "per-edge thresholds: with per-node recovery, never counted");
    extern __shared__ uint32_t smem_w[];
    const int nwords = (n + 31) >> 5;
    const int nw4 = (nwords + 3) & ~3;
    uint32_t* bits = smem_w;                                   // ever infected (seeds included): susceptible <=> bit clear
    uint32_t* spent = smem_w + nw4;                            // node whose neighbours have ALL been infected: its row can never
                                                               // infect anybody again (infection is monotone) and is not walked any more
    uint32_t* recb = smem_w + 2 * nw4;                         // recovered
    // per-wave queue of (CSR position, target) pairs whose target was susceptible: their coins are drawn 64 at a time (below)
    int* const cq = reinterpret_cast<int*>(smem_w + 3 * nw4) + (threadIdx.x >> 6) * 256;       // 128 positions | 128 targets
    uint32_t* const after_q = smem_w + 3 * nw4 + (blockDim.x >> 6) * 256;
    IdT* lists = LISTS_IN_LDS ? reinterpret_cast<IdT*>(after_q)
                              : reinterpret_cast<IdT*>(glists + (size_t)blockIdx.x * 3 * n);
    IdT* cur = lists;
    IdT* nxt = lists + n;
    IdT* big = lists + 2 * (size_t)n;                          // [rows longer than GN_SIR_BIGROW in the graph] (LDS form), [n] (workspace form)
    __shared__ int cnt[3];                                     // [0] next-list length, [1] big-row list length, [2] ever infected
    __shared__ int olds[OUT::LDS_INTS ? OUT::LDS_INTS : 1];    // the output policy's; a policy without LDS never names it
    const auto state_of = [&](int v) -> int {                  // S / I / R of node v off the two bitmaps
        const uint32_t m = 1u << (v & 31);
        return (bits[v >> 5] & m) ? ((recb[v >> 5] & m) ? 2 : 1) : 0;
    };
    uint32_t* hinf = hist;
    uint32_t* hrec = hist + (size_t)T * n;
    const int nthr = blockDim.x, tid = threadIdx.x;
    const int sub = tid & 15, gid = tid >> 4, ngroups = nthr >> 4, lane_in_wave = tid & 63;
    unsigned long long st_blocks = 0, st_ecoins = 0, st_rcoins = 0, st_entries = 0;
    int16_t* ev_inf = nullptr; int16_t* ev_rec = nullptr; uint32_t* curves = nullptr;
    if constexpr (TRAJ) { ev_inf = tr.events; if (tr.events) ev_rec = tr.events + (size_t)sims * n; curves = tr.curves; }
    size_t sched_nnz = 0;                                      // (SCHED) the length of one infection table
    if constexpr (SCHED) sched_nnz = (size_t)rowptr[n];
    long jobs = sims;                                          // (SWEEP) C * sims of them, the candidates interleaved
    if constexpr (SWEEP) jobs = sims * sw.C;
    for (long job = blockIdx.x; job < jobs; job += gridDim.x) {
        long s = job; int cj = 0, cnode = -1, cact = 0;        // (SWEEP) the candidate, its node and action
        if constexpr (SWEEP) { sir_sweep_job(job, sw.C, sims, cj, s); cnode = sw.cand[cj]; if (cnode >= n) cnode = -1; cact = sw.action; }
        typename OUT::Job jb;
        const SirSched<SCHED> sc = sir_job_sched<SWEEP>(sc_call, sw, cj);
        const uint32_t sim = (uint32_t)(sim_offset + s);
        for (int w = tid; w < nwords; w += nthr) { bits[w] = 0u; spent[w] = 0u; recb[w] = 0u; }
        if (tid < 3) cnt[tid] = 0;
        outp.reset(olds, T, tid, nthr);
        __syncthreads();
        if constexpr (INIT) {
            // drawn start (sir_init_draw): I and R starts have left S (ever-infected bit, one infection event at t = 0), R
            // starts have recovered too (recb, one recovery event at t = 0), I starts make the first frontier -- which may be a
            // large share of n, so the list grows by ONE LDS atomic per wave, as the survivors' append does.  Every lane of the
            // workgroup runs every iteration: the ballots need whole waves.
            const int nq = (n + 3) >> 2;
            for (int q0 = 0; q0 < nq; q0 += nthr) {
                const int q = q0 + tid, u0 = 4 * q;
                uint32_t inf = 0, rec = 0;
                if (q < nq) sir_start_quad<SWEEP>(in.thr, n, q, sim, k0, k1, cnode, cact, inf, rec);
                const uint32_t out = inf | rec;
                if (out) atomicOr(&bits[u0 >> 5], out << (u0 & 31));
                if (rec) atomicOr(&recb[u0 >> 5], rec << (u0 & 31));
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((out >> j) & 1u) {
                        const bool r = (rec >> j) & 1u;
                        sir_hist_add<SWEEP>(&hinf[u0 + j]); outp.template event<0>(olds, T, u0 + j, 0);
                        if (r) { sir_hist_add<SWEEP>(&hrec[u0 + j]); outp.template event<1>(olds, T, u0 + j, 0); }
                        if (TRAJ && ev_inf) { ev_inf[(size_t)s * n + u0 + j] = 0; if (r) ev_rec[(size_t)s * n + u0 + j] = 0; }
                    }
                // this wave's I starts: slot = wave base + the I starts of the lanes below + this lane's own in front
                const unsigned long long below = (1ull << lane_in_wave) - 1ull;
                int before = 0, n_i = 0, n_out = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const unsigned long long mi = __ballot((inf >> j) & 1u);
                    before += __popcll(mi & below); n_i += __popcll(mi);
                    n_out += __popcll(__ballot((out >> j) & 1u));
                }
                int basep = 0;
                if (lane_in_wave == 0 && n_out) { basep = atomicAdd(&cnt[0], n_i); atomicAdd(&cnt[2], n_out); }
                basep = __shfl(basep, 0, 64) + before;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((inf >> j) & 1u) cur[basep++] = (IdT)(u0 + j);
            }
        } else {
            for (int j = tid; j < n_seeds; j += nthr) {        // distinct seeds: one infection event at t = 0 each
                const int v = seeds[j];
                const uint32_t m = 1u << (v & 31);
                if (!(atomicOr(&bits[v >> 5], m) & m)) {
                    cur[atomicAdd(&cnt[0], 1)] = (IdT)v; atomicAdd(&hinf[v], 1u);
                    if (TRAJ && ev_inf) ev_inf[(size_t)s * n + v] = 0;
                }
            }
        }
        __syncthreads();
        int n_inf = cnt[0];
        int n_ever = INIT ? cnt[2] : n_inf;                // once it reaches n nobody is left to infect: recovery coins only
        __syncthreads();
        if (tid == 0) cnt[2] = n_ever;
        int rows_done = 1;                                     // (TRAJ, SWEEP) rows of `curves` / of the sums written so far
        const bool rows = OUT::ROWS || (TRAJ && curves);
        int t_end = outp.steps(T);
        // (the start is step 0, closed by the barriers above; the first step's writes lie behind its own)
        if constexpr (OUT::CLOSES) if (!outp.closed(jb, olds, sw, cj, 0, n, tid, nthr, state_of)) t_end = 0;
        if constexpr (SWEEP) outp.row(jb, olds, sw, cj, T, 0, n, n_ever, n_ever - n_inf, tid); else
        if (rows && tid == 0) sir_curve_row(curves, s, T, 0, n, n_ever, INIT ? n_ever - n_inf : 0);
        for (int it = 1; it < t_end && n_inf > 0; ++it) {
            // this step's tables: drain, the recovery loop and the recovery-only branch read nothing else
            const SirThr<NODES> tb_step = sir_step_thr<NODES>(thr_beta, sc, it, sched_nnz), tg_step = sir_step_thr<NODES>(thr_gamma, sc, it, (size_t)n);
            if (tid == 0) { cnt[0] = 0; cnt[1] = 0; }
            __syncthreads();
#ifndef GN_SIR_MODEB
#define GN_SIR_MODEB 1
#endif
            if (GN_SIR_MODEB && n_ever >= n) {
                // ---- everybody has been infected: only recovery coins remain, and the infected set is "not recovered".  No
                // lists: a thread takes four consecutive nodes = ONE Philox block
                int alive = 0;
                for (int q = tid; 4 * q < n; q += nthr) {
                    const int u0 = 4 * q;
                    uint32_t nib = (~recb[u0 >> 5] >> (u0 & 31)) & 0xFu;
                    if (u0 + 4 > n) nib &= (1u << (n - u0)) - 1u;
                    if (!nib) continue;
                    uint32_t w[4];
                    philox_block((uint32_t)q, (uint32_t)it, sim, 1u, k0, k1, w);
                    if (COUNT) { ++st_blocks; st_rcoins += __popc(nib); }
                    uint32_t gone = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if ((nib >> j) & 1u) {
                            if ((unsigned long long)w[j] < sir_thr(tg_step, u0 + j)) {
                                gone |= 1u << j; sir_hist_add<SWEEP>(&hrec[(size_t)it * n + u0 + j]); outp.template event<1>(olds, T, u0 + j, it);
                                if (TRAJ && ev_inf) ev_rec[(size_t)s * n + u0 + j] = (int16_t)it;
                            } else ++alive;
                        }
                    if (gone) atomicOr(&recb[u0 >> 5], gone << (u0 & 31));
                }
                if (alive) atomicAdd(&cnt[0], alive);
                __syncthreads();
                n_inf = cnt[0];
                if (rows) {
                    n_ever = n;
                    if constexpr (SWEEP) outp.row(jb, olds, sw, cj, T, it, n, n_ever, n_ever - n_inf, tid); else
                    if (tid == 0) sir_curve_row(curves, s, T, it, n, n_ever, n_ever - n_inf);
                    rows_done = it + 1;
                }
                __syncthreads();
                if constexpr (OUT::CLOSES) if (!outp.closed(jb, olds, sw, cj, it, n, tid, nthr, state_of)) break;
                continue;
            }
            // infection attempts along the out-edges of the frontier: one 16-lane group per infected node, a lane takes
            // FOUR consecutive CSR positions (an aligned quad: one 16-byte read of the column list, one Philox block)
            auto infect = [&](int v) {
                const uint32_t m = 1u << (v & 31);
                if (!(atomicOr(&bits[v >> 5], m) & m)) {       // first edge to reach v this step (it was susceptible)
                    nxt[atomicAdd(&cnt[0], 1)] = (IdT)v;
                    atomicAdd(&cnt[2], 1);
                    sir_hist_add<SWEEP>(&hinf[(size_t)it * n + v]); outp.template event<0>(olds, T, v, it);
                    if (TRAJ && ev_inf) ev_inf[(size_t)s * n + v] = (int16_t)it;
                }
            };
            // Counted on the wiki-vote-size workload (beta 0.3): 2.6e9 CSR entries read, 0.24e9 of them with a susceptible target.
            // A coin drawn where it is found runs the ~60-instruction Philox sequence for the WHOLE wave whenever any of its 64
            // lanes needs one -- almost always, at 9 % of the lanes: the kernel issued 4.7e9 vector instructions, two per CSR
            // entry, ~40 % of the chip's issue rate, nearly all of it Philox on idle lanes.  So susceptible (position, target)
            // pairs go through a per-wave LDS queue and their coins are drawn 64 at a time.  A target may now be queued by
            // several rows before the first coin infects it; the extra coins change nothing (infection = OR over the coins of
            // the edges whose target was susceptible at the start of the step, exactly the reference's rule).
            int qn = 0;                                        // wave-uniform queue length
            auto drain = [&](int take) {                       // the last `take` (<= 64) queued pairs
                const int slot = qn - take + lane_in_wave;
                if (lane_in_wave < take) {
                    const int e = cq[slot], v = cq[128 + slot];
                    if (COUNT) { ++st_blocks; ++st_ecoins; }
                    const unsigned long long tb = sir_thr(tb_step, EDGES ? e : v);
                    if ((unsigned long long)philox_coin((uint32_t)e, (uint32_t)it, sim, 0u, k0, k1) < tb) infect(v);
                }
                qn -= take;
            };
            auto push = [&](bool sus, int e, int v) {          // every lane of the wave calls it (sus = false: nothing to add)
                const unsigned long long mk = __ballot(sus);
                if (sus) { const int slot = qn + __popcll(mk & ((1ull << lane_in_wave) - 1ull)); cq[slot] = e; cq[128 + slot] = v; }
                qn += __popcll(mk);
                __builtin_amdgcn_wave_barrier();
                if (qn >= 64) drain(64);
            };
            auto try_edge = [&](int e, bool on) -> bool {      // one lane per CSR position; `on`: this lane has an entry
                const int v = on ? col[e] : 0;
                const bool sus = on && !(bits[v >> 5] & (1u << (v & 31)));
                if (COUNT && on) ++st_entries;
                push(sus, e, v);
                return sus;
            };
            // The walk of one frontier row is a chain of dependent loads (list entry -> row extent -> column ids -> bitmap), ~2 us
            // of L2 round trips for a few dozen integer instructions: counted, the wiki-vote-size workload reads 2.8e9 CSR
            // entries and draws 0.58e9 coins in 10 ms, an order of magnitude below both the integer and the L2 rate --
            // it was LATENCY bound, one row per lane group at a time.  So the rows are software-pipelined three deep per lane
            // group: while row i is tested, the column ids of row i+1 and the extent of row i+2 are in flight.
            struct Row { int u, lo, hi, ca, cb; };
            Row r1 = {-1, 0, 0, 0, 0}, r2 = {-1, 0, 0, 0, 0};
            for (int idx = gid; __any(idx < n_inf + 2 * ngroups); idx += ngroups) {
                // stage A: the next row's node and extent
                Row r0 = {-1, 0, 0, 0, 0};
                if (idx < n_inf) {
                    const int u = (int)cur[idx];
                    if (!(spent[u >> 5] & (1u << (u & 31)))) { r0.u = u; r0.lo = rowptr[u]; r0.hi = rowptr[u + 1]; }   // (spent: nothing left to do for u)
                }
                // stage B: column ids 0..31 of the row fetched one iteration ago (rows for the whole workgroup go on `big`)
                if (r1.u >= 0) {
                    if (r1.hi - r1.lo > GN_SIR_BIGROW) { if (sub == 0) big[atomicAdd(&cnt[1], 1)] = (IdT)r1.u; r1.u = -1; }
                    else {
                        if (r1.lo + sub < r1.hi) r1.ca = col[r1.lo + sub];
                        if (r1.lo + 16 + sub < r1.hi) r1.cb = col[r1.lo + 16 + sub];
                    }
                }
                // stage C: test the row whose column ids were requested one iteration ago (wave-uniform control flow: the
                // queue's ballots need every lane)
                {
                    bool any_sus = false;
                    auto test = [&](bool on, int e, int v) {
                        const bool sus = on && !(bits[v >> 5] & (1u << (v & 31)));
                        if (COUNT && on) ++st_entries;
                        push(sus, e, v);
                        any_sus |= sus;
                    };
                    const bool live = r2.u >= 0;
                    test(live && r2.lo + sub < r2.hi, r2.lo + sub, r2.ca);
                    if (__any(live && r2.hi - r2.lo > 16)) test(live && r2.lo + 16 + sub < r2.hi, r2.lo + 16 + sub, r2.cb);
                    for (int e0 = 32; __any(live && r2.lo + e0 < r2.hi); e0 += 16) {
                        const int e = r2.lo + e0 + sub;
                        const bool on = live && e < r2.hi;
                        test(on, e, on ? col[e] : 0);
                    }
                    // (a target infected during this very walk still counted as susceptible: the row is retired one step later)
                    const unsigned long long bal = __ballot(any_sus);
                    if (live && sub == 0 && !((bal >> (lane_in_wave & 48)) & 0xFFFFull)) atomicOr(&spent[r2.u >> 5], 1u << (r2.u & 31));
                }
                r2 = r1; r1 = r0;
            }
            if (qn > 0) drain(qn);
            // recovery coin of every node of the frontier (decided on the pre-step state: a node infected in this step is
            // not on `cur`); survivors go on the next list
            for (int idx = tid; idx < n_inf; idx += nthr) {
                const int u = (int)cur[idx];
                if (COUNT) { ++st_blocks; ++st_rcoins; }
                const unsigned long long tg = sir_thr(tg_step, u);
                const bool gone = (unsigned long long)philox_coin((uint32_t)u, (uint32_t)it, sim, 1u, k0, k1) < tg;
                if (gone) {
                    sir_hist_add<SWEEP>(&hrec[(size_t)it * n + u]); outp.template event<1>(olds, T, u, it);
                    if (TRAJ && ev_inf) ev_rec[(size_t)s * n + u] = (int16_t)it;
                    atomicOr(&recb[u >> 5], 1u << (u & 31));
                }
                // survivors go on the next list: ONE LDS atomic per wave (64 lanes adding to the same word serialise)
                const unsigned long long keep = __ballot(!gone);
                int basep = 0;
                if (lane_in_wave == 0 && keep) basep = atomicAdd(&cnt[0], __popcll(keep));
                basep = __shfl(basep, 0, 64);
                if (!gone) nxt[basep + __popcll(keep & ((1ull << lane_in_wave) - 1ull))] = (IdT)u;
            }
            __syncthreads();
            const int n_big = cnt[1];
            for (int b = 0; b < n_big; ++b) {                   // hub rows: the whole workgroup strides one row
                const int u = (int)big[b];
                const int lo = rowptr[u], hi = rowptr[u + 1];
                for (int e0 = lo; e0 < hi; e0 += nthr) try_edge(e0 + tid, e0 + tid < hi);
                if (qn > 0) drain(qn);
            }
            __syncthreads();
            n_inf = cnt[0];
            n_ever = cnt[2];
            if (rows) {
                if constexpr (SWEEP) outp.row(jb, olds, sw, cj, T, it, n, n_ever, n_ever - n_inf, tid); else
                if (tid == 0) sir_curve_row(curves, s, T, it, n, n_ever, n_ever - n_inf);
                rows_done = it + 1;
            }
            IdT* t = cur; cur = nxt; nxt = t;
            __syncthreads();
            // the next step's first write to a bitmap lies behind its own barrier: a walk of the nodes reads a state at rest
            if constexpr (OUT::CLOSES) if (!outp.closed(jb, olds, sw, cj, it, n, tid, nthr, state_of)) break;
        }
        if constexpr (SWEEP) {
            // (every step ends in a barrier, and so does the start: every event lies behind one)
            outp.finish(jb, olds, sw, cj, s, sims, T, rows_done, n, n_ever, n_ever - n_inf, tid, nthr, state_of);
            if constexpr (OUT::LDS_AT_END) __syncthreads();    // the next job resets the policy's LDS behind this
        } else if (rows) {                                     // the rows after an early end repeat the final state
            for (int r = rows_done + tid; r < T; r += nthr) sir_curve_row(curves, s, T, r, n, n_ever, n_ever - n_inf);
        }
    }
    if (COUNT) {
        atomicAdd(&stats[0], st_blocks); atomicAdd(&stats[1], st_ecoins); atomicAdd(&stats[2], st_rcoins); atomicAdd(&stats[3], st_entries);
    }
}

// counts[0..2][t][v] += (sims - cumInf, cumInf - cumRec, cumRec) for t >= 1; row 0 assigned -- or, ACC0 (a drawn start:
// the trajectories do not share one initial state), accumulated like the others from the events of step 0.
template <bool ACC0>
__global__ __launch_bounds__(256) void k_sir_finalize(const uint32_t* __restrict__ hist, int n, int T, uint32_t sims,
                                                      uint32_t* __restrict__ counts) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const uint32_t* hinf = hist;
    const uint32_t* hrec = hist + (size_t)T * n;
    const size_t plane = (size_t)T * n;
    uint32_t ci = hinf[v], cr = 0;
    if constexpr (ACC0) {
        cr = hrec[v];
        counts[v] += sims - ci; counts[plane + v] += ci - cr; counts[2 * plane + v] += cr;
    } else {
        const uint32_t seeded = ci ? 1u : 0u;        // every trajectory starts from the same seed set
        counts[v] = 1u - seeded;                     // S row 0: assigned, ode_nn.py:56
        counts[plane + v] = seeded;                  // I row 0: assigned, ode_nn.py:55
        ci = seeded * sims;
    }
    for (int t = 1; t < T; ++t) {
        ci += hinf[(size_t)t * n + v];
        cr += hrec[(size_t)t * n + v];
        counts[(size_t)t * n + v] += sims - ci;
        counts[plane + (size_t)t * n + v] += ci - cr;
        counts[2 * plane + (size_t)t * n + v] += cr;
    }
}

// --------------------------------------------------------------------------- parity kernel (recorded coin stream)
__device__ __forceinline__ int block_rank(bool pred, int* wave_tot, int& total) {
    // stable exclusive rank of `pred` lanes over the 256-thread block
    const unsigned long long m = __ballot(pred);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) wave_tot[w] = __popcll(m);
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) { const int c = wave_tot[q]; base += (q < w) ? c : 0; total += c; }
    return base + r;
}

__global__ __launch_bounds__(256) void k_sir_coins(const int* __restrict__ tsrc, const int* __restrict__ tdst, long nt,
                                                   int n, const int* __restrict__ seeds, int n_seeds, double beta,
                                                   double gamma, long sims, int T, const double* __restrict__ coins,
                                                   long n_coins, uint32_t* __restrict__ counts,
                                                   long long* __restrict__ used) {
    extern __shared__ uint8_t smem[];
    uint8_t* state = smem;
    uint8_t* flag = smem + n;
    __shared__ int wave_tot[4];
    const size_t plane = (size_t)T * n;
    long pos = 0;
    bool overrun = false;
    for (long s = 0; s < sims; ++s) {
        for (int v = threadIdx.x; v < n; v += 256) { state[v] = ST_S; flag[v] = 0; }
        __syncthreads();
        for (int j = threadIdx.x; j < n_seeds; j += 256) state[seeds[j]] = ST_I;
        __syncthreads();
        for (int v = threadIdx.x; v < n; v += 256) {          // row 0 assigned each sim (ode_nn.py:55-56)
            counts[v] = state[v] == ST_S;
            counts[plane + v] = state[v] == ST_I;
        }
        for (int it = 1; it < T; ++it) {
            // coins #1: one per active table row, in table order (ode_nn.py:61-67)
            for (long e0 = 0; e0 < nt; e0 += 256) {
                const long e = e0 + threadIdx.x;
                int v = 0;
                bool act = false;
                if (e < nt) { v = tdst[e]; act = state[tsrc[e]] == ST_I && state[v] == ST_S; }
                int total;
                const int rk = block_rank(act, wave_tot, total);
                if (act) {
                    const long ci = pos + rk;
                    if (ci < n_coins) { if (coins[ci] < beta) flag[v] = 1; } else overrun = true;
                }
                pos += total;
            }
            __syncthreads();
            // coins #2: one per infected node, ascending id (ode_nn.py:70-72)
            for (int u0 = 0; u0 < n; u0 += 256) {
                const int u = u0 + threadIdx.x;
                const bool inf = u < n && state[u] == ST_I;
                int total;
                const int rk = block_rank(inf, wave_tot, total);
                if (inf) {
                    const long ci = pos + rk;
                    if (ci < n_coins) { if (coins[ci] < gamma) flag[u] = 2; } else overrun = true;
                }
                pos += total;
            }
            __syncthreads();
            for (int v = threadIdx.x; v < n; v += 256) {
                const uint8_t f = flag[v];
                if (f == 1) state[v] = ST_I; else if (f == 2) state[v] = ST_R;
                flag[v] = 0;
                const uint8_t st = state[v];
                counts[(size_t)it * n + v] += st == ST_S;
                counts[plane + (size_t)it * n + v] += st == ST_I;
                counts[2 * plane + (size_t)it * n + v] += st == ST_R;
            }
            __syncthreads();
        }
    }
    if (__syncthreads_or(overrun)) pos = -1;
    if (threadIdx.x == 0) *used = pos;
}

// --------------------------------------------------------------------------- host side
// Layout, path selection, geometry and staging are gnode_sir_plan.{h,cpp}; here: the kernel instances and the calls.
struct SeedArg { int32_t v[32]; };
__global__ void k_put_seeds(SeedArg sa, int n_seeds, int32_t* __restrict__ seeds) {
    if ((int)threadIdx.x < n_seeds) seeds[threadIdx.x] = sa.v[threadIdx.x];
}

// The kernels one form of call can launch, by path (SirPath): RATES is SIR_SCALAR / SIR_NODES / SIR_EDGES.  The launch and the
// registration below both go through sir_dispatch, so an instance cannot be launched without being registered.
// SCHED_: the four scheduled forms (per-edge rates only, TRAJ x INIT), reached through sir_dispatch_sched.
// OUT: the candidate sweep, one form per output policy (the drawn-start scheduled one without per-trajectory output), through
// sir_dispatch_sweep<OUT>.
template <int RATES, bool TRAJ_, bool INIT_, bool SCHED_ = false, class OUT = SirNoSweep>
struct SirKernels {
    static constexpr bool NODES = RATES >= SIR_NODES, EDGES = RATES == SIR_EDGES, TRAJ = TRAJ_, INIT = INIT_, SCHED = SCHED_;
    static constexpr auto frontier_lds = &k_sir_frontier<uint16_t, true, false, NODES, TRAJ, EDGES, INIT, SCHED, OUT>;
    static constexpr auto frontier_mem = &k_sir_frontier<int32_t, false, false, NODES, TRAJ, EDGES, INIT, SCHED, OUT>;
    static constexpr auto scan_lds = &k_sir_philox<true, NODES, TRAJ, EDGES, INIT, SCHED, OUT>;
    static constexpr auto scan_mem = &k_sir_philox<false, NODES, TRAJ, EDGES, INIT, SCHED, OUT>;
};
// the counting instances (gnode_sir_mc_philox_counted): the frontier walk of SirKernels<SIR_SCALAR, false, false>
static constexpr auto kSirCountedLds = &k_sir_frontier<uint16_t, true, true, false, false>;
static constexpr auto kSirCountedMem = &k_sir_frontier<int32_t, false, true, false, false>;

template <int RATES, class F> static void sir_dispatch_rates(bool traj, bool init, F&& f) {
    if (traj) { if (init) f(SirKernels<RATES, true, true>{}); else f(SirKernels<RATES, true, false>{}); }
    else { if (init) f(SirKernels<RATES, false, true>{}); else f(SirKernels<RATES, false, false>{}); }
}
template <class F> static void sir_dispatch(int rates, bool traj, bool init, F&& f) {   // f(SirKernels<...>{}) of the 3 x 2 x 2 forms
    if (rates == SIR_EDGES) sir_dispatch_rates<SIR_EDGES>(traj, init, f);
    else if (rates == SIR_NODES) sir_dispatch_rates<SIR_NODES>(traj, init, f);
    else sir_dispatch_rates<SIR_SCALAR>(traj, init, f);
}
template <class F> static void sir_dispatch_sched(bool traj, bool init, F&& f) {        // f(SirKernels<SIR_EDGES, ..., true>{}) of the 2 x 2 scheduled forms
    if (traj) { if (init) f(SirKernels<SIR_EDGES, true, true, true>{}); else f(SirKernels<SIR_EDGES, true, false, true>{}); }
    else { if (init) f(SirKernels<SIR_EDGES, false, true, true>{}); else f(SirKernels<SIR_EDGES, false, false, true>{}); }
}
template <class OUT, class F> static void sir_dispatch_sweep(F&& f) { f(SirKernels<SIR_EDGES, false, true, true, OUT>{}); }

int gn_sir_set_attributes() {       // once per device, from gnode_graph_create
    hipError_t err = hipSuccess;
    auto lift = [&](auto kernel) {   // dynamic LDS up to kLdsStateLimit (scan_mem takes none)
        const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsStateLimit);
        if (err == hipSuccess) err = e;
    };
    const auto lift_form = [&](auto K) { lift(K.frontier_lds); lift(K.frontier_mem); lift(K.scan_lds); };
    for (int form = 0; form < 12; ++form) sir_dispatch(form >> 2, form & 2, form & 1, lift_form);
    for (int form = 0; form < 4; ++form) sir_dispatch_sched(form & 2, form & 1, lift_form);
    // (an output policy's static LDS comes on top: sir_launch_plan keeps dynamic + static_lds within kLdsStateLimit)
    sir_each_output([&](auto out) { sir_dispatch_sweep<decltype(out)>(lift_form); });
    lift(kSirCountedLds); lift(kSirCountedMem); lift(&k_sir_coins);
    GN_HIP(err);
    return 0;
}

extern "C" size_t gnode_sir_coins_workspace_bytes(void) { return gn_align(4096 * sizeof(int32_t)) + gn_align(64); }
static size_t sir_ws_bytes(gnode_graph_t g, int32_t T, int form) { return g ? sir_layout(g->info.n, g->nnz, g->n_bigrow, T).bytes[form] : 0; }
extern "C" size_t gnode_sir_workspace_bytes(gnode_graph_t g, int32_t T) { return sir_ws_bytes(g, T, SIR_SCALAR); }
extern "C" size_t gnode_sir_nodes_workspace_bytes(gnode_graph_t g, int32_t T) { return sir_ws_bytes(g, T, SIR_NODES); }
extern "C" size_t gnode_sir_traj_workspace_bytes(gnode_graph_t g, int32_t T) { return sir_ws_bytes(g, T, SIR_NODES); }   // scalar rates too
extern "C" size_t gnode_sir_edges_workspace_bytes(gnode_graph_t g, int32_t T) { return sir_ws_bytes(g, T, SIR_EDGES); }
extern "C" size_t gnode_sir_init_workspace_bytes(gnode_graph_t g, int32_t T) { return sir_ws_bytes(g, T, SIR_INIT); }
extern "C" size_t gnode_sir_schedule_workspace_bytes(gnode_graph_t g, int32_t T, int32_t P) {
    return g && P >= 1 ? sir_schedule_layout(g->info.n, g->nnz, g->n_bigrow, T, P).total : 0;
}

// One Monte-Carlo call, as its entry states it (include/gnode.h documents the arrays).
struct SirCall {
    const char* who = "";                    // the entry's name, for the messages
    gnode_graph_t g = nullptr;
    // the start: a seed list on the host, or (drawn) host fp64 [n][3], each trajectory's start drawn from (pS, pI, pR)
    const int32_t* seeds = nullptr; int32_t n_seeds = 0; bool drawn = false; const double* init = nullptr;
    SirRates rates;
    // the outputs.  need_traj: the entry is for per-trajectory output (counts alone will not do)
    uint32_t* counts = nullptr; int16_t* events = nullptr; uint32_t* curves = nullptr; bool need_traj = false;
    int64_t sims = 0, sim_offset = 0; int32_t T = 0; uint64_t rng_seed = 0;
    void *workspace = nullptr, *stream = nullptr; size_t workspace_bytes = 0; int ws_form = SIR_SCALAR;   // which of SirLayout::bytes the entry asks for
    bool edge_scan = false;                  // the scan kernel (the cross-check) instead of the frontier walk
    uint64_t* stats_host = nullptr;          // gnode_sir_mc_philox_counted: the counting instances, their tally [4] copied here
    // gnode_sir_mc_philox_schedule (sched): P phases of per-edge tables, host fp64 w [P][nnz] and gamma [P][n], and the host phase
    // table [T]; `rates` rests
    bool sched = false; const int32_t* phase = nullptr; int32_t P = 0; const double *w_sched = nullptr, *gamma_sched = nullptr;
};
// the arguments every entry has, under the names every entry gives them
#define SIR_CALL(c, name)                                                                                                         \
    SirCall c; c.who = name; c.g = g; c.counts = counts; c.sims = sims; c.sim_offset = sim_offset; c.T = T; c.rng_seed = rng_seed; \
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = stream

static int sir_mc_philox_impl(const SirCall& c) {
    const gnode_graph_t g = c.g;
    const SirRates& r = c.rates;
    const bool traj = c.events || c.curves;
    const hipStream_t st = (hipStream_t)c.stream;
    GN_CHECK_ARG(g && c.workspace && (!c.drawn || c.init), "%s: null pointer", c.who);
    GN_CHECK_ARG(!c.sched || (c.P >= 1 && c.gamma_sched && (c.w_sched || g->nnz == 0) && (c.phase || c.T <= 1)), "%s: a schedule takes P >= 1 phases (P = %d), the phase table and both rate tables", c.who, c.P);
    GN_CHECK_ARG(c.need_traj ? traj : (traj || c.counts), "%s: no output array given", c.who);
    GN_CHECK_ARG(!c.events || (c.T <= 32767 && ((uintptr_t)c.events & 1u) == 0), "%s: events hold int16 steps (T = %d, at most 32767) at an even address", c.who, c.T);
    GN_CHECK_ARG(r.form != SIR_NODES || (r.beta_nodes && r.gamma_nodes), "%s: one per-node rate array without the other", c.who);
    GN_CHECK_ARG(r.form != SIR_EDGES || ((r.w_edges || g->nnz == 0) && !r.beta_nodes), "%s: per-edge rates take a weight array and no per-node beta", c.who);
    GN_CHECK_ARG(c.n_seeds >= 0 && c.n_seeds <= 4096 && (c.seeds || c.n_seeds == 0), "%s: 0..4096 seeds", c.who);
    GN_CHECK_ARG(c.T >= 1 && c.sims >= 0 && c.sims <= 0xFFFFFFFFll && c.sim_offset >= 0 && c.sim_offset + c.sims <= 0xFFFFFFFFll, "%s: bad T/sims/sim_offset", c.who);
    const int n = g->info.n, T = c.T;
    for (int i = 0; i < c.n_seeds; ++i)
        GN_CHECK_ARG(c.seeds[i] >= 0 && c.seeds[i] < n, "%s: seed %d out of range", c.who, c.seeds[i]);
    const SirScheduleLayout SL = sir_schedule_layout(n, g->nnz, g->n_bigrow, T, c.sched ? c.P : 1);
    const SirLayout L = c.sched ? static_cast<const SirLayout&>(SL) : sir_layout(n, g->nnz, g->n_bigrow, T);
    const size_t need = c.sched ? SL.total : L.bytes[c.ws_form];
    if (c.workspace_bytes < need) {
        gnode_set_error("%s: workspace %zu < %zu", c.who, c.workspace_bytes, need);
        return c.stats_host ? GNODE_ERR_ARG : GNODE_ERR_WORKSPACE;   // (the counted entry has always called it an argument)
    }
    // A drawn start with per-node rates on a graph of fewer entries than nodes: two per-node arrays would reach into the start
    // thresholds.  The per-node form is the per-edge one with w[p] = beta[col[p]] (same coins, same counts), and that one fits:
    // sir_stage restates it.  The column ids come back on the caller's stream, which the call synchronises anyway
    const bool restate = c.drawn && r.form == SIR_NODES && L.bytes[SIR_NODES] > L.bytes[SIR_EDGES];
    std::vector<int32_t> col(restate ? (size_t)std::max<int64_t>(g->nnz, 1) : 0);
    if (restate && g->nnz) {
        GN_HIP(hipMemcpyAsync(col.data(), g->col, sizeof(int32_t) * (size_t)g->nnz, hipMemcpyDeviceToHost, st));
        GN_HIP(hipStreamSynchronize(st));
    }
    const SirThresholds thr = c.sched ? sir_stage_schedule(c.who, n, g->nnz, T, c.P, c.phase, c.w_sched, c.gamma_sched, c.init)
                                      : sir_stage(c.who, n, g->nnz, r, restate ? col.data() : nullptr, c.init);
    GN_CHECK_ARG(thr.error.empty(), "%s", thr.error.c_str());
    const int form = restate || c.sched ? SIR_EDGES : r.form;
    char* ws = (char*)c.workspace;
    uint32_t* hist = (uint32_t*)(ws + L.hist);
    int32_t* seeds = (int32_t*)(ws + L.seeds);
    unsigned long long* stats = c.stats_host ? (unsigned long long*)(ws + L.rows) : nullptr;
    const unsigned long long *thr_b = (const unsigned long long*)(ws + L.thr), *thr_g = thr_b + (thr.rates.size() - (form ? (size_t)n * (c.sched ? c.P : 1) : 0));
    const int32_t* phase_dev = (const int32_t*)(ws + SL.phase);                      // (sched)
    const unsigned long long* thr_start = (const unsigned long long*)(ws + L.start);
    if (stats) GN_HIP(hipMemsetAsync(stats, 0, 4 * sizeof(unsigned long long), st));
    if (int e = gn_zero_async(hist, L.seeds - L.hist, st)) return e;
    if (c.events && c.sims > 0) {                          // the "never" background, by a kernel like the zero fill above
        const size_t count = (size_t)2 * (size_t)c.sims * (size_t)n;
        const int grid = (int)std::min<size_t>((count / 8 + 255) / 256 + 1, (size_t)g->info.num_cu * 8);
        hipLaunchKernelGGL(k_fill_i16, dim3(grid), dim3(256), 0, st, c.events, count, (int16_t)-1);
        GN_LAUNCH_CHECK();
    }
    // seed ids: up to 32 travel as a kernel argument (no copy, no synchronisation -- the reference's experiments use 2);
    // longer lists are copied from the caller's host array, which may be a temporary, so the stream is synchronised
    // before returning control (documented in gnode.h)
    SeedArg sa;
    for (int i = 0; i < 32; ++i) sa.v[i] = i < c.n_seeds ? c.seeds[i] : 0;
    if (c.n_seeds <= 32) {
        hipLaunchKernelGGL(k_put_seeds, dim3(1), dim3(32), 0, st, sa, c.n_seeds, seeds);
        GN_LAUNCH_CHECK();
    } else {
        GN_HIP(hipMemcpyAsync(seeds, c.seeds, sizeof(int32_t) * c.n_seeds, hipMemcpyHostToDevice, st));
    }
    if (form) GN_HIP(hipMemcpyAsync((void*)thr_b, thr.rates.data(), thr.rates.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    if (c.init) GN_HIP(hipMemcpyAsync((void*)thr_start, thr.start.data(), thr.start.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    if (c.sched && T > 1) GN_HIP(hipMemcpyAsync((void*)phase_dev, c.phase, sizeof(int32_t) * (size_t)T, hipMemcpyHostToDevice, st));
    if (c.n_seeds > 32 || form || c.init) GN_HIP(hipStreamSynchronize(st));     // the host arrays are done with
    const uint32_t k0 = (uint32_t)(c.rng_seed & 0xFFFFFFFFull), k1 = (uint32_t)(c.rng_seed >> 32);
    if (c.sims > 0) {
        const bool sampled = gn_prof_begin(3, st);
        const SirLaunch P = sir_launch_plan(n, g->n_bigrow, g->info.num_cu, c.sims, c.edge_scan);
        const bool frontier = P.path == SIR_FRONTIER_LDS || P.path == SIR_FRONTIER_MEM;
        void* tail = P.path == SIR_FRONTIER_MEM || P.path == SIR_SCAN_MEM ? ws + L.tail : nullptr;   // the lists / the state, when not in LDS
        auto launch = [&](auto K) {
            using Kt = decltype(K);
            SirTraj<Kt::TRAJ> tr;
            SirInit<Kt::INIT> in;
            SirSched<Kt::SCHED> sc;
            if constexpr (Kt::SCHED) sc.phase = phase_dev;
            SirThr<Kt::NODES> tb, tg;                      // the staged arrays, or the two numbers
            if constexpr (Kt::TRAJ) { tr.events = c.events; tr.curves = c.curves; }
            if constexpr (Kt::INIT) in.thr = thr_start;
            if constexpr (Kt::NODES) { tb = thr_b; tg = thr_g; } else { tb = thr.tb; tg = thr.tg; }
            if (frontier) {
                auto kernel = P.path == SIR_FRONTIER_LDS ? Kt::frontier_lds : Kt::frontier_mem;
                if constexpr (!Kt::NODES && !Kt::TRAJ && !Kt::INIT) if (stats) kernel = P.path == SIR_FRONTIER_LDS ? kSirCountedLds : kSirCountedMem;
                hipLaunchKernelGGL(kernel, dim3(P.grid), dim3(P.threads), P.lds, st, g->rowptr, g->col, n, seeds, c.n_seeds, tb, tg, (long)c.sims,
                                   (long)c.sim_offset, T, k0, k1, hist, (int32_t*)tail, stats, tr, in, sc, SirNoJobs{}, SirNoSweep{});
            } else {
                auto kernel = P.path == SIR_SCAN_LDS ? Kt::scan_lds : Kt::scan_mem;
                hipLaunchKernelGGL(kernel, dim3(P.grid), dim3(P.threads), P.lds, st, g->src, g->col, (long)g->nnz, n, seeds, c.n_seeds, tb, tg, (long)c.sims,
                                   (long)c.sim_offset, T, k0, k1, hist, (uint8_t*)tail, tr, in, sc, SirNoJobs{}, SirNoSweep{});
            }
        };
        // the drawn start and the schedule are sets of instances of their own: the others do not carry them
        if (c.sched) sir_dispatch_sched(traj, c.init != nullptr, launch);
        else sir_dispatch(form, traj, c.init != nullptr, launch);
        if (sampled) gn_prof_end(3, st);
        GN_LAUNCH_CHECK();
    }
    if (c.counts) {                                        // (per-trajectory output alone: no counts)
        hipLaunchKernelGGL(c.init ? k_sir_finalize<true> : k_sir_finalize<false>, dim3((n + 255) / 256), dim3(256), 0, st, hist, n, T, (uint32_t)c.sims, c.counts);
        GN_LAUNCH_CHECK();
    }
    if (stats) {
        GN_HIP(hipMemcpyAsync(c.stats_host, stats, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        GN_HIP(hipStreamSynchronize(st));
    }
    return 0;
}

extern "C" int gnode_sir_mc_philox(gnode_graph_t g, const int32_t* seeds_host, int32_t n_seeds, double beta, double gamma, int64_t sims,
                                   int64_t sim_offset, int32_t T, uint64_t rng_seed, uint32_t* counts, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    SIR_CALL(c, "gnode_sir_mc_philox");
    c.seeds = seeds_host; c.n_seeds = n_seeds; c.rates.beta = beta; c.rates.gamma = gamma;
    return sir_mc_philox_impl(c);
}

// The profiling instantiation: the same counts, plus stats_host[0] Philox blocks computed, [1] infection coins drawn, [2] recovery
// coins drawn, [3] CSR entries read.  Synchronises `stream`.
extern "C" int gnode_sir_mc_philox_counted(gnode_graph_t g, const int32_t* seeds_host, int32_t n_seeds, double beta, double gamma, int64_t sims,
                                           int64_t sim_offset, int32_t T, uint64_t rng_seed, uint32_t* counts, void* workspace,
                                           size_t workspace_bytes, void* stream, uint64_t* stats_host) {
    GN_CHECK_ARG(stats_host && g && g->nnz >= 8, "gnode_sir_mc_philox_counted: null pointer, or a graph too small to hold the tally");
    SIR_CALL(c, "gnode_sir_mc_philox_counted");
    c.seeds = seeds_host; c.n_seeds = n_seeds; c.rates.beta = beta; c.rates.gamma = gamma; c.stats_host = stats_host;
    return sir_mc_philox_impl(c);
}

extern "C" int gnode_sir_mc_philox_scan(gnode_graph_t g, const int32_t* seeds_host, int32_t n_seeds, double beta, double gamma, int64_t sims,
                                        int64_t sim_offset, int32_t T, uint64_t rng_seed, uint32_t* counts, void* workspace, size_t workspace_bytes,
                                        void* stream) {
    SIR_CALL(c, "gnode_sir_mc_philox_scan");
    c.seeds = seeds_host; c.n_seeds = n_seeds; c.rates.beta = beta; c.rates.gamma = gamma; c.edge_scan = true;
    return sir_mc_philox_impl(c);
}

// Per-node rates: beta_host[v] is the probability that an entry (u -> v) with u infected infects the susceptible v, gamma_host[u]
// that the infected u recovers.  Staged through the workspace (sir_stage); synchronises `stream`.
extern "C" int gnode_sir_mc_philox_nodes(gnode_graph_t g, const int32_t* seeds_host, int32_t n_seeds, const double* beta_host,
                                         const double* gamma_host, int64_t sims, int64_t sim_offset, int32_t T, uint64_t rng_seed, uint32_t* counts,
                                         void* workspace, size_t workspace_bytes, void* stream, int32_t edge_scan) {
    SIR_CALL(c, "gnode_sir_mc_philox_nodes");
    c.seeds = seeds_host; c.n_seeds = n_seeds; c.ws_form = SIR_NODES; c.edge_scan = edge_scan != 0;
    c.rates.form = SIR_NODES; c.rates.beta_nodes = beta_host; c.rates.gamma_nodes = gamma_host;
    return sir_mc_philox_impl(c);
}

// Per-trajectory output: the kernels' TRAJ instances; scalar rates when both arrays are null, the per-node form's workspace either way.
extern "C" int gnode_sir_mc_philox_traj(gnode_graph_t g, const int32_t* seeds_host, int32_t n_seeds, double beta, double gamma,
                                        const double* beta_host, const double* gamma_host, int64_t sims, int64_t sim_offset, int32_t T,
                                        uint64_t rng_seed, int16_t* events, uint32_t* curves, uint32_t* counts, void* workspace,
                                        size_t workspace_bytes, void* stream, int32_t edge_scan) {
    SIR_CALL(c, "gnode_sir_mc_philox_traj");
    c.seeds = seeds_host; c.n_seeds = n_seeds; c.ws_form = SIR_NODES; c.edge_scan = edge_scan != 0; c.events = events; c.curves = curves; c.need_traj = true;
    c.rates.form = (beta_host || gamma_host) ? SIR_NODES : SIR_SCALAR; c.rates.beta = beta; c.rates.gamma = gamma; c.rates.beta_nodes = beta_host; c.rates.gamma_nodes = gamma_host;
    return sir_mc_philox_impl(c);
}

// Per-edge transmission probabilities: w_host[p] is the probability that the row of CSR position p infects col[p] (EDGES instances).
extern "C" int gnode_sir_mc_philox_edges(gnode_graph_t g, const int32_t* seeds_host, int32_t n_seeds, const double* w_host, double gamma,
                                         const double* gamma_host, int64_t sims, int64_t sim_offset, int32_t T, uint64_t rng_seed, uint32_t* counts,
                                         void* workspace, size_t workspace_bytes, void* stream, int32_t edge_scan) {
    SIR_CALL(c, "gnode_sir_mc_philox_edges");
    c.seeds = seeds_host; c.n_seeds = n_seeds; c.ws_form = SIR_EDGES; c.edge_scan = edge_scan != 0;
    c.rates.form = SIR_EDGES; c.rates.w_edges = w_host; c.rates.gamma = gamma; c.rates.gamma_nodes = gamma_host;
    return sir_mc_philox_impl(c);
}
extern "C" int gnode_sir_mc_philox_traj_edges(gnode_graph_t g, const int32_t* seeds_host, int32_t n_seeds, const double* w_host, double gamma,
                                              const double* gamma_host, int64_t sims, int64_t sim_offset, int32_t T, uint64_t rng_seed,
                                              int16_t* events, uint32_t* curves, uint32_t* counts, void* workspace, size_t workspace_bytes,
                                              void* stream, int32_t edge_scan) {
    SIR_CALL(c, "gnode_sir_mc_philox_traj_edges");
    c.seeds = seeds_host; c.n_seeds = n_seeds; c.ws_form = SIR_EDGES; c.edge_scan = edge_scan != 0; c.events = events; c.curves = curves; c.need_traj = true;
    c.rates.form = SIR_EDGES; c.rates.w_edges = w_host; c.rates.gamma = gamma; c.rates.gamma_nodes = gamma_host;
    return sir_mc_philox_impl(c);
}

// Initial-state distributions: one entry for the three rate forms and every output; each trajectory's start is drawn from the
// staged thresholds of `init_host` instead of a seed list (INIT instances).
extern "C" int gnode_sir_mc_philox_init(gnode_graph_t g, const double* init_host, double beta, const double* beta_host, const double* w_host,
                                        double gamma, const double* gamma_host, int64_t sims, int64_t sim_offset, int32_t T, uint64_t rng_seed,
                                        int16_t* events, uint32_t* curves, uint32_t* counts, void* workspace, size_t workspace_bytes, void* stream,
                                        int32_t edge_scan) {
    SIR_CALL(c, "gnode_sir_mc_philox_init");
    c.drawn = true; c.init = init_host; c.ws_form = SIR_INIT; c.edge_scan = edge_scan != 0; c.events = events; c.curves = curves;
    c.rates.form = w_host ? SIR_EDGES : (beta_host || gamma_host) ? SIR_NODES : SIR_SCALAR; c.rates.beta = beta; c.rates.gamma = gamma;
    c.rates.beta_nodes = beta_host; c.rates.gamma_nodes = gamma_host; c.rates.w_edges = w_host;
    return sir_mc_philox_impl(c);
}

// Rates that change over time: P phases of the per-edge form, chosen per step by the phase table (SCHED instances).  The start
// is a seed list (rows as gnode_sir_mc_philox_traj_edges) or drawn (rows as gnode_sir_mc_philox_init), exactly one of them.
extern "C" int gnode_sir_mc_philox_schedule(gnode_graph_t g, const int32_t* seeds_host, int32_t n_seeds, const double* init_host,
                                            const int32_t* phase_host, int32_t P, const double* w_host, const double* gamma_host, int64_t sims,
                                            int64_t sim_offset, int32_t T, uint64_t rng_seed, int16_t* events, uint32_t* curves, uint32_t* counts,
                                            void* workspace, size_t workspace_bytes, void* stream, int32_t edge_scan) {
    const bool listed = seeds_host != nullptr || n_seeds != 0;
    GN_CHECK_ARG(listed != (init_host != nullptr), "gnode_sir_mc_philox_schedule: the start is a seed list or init_host, exactly one of them");
    SIR_CALL(c, "gnode_sir_mc_philox_schedule");
    c.seeds = seeds_host; c.n_seeds = n_seeds; c.drawn = init_host != nullptr; c.init = init_host; c.edge_scan = edge_scan != 0;
    c.events = events; c.curves = curves;
    c.sched = true; c.phase = phase_host; c.P = P; c.w_sched = w_host; c.gamma_sched = gamma_host;
    return sir_mc_philox_impl(c);
}

// Outbreak sizes for many candidates in one launch (SWEEP instances): C x sims trajectories of the drawn-start scheduled form,
// candidate c's node overridden in the start and its phase row read from shifts[c] on; the sums, no histogram.
extern "C" size_t gnode_sir_sweep_workspace_bytes(gnode_graph_t g, int32_t T, int32_t P, int32_t L, int32_t C) {
    return g && T >= 1 && P >= 1 && L >= T && C >= 1 ? sir_sweep_layout(g->info.n, g->nnz, g->n_bigrow, T, P, L, C).total : 0;
}
// A sweep call with output `out` (its description, gnode_sir_sweep.h): check, layout, stage, workspace check, upload, launch.
template <class OUTPUT> static int sir_sweep_impl(const SirSweepCall& c, const OUTPUT& out) {
    using OUT = typename OUTPUT::Policy;
    const gnode_graph_t g = c.g;
    const hipStream_t st = (hipStream_t)c.stream;
    const int32_t C = c.C, P = c.P, L = c.L, T = c.T;
    GN_CHECK_ARG(g && c.workspace && c.init && c.cand && out.complete(), "%s: null pointer", c.who);
    GN_CHECK_ARG(P >= 1 && c.gamma && (c.w || g->nnz == 0) && (c.phase || L <= 1), "%s: a schedule takes P >= 1 phases (P = %d), the phase row and both rate tables", c.who, P);
    GN_CHECK_ARG(C >= 1, "%s: C = %d: at least one candidate", c.who, C);
    GN_CHECK_ARG(c.action == 0 || c.action == 1, "%s: action %d is neither 0 (seed) nor 1 (immunise)", c.who, c.action);
    GN_CHECK_ARG(T >= 1 && c.sims >= 0 && c.sims <= 0xFFFFFFFFll && c.sim_offset >= 0 && c.sim_offset + c.sims <= 0xFFFFFFFFll, "%s: bad T/sims/sim_offset", c.who);
    GN_CHECK_ARG(L >= T, "%s: the phase row holds L = %d entries, fewer than T = %d", c.who, L, T);
    const int n = g->info.n;
    const typename OUTPUT::Layout W = out.layout(c);
    const typename OUTPUT::Staged staged = out.stage(c);
    const SirThresholds& thr = staged.thr;
    if (OUTPUT::args_first) GN_CHECK_ARG(thr.error.empty(), "%s", thr.error.c_str());
    if (c.workspace_bytes < W.total) {
        gnode_set_error("%s: workspace %zu < %zu", c.who, c.workspace_bytes, W.total);
        return GNODE_ERR_WORKSPACE;
    }
    GN_CHECK_ARG(thr.error.empty(), "%s", thr.error.c_str());
    char* ws = (char*)c.workspace;
    const unsigned long long *thr_b = (const unsigned long long*)(ws + W.thr), *thr_g = thr_b + (size_t)P * (size_t)g->nnz;
    const std::vector<int32_t> no_shift(c.shifts ? 0 : (size_t)C, 0);
    std::vector<SirUpload> up = {{W.thr, thr.rates.data(), thr.rates.size() * sizeof(unsigned long long)},
                                 {W.start, thr.start.data(), thr.start.size() * sizeof(unsigned long long)},
                                 {W.phase, c.phase, L > 1 ? sizeof(int32_t) * (size_t)L : 0},
                                 {W.cand, c.cand, sizeof(int32_t) * (size_t)C},
                                 {W.shifts, c.shifts ? c.shifts : no_shift.data(), sizeof(int32_t) * (size_t)C}};
    for (const SirUpload& u : staged.uploads(W)) up.push_back(u);
    for (const SirUpload& u : up)
        if (u.bytes) GN_HIP(hipMemcpyAsync(ws + u.at, u.from, u.bytes, hipMemcpyHostToDevice, st));
    GN_HIP(hipStreamSynchronize(st));                          // the host arrays are done with
    if (c.sims == 0) return 0;
    const uint32_t k0 = (uint32_t)(c.rng_seed & 0xFFFFFFFFull), k1 = (uint32_t)(c.rng_seed >> 32);
    const bool sampled = gn_prof_begin(3, st);
    const SirLaunch Pl = sir_launch_plan(n, g->n_bigrow, g->info.num_cu, (int64_t)C * c.sims, c.edge_scan != 0, OUTPUT::static_lds);
    void* tail = Pl.path == SIR_FRONTIER_MEM || Pl.path == SIR_SCAN_MEM ? ws + W.tail : nullptr;   // the lists / the state, when not in LDS
    SirInit<true> in; in.thr = (const unsigned long long*)(ws + W.start);
    SirSched<true> sc; sc.phase = (const int32_t*)(ws + W.phase);
    typename OUT::Jobs jobs; jobs.cand = (const int32_t*)(ws + W.cand); jobs.shifts = (const int32_t*)(ws + W.shifts); jobs.C = C; jobs.action = c.action;
    OUT o;
    out.fill(jobs, o, ws, W);
    sir_dispatch_sweep<OUT>([&](auto K) {
        using Kt = decltype(K);
        if (Pl.path == SIR_FRONTIER_LDS || Pl.path == SIR_FRONTIER_MEM) {
            auto kernel = Pl.path == SIR_FRONTIER_LDS ? Kt::frontier_lds : Kt::frontier_mem;
            hipLaunchKernelGGL(kernel, dim3(Pl.grid), dim3(Pl.threads), Pl.lds, st, g->rowptr, g->col, n, (const int*)nullptr, 0, thr_b, thr_g, (long)c.sims,
                               (long)c.sim_offset, T, k0, k1, (uint32_t*)nullptr, (int32_t*)tail, (unsigned long long*)nullptr, SirTraj<false>{}, in, sc, jobs, o);
        } else {
            auto kernel = Pl.path == SIR_SCAN_LDS ? Kt::scan_lds : Kt::scan_mem;
            hipLaunchKernelGGL(kernel, dim3(Pl.grid), dim3(Pl.threads), Pl.lds, st, g->src, g->col, (long)g->nnz, n, (const int*)nullptr, 0, thr_b, thr_g,
                               (long)c.sims, (long)c.sim_offset, T, k0, k1, (uint32_t*)nullptr, (uint8_t*)tail, SirTraj<false>{}, in, sc, jobs, o);
        }
    });
    if (sampled) gn_prof_end(3, st);
    GN_LAUNCH_CHECK();
    return 0;
}
// the arguments every sweep entry has, under the names every one gives them
#define SIR_SWEEP_CALL(name)                                                                                                                   \
    SirSweepCall{name, g, init_host, candidates_host, shifts_host, C, action, phase_host, P, L, w_host, gamma_host, sims, sim_offset, T, rng_seed, \
                 workspace, workspace_bytes, stream, edge_scan}
extern "C" int gnode_sir_mc_philox_sweep(gnode_graph_t g, const double* init_host, const int32_t* candidates_host, const int32_t* shifts_host,
                                         int32_t C, int32_t action, const int32_t* phase_host, int32_t P, int32_t L, const double* w_host,
                                         const double* gamma_host, int64_t sims, int64_t sim_offset, int32_t T, uint64_t rng_seed,
                                         uint64_t* sums, uint32_t* ever, void* workspace, size_t workspace_bytes, void* stream,
                                         int32_t edge_scan) {
    return sir_sweep_impl(SIR_SWEEP_CALL("gnode_sir_mc_philox_sweep"), SirSumsOutput{sums, ever});
}

// Monte-Carlo source scores (SirScores): the sweep's trajectories, every step of every one binned by its similarity with each of
// O snapshots; the histogram, no sums.
extern "C" size_t gnode_sir_sweep_scores_workspace_bytes(gnode_graph_t g, int32_t T, int32_t P, int32_t L, int32_t C, int32_t O) {
    return g && T >= 1 && P >= 1 && L >= T && C >= 1 && O >= 1 && O <= GN_SIR_SCORE_MAXO ? sir_score_layout(g->info.n, g->nnz, g->n_bigrow, T, P, L, C, O).total : 0;
}
extern "C" int gnode_sir_mc_philox_sweep_scores(gnode_graph_t g, const double* init_host, const int32_t* candidates_host, const int32_t* shifts_host,
                                                int32_t C, int32_t action, const int32_t* phase_host, int32_t P, int32_t L, const double* w_host,
                                                const double* gamma_host, const int8_t* obs_host, int32_t O, int32_t measure, int32_t bins,
                                                int64_t sims, int64_t sim_offset, int32_t T, uint64_t rng_seed, uint64_t* hist, void* workspace,
                                                size_t workspace_bytes, void* stream, int32_t edge_scan) {
    return sir_sweep_impl(SIR_SWEEP_CALL("gnode_sir_mc_philox_sweep_scores"), SirScoresOutput{obs_host, O, measure, bins, hist});
}

// Monte-Carlo source scores from timed evidence (SirTimedScores): the sweep's trajectories, every age t of every one binned by
// the number of records of each of O evidence sets it agrees with; the histogram, no sums.
extern "C" size_t gnode_sir_sweep_timed_workspace_bytes(gnode_graph_t g, int32_t T, int32_t P, int32_t L, int32_t C, int32_t O, int32_t R) {
    return g && T >= 1 && P >= 1 && L >= T && C >= 1 && O >= 1 && O <= GN_SIR_SCORE_MAXO && R >= 1 ? sir_timed_layout(g->info.n, g->nnz, g->n_bigrow, T, P, L, C, O, R).total : 0;
}
extern "C" int gnode_sir_mc_philox_sweep_timed(gnode_graph_t g, const double* init_host, const int32_t* candidates_host, const int32_t* shifts_host,
                                               int32_t C, int32_t action, const int32_t* phase_host, int32_t P, int32_t L, const double* w_host,
                                               const double* gamma_host, const int32_t* rec_set, const int32_t* rec_node, const int32_t* rec_offset,
                                               const int32_t* rec_kind, int32_t R, int32_t O, int32_t bins, int64_t sims, int64_t sim_offset, int32_t T,
                                               uint64_t rng_seed, uint64_t* hist, void* workspace, size_t workspace_bytes, void* stream,
                                               int32_t edge_scan) {
    return sir_sweep_impl(SIR_SWEEP_CALL("gnode_sir_mc_philox_sweep_timed"), SirTimedOutput{{rec_set, rec_node, rec_offset, rec_kind, R, O}, bins, hist});
}

// Nowcast and forecast from timed evidence (SirPosteriorCounts): the sweep's trajectories, each accepted for the evidence sets whose
// records it matches at age `now`, and the states of the accepted ones counted per node at now + horizons[j]; no sums.
extern "C" size_t gnode_sir_sweep_posterior_workspace_bytes(gnode_graph_t g, int32_t T, int32_t P, int32_t L, int32_t C, int32_t O, int32_t R, int32_t H) {
    return g && T >= 1 && P >= 1 && L >= T && C >= 1 && O >= 1 && O <= GN_SIR_SCORE_MAXO && R >= 1 && H >= 1 && H <= GN_SIR_POST_MAXH
               ? sir_post_layout(g->info.n, g->nnz, g->n_bigrow, T, P, L, C, O, R, H).total : 0;
}
extern "C" int gnode_sir_mc_philox_sweep_posterior(gnode_graph_t g, const double* init_host, const int32_t* candidates_host, const int32_t* shifts_host,
                                                   int32_t C, int32_t action, const int32_t* phase_host, int32_t P, int32_t L, const double* w_host,
                                                   const double* gamma_host, const int32_t* rec_set, const int32_t* rec_node, const int32_t* rec_offset,
                                                   const int32_t* rec_kind, int32_t R, int32_t O, int32_t now, const int32_t* horizons_host, int32_t H,
                                                   int64_t sims, int64_t sim_offset, int32_t T, uint64_t rng_seed, uint64_t* counts, uint64_t* accepted,
                                                   void* workspace, size_t workspace_bytes, void* stream, int32_t edge_scan) {
    return sir_sweep_impl(SIR_SWEEP_CALL("gnode_sir_mc_philox_sweep_posterior"),
                          SirPosteriorOutput{{rec_set, rec_node, rec_offset, rec_kind, R, O}, now, horizons_host, H, counts, accepted});
}
// The posterior by the number of missed records (SirPosteriorStrata): a trajectory that misses d <= mismatches records of a set is
// counted for it in stratum d; the posterior's workspace.
extern "C" int gnode_sir_mc_philox_sweep_posterior_strata(gnode_graph_t g, const double* init_host, const int32_t* candidates_host,
                                                          const int32_t* shifts_host, int32_t C, int32_t action, const int32_t* phase_host, int32_t P,
                                                          int32_t L, const double* w_host, const double* gamma_host, const int32_t* rec_set,
                                                          const int32_t* rec_node, const int32_t* rec_offset, const int32_t* rec_kind, int32_t R, int32_t O,
                                                          int32_t now, const int32_t* horizons_host, int32_t H, int32_t mismatches, int64_t sims,
                                                          int64_t sim_offset, int32_t T, uint64_t rng_seed, uint64_t* counts, uint64_t* accepted,
                                                          void* workspace, size_t workspace_bytes, void* stream, int32_t edge_scan) {
    return sir_sweep_impl(SIR_SWEEP_CALL("gnode_sir_mc_philox_sweep_posterior_strata"),
                          SirStrataOutput{{{rec_set, rec_node, rec_offset, rec_kind, R, O}, now, horizons_host, H, counts, accepted}, mismatches});
}

extern "C" int gnode_sir_mc_coins(const int32_t* table_src, const int32_t* table_dst, int64_t n_table, int32_t n,
                                  const int32_t* seeds_host, int32_t n_seeds, double beta, double gamma, int64_t sims,
                                  int32_t T, const double* coins, int64_t n_coins, uint32_t* counts,
                                  int64_t* coins_used_host, void* workspace, size_t workspace_bytes, void* stream) {
    GN_CHECK_ARG(table_src && table_dst && counts && workspace && coins_used_host && (coins || n_coins == 0),
                 "gnode_sir_mc_coins: null pointer");
    GN_CHECK_ARG(n > 0 && (size_t)2 * n <= kLdsStateLimit, "gnode_sir_mc_coins: parity mode supports n <= %zu (got %d)",
                 kLdsStateLimit / 2, n);
    GN_CHECK_ARG(n_seeds >= 0 && n_seeds <= 4096 && T >= 1 && sims >= 0 && n_table >= 0, "gnode_sir_mc_coins: bad sizes");
    for (int i = 0; i < n_seeds; ++i)
        GN_CHECK_ARG(seeds_host[i] >= 0 && seeds_host[i] < n, "gnode_sir_mc_coins: seed %d out of range", seeds_host[i]);
    if (workspace_bytes < gnode_sir_coins_workspace_bytes()) {
        gnode_set_error("gnode_sir_mc_coins: workspace too small");
        return GNODE_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    int32_t* seeds = (int32_t*)workspace;
    long long* used = (long long*)((char*)workspace + gn_align(4096 * sizeof(int32_t)));
    if (n_seeds) GN_HIP(hipMemcpyAsync(seeds, seeds_host, sizeof(int32_t) * n_seeds, hipMemcpyHostToDevice, st));
    {   // the parity kernel takes no graph handle: make sure this device's kernel attributes are set (once, under the lock)
        int dev = 0;
        GN_HIP(hipGetDevice(&dev));
        if (int e = gn_device_setup_once(dev)) return e;
    }
    hipLaunchKernelGGL(k_sir_coins, dim3(1), dim3(256), (size_t)2 * n, st, table_src, table_dst, (long)n_table, n, seeds,
                       n_seeds, beta, gamma, (long)sims, T, coins, (long)n_coins, counts, used);
    GN_LAUNCH_CHECK();
    long long h = 0;
    GN_HIP(hipMemcpyAsync(&h, used, sizeof(h), hipMemcpyDeviceToHost, st));
    GN_HIP(hipStreamSynchronize(st));
    *coins_used_host = h;
    if (h < 0) {
        gnode_set_error("gnode_sir_mc_coins: coin stream exhausted (n_coins=%lld)", (long long)n_coins);
        return GNODE_ERR_ARG;
    }
    return 0;
}
