// The output of the Monte-Carlo candidate sweep, one policy per output: what k_sir_philox and k_sir_frontier (gnode_sir.hip) put
// out for the C x sims jobs of gnode_sir_mc_philox_sweep and its three scored forms.  A kernel instance takes ONE policy type, OUT,
// and two arguments from it, the jobs (OUT::Jobs) and the policy; an instance that is not a sweep takes SirNoSweep, both empty.
// A policy states
//   Jobs        the type of the jobs argument: SirJobs, with the sums' two pointers behind them for SirSums, empty for SirNoSweep
//   SWEEP      the job loop, the start override, the schedule shift, and no [2][T][n] histogram (sir_hist_add)
//   ROWS        it puts out a row per closed step, for which the kernels keep the trajectory's totals (n_ever, n_rec)
//   CLOSES      closed() can end a job: the kernels call it only then, so that the other instances keep their code
//   LDS_INTS    the int32 of static LDS it keeps per workgroup; each kernel declares one array of them and hands it to every hook
//   LDS_AT_END  finish() reads that LDS: a kernel without a barrier of its own at the end of a job places one before the next reset
//   Job         what it carries through one job, in registers
//   reset       in front of the barrier that resets the kernel's counters
//   event<KIND> node v leaves S (KIND 0) or recovers (KIND 1) at step `it`: the one call at every site that holds an event
//   steps       the steps a job runs
//   row         the row of a step whose events lie behind a barrier, (n_ever, n_rec) being the kernel's own counters
//   closed      step `st` is closed by a barrier and the next step has not written to the state; false ends the job
//   finish      the end of a job, every event behind a barrier
// state_of(v) is 0 / 1 / 2 = S / I / R off the kernel's own state: the scan's byte, the frontier's two bitmaps.  The coins, the
// order of the jobs and every address below are the kernels' and the entries' (include/gnode.h); integer adds commute, so every
// output is exact whatever the order of the jobs.  The host half of each output is at the end (SirSumsOutput .. SirStrataOutput).
#pragma once
#include "gnode_common.h"
#include "gnode_sir_plan.h"

// The order of (c, s) within the job index.  0, the choice: candidates interleaved, c = j % C -- the workgroups resident at one
// time add to the sums of as many candidates as there are, and each workgroup's share of the jobs mixes the candidates.  1:
// candidate-major, c = j / sims, kept as a build option for the measurement of DESIGN 4.16.  No result depends on it.
#ifndef GN_SIR_SWEEP_MAJOR
#define GN_SIR_SWEEP_MAJOR 0
#endif
__device__ __forceinline__ void sir_sweep_job(long job, int C, long sims, int& c, long& s) {
    if (GN_SIR_SWEEP_MAJOR) { c = (int)(job / sims); s = job % sims; } else { c = (int)(job % C); s = job / C; }
}

// The jobs of a sweep (INIT and SCHED instances only): job j is candidate c = j % C and trajectory s = j / C (sir_sweep_job).
// Trajectory (c, s) draws the start of `sim` like every INIT instance and then overrides the node cand[c] -- action 0: it starts
// in I, action 1: in R; an id outside [0, n) matches no node -- and reads the phase row from shifts[c] on.  The coins do not know c.
// They are a kernel argument of their own in front of the policy, as SirInit and SirSched are (SirNoJobs, empty, in an instance
// that is not a sweep), and every hook that addresses an output takes them.  Two arguments, not one struct: with the same
// optimised IR, the backend reads the fields of ONE argument off one base in other groups, and the scored instances came out
// with another schedule and more lane spills, the timed frontier ones 0.3 % slower at fb-social size.
struct SirNoJobs {};
struct SirJobs { const int32_t* cand; const int32_t* shifts; int C; int action; };

// what a policy does not state
struct SirOutputDefaults {
    static constexpr bool SWEEP = true, ROWS = false, CLOSES = false, LDS_AT_END = false;
    static constexpr int LDS_INTS = 0;
    using Jobs = SirJobs;
    struct Job {};
    __device__ __forceinline__ void reset(int*, int, int, int) const {}
    template <int KIND> __device__ __forceinline__ void event(int*, int, int, int) const {}
    __device__ __forceinline__ int steps(int T) const { return T; }
    template <class J> __device__ __forceinline__ void row(J&, const int*, const SirJobs&, int, int, int, int, int, int, int) const {}
    template <class J, class StateOf> __device__ __forceinline__ bool closed(J&, int*, const SirJobs&, int, int, int, int, int, StateOf) const { return true; }
};
// every instance that is not a sweep: trajectories instead of jobs, the label outputs (hist, events, curves) of gnode_sir.hip
struct SirNoSweep : SirOutputDefaults { static constexpr bool SWEEP = false; using Jobs = SirNoJobs; };

// Outbreak sizes (gnode_sir_mc_philox_sweep): (S_t, I_t, R_t) added to sums[c][t] by integer atomics where a TRAJ instance writes
// a row of `curves` -- the rows after an early end repeat the final state -- and the number of nodes that were ever infected (the
// I starts included, the R starts not) in ever[c][s] when `ever` is non-null.
// The sums travel with the jobs in one argument, as the kernels have always read them (SirSumsJobs); the policy itself is empty.
struct SirSumsJobs : SirJobs {
    unsigned long long* sums;   // [C][T][3], accumulated
    uint32_t* ever;             // [C][sims], overwritten, or null
};
struct SirSums : SirOutputDefaults {
    using Jobs = SirSumsJobs;
    static constexpr bool ROWS = true;
    struct Job { int rec0 = 0; };                       // the R starts: they were never infected
    __device__ __forceinline__ void add(const Jobs& sw, int c, int T, int row, int n, int n_ever, int n_rec) const {
        unsigned long long* r = sw.sums + ((size_t)c * T + row) * 3;
        atomicAdd(&r[0], (unsigned long long)(n - n_ever)); atomicAdd(&r[1], (unsigned long long)(n_ever - n_rec));
        atomicAdd(&r[2], (unsigned long long)n_rec);
    }
    __device__ __forceinline__ void row(Job& jb, const int*, const Jobs& sw, int c, int T, int row, int n, int n_ever, int n_rec, int tid) const {
        if (row == 0) jb.rec0 = n_rec;
        if (tid == 0) add(sw, c, T, row, n, n_ever, n_rec);
    }
    template <class StateOf>
    __device__ __forceinline__ void finish(Job& jb, int*, const Jobs& sw, int c, long s, long sims, int T, int from, int n, int n_ever, int n_rec, int tid,
                                           int nthr, StateOf) const {
        for (int r = from + tid; r < T; r += nthr) add(sw, c, T, r, n, n_ever, n_rec);
        if (sw.ever && tid == 0) sw.ever[(size_t)c * sims + s] = (uint32_t)(n_ever - jb.rec0);
    }
};

// Source scores (gnode_sir_mc_philox_sweep_scores): each step of each job compared with O snapshots of the epidemic (obs,
// node-major int8 [n][O]: -1 not observed, 0 / 1 / 2 = S / I / R).  Two integer tallies per snapshot live in LDS and move with the
// events; an R start is both.  Where SirSums adds a row, thread o adds ONE to hist[o][c][row][k], k the binned similarity of the
// state with snapshot o:
//   measure 0, Jaccard:  lds[o] = inter = |left S & obs in {1, 2}|, lds[MAXO + o] = pos = |left S & observed|;
//                        k = inter * bins / (marked[o] + pos - inter), marked[o] = |obs in {1, 2}|
//   measure 1, match:    lds[o] = agree = |observed & obs == state|, from seen[o] - marked[o] (the zeros: everybody in S) on;
//                        k = agree * bins / seen[o], seen[o] = |observed|
// in 64-bit integer division, k = bins for a zero denominator: k = bins exactly when state and snapshot agree completely.
struct SirScores : SirOutputDefaults {
    const int8_t* obs; const int32_t* marked; const int32_t* seen; int O; int measure; int bins;
    unsigned long long* hist;   // [O][C][T][bins + 1], accumulated
    static constexpr bool ROWS = true, LDS_AT_END = true;
    static constexpr int LDS_INTS = 2 * GN_SIR_SCORE_MAXO;
    __device__ __forceinline__ void reset(int* tal, int, int tid, int) const {
        if (tid < 2 * GN_SIR_SCORE_MAXO) tal[tid] = (measure == 1 && tid < O) ? seen[tid] - marked[tid] : 0;
    }
    template <int KIND> __device__ __forceinline__ void event(int* tal, int, int v, int) const {
        if (KIND == 1 && measure == 0) return;                  // the Jaccard sets do not know a recovery
        const int8_t* ob = obs + (size_t)v * O;
        for (int o = 0; o < O; ++o) {
            const int x = ob[o];
            if (measure == 0) {
                if (x >= 0) { atomicAdd(&tal[GN_SIR_SCORE_MAXO + o], 1); if (x >= 1) atomicAdd(&tal[o], 1); }
            } else {
                const int d = KIND == 0 ? (x == 1) - (x == 0) : (x == 2) - (x == 1);
                if (d) atomicAdd(&tal[o], d);
            }
        }
    }
    // one trajectory's row `row` against snapshot o: its bin, counted
    __device__ __forceinline__ void cell(const int* tal, int C, int c, int T, int row, int o) const {
        unsigned long long num = (unsigned long long)tal[o], den;
        if (measure == 0) den = (unsigned long long)(marked[o] + tal[GN_SIR_SCORE_MAXO + o]) - num; else den = (unsigned long long)seen[o];
        const unsigned long long k = den ? num * (unsigned long long)bins / den : (unsigned long long)bins;
        atomicAdd(&hist[(((size_t)o * C + c) * T + row) * ((size_t)bins + 1) + k], 1ull);
    }
    __device__ __forceinline__ void row(Job&, const int* tal, const Jobs& sw, int c, int T, int row, int, int, int, int tid) const {
        if (tid < O) cell(tal, sw.C, c, T, row, tid);
    }
    // the rows after an early end repeat the final bin, spread over the threads as SirSums spreads its rows
    template <class StateOf>
    __device__ __forceinline__ void finish(Job&, int* tal, const Jobs& sw, int c, long, long, int T, int from, int, int, int, int tid, int nthr, StateOf) const {
        for (int r = from + tid; r < T; r += nthr)
            for (int o = 0; o < O; ++o) cell(tal, sw.C, c, T, r, o);
    }
};

// The records of timed evidence, as both policies below read them: those of node v are rec[rec_ptr[v] .. rec_ptr[v + 1]), one
// word each -- set | kind << 4 | min(back, T) << 8, back = -offset -- so that an event of a node without a record costs the two
// reads of rec_ptr (DESIGN 4.18 on why not a bitmap); zeros[o], the kind-0 records of set o, and records[o], its size.  For "now"
// = t steps after the run began a record (node v, offset d <= 0, kind) is read at model step m = t + d and is matched when: m < 0
// and the kind is 0; kind 0 / 1 / 2 and v is S / I / R at step m; kind 3 and v became infected AT step m; kind 4 and it recovered
// AT step m.
struct SirRecords { const int32_t* rec_ptr; const uint32_t* rec; const int32_t* zeros; const int32_t* records; };

// Source scores from timed evidence (gnode_sir_mc_philox_sweep_timed): each job compared at every age t with O sets of records
// jointly.  agree[o][t], the matched records of set o, is a sum of steps and pulses in t that begin at (event step + back): the
// LDS, int32 [O][T], holds its DIFFERENCES and moves with the events by LDS integer atomics; positions >= T are dropped:
//   v leaves S at step `it`:   kind 0: -1 at it + back;  kind 1: +1 at it + back;  kind 3: +1 at it + back, -1 at it + back + 1
//   v recovers at step `it`:   kind 1: -1 at it + back;  kind 2: +1 at it + back;  kind 4: +1 at it + back, -1 at it + back + 1
// from dif[o][0] = zeros[o] (everybody in S, for ever), and 0 elsewhere.  Nothing is put out per step.  When the trajectory has
// ended an inclusive prefix sum over t turns dif into agree, and the job adds ONE to hist[o][c][t][k], k = agree * bins /
// records[o] in integers, for every (o, t): k = bins exactly when every record of the set is matched.
struct SirTimedScores : SirOutputDefaults, SirRecords {
    int O; int bins;
    unsigned long long* hist;   // [O][C][T][bins + 1], accumulated
    static constexpr bool LDS_AT_END = true;
    static constexpr int LDS_INTS = GN_SIR_TIMED_CELLS;
    __device__ __forceinline__ void reset(int* dif, int T, int tid, int nthr) const {
        for (int i = tid, cells = O * T; i < cells; i += nthr) { const int o = i / T; dif[i] = i == o * T ? zeros[o] : 0; }
    }
    template <int KIND> __device__ __forceinline__ void event(int* dif, int T, int v, int it) const {
        for (int r = rec_ptr[v], end = rec_ptr[v + 1]; r < end; ++r) {
            const uint32_t w = rec[r];
            const int kind = (int)((w >> 4) & 7u), pos = it + (int)(w >> 8);
            const int d = KIND == 0 ? (kind == 1 || kind == 3) - (kind == 0) : (kind == 2 || kind == 4) - (kind == 1);
            if (d == 0 || pos >= T) continue;
            int* row = dif + (int)(w & 15u) * T;
            atomicAdd(&row[pos], d);
            if (kind == 3 + KIND && pos + 1 < T) atomicAdd(&row[pos + 1], -1);      // "at that step": a pulse, not a step
        }
    }
    // dif to agree (thread o takes set o: T dependent LDS adds, a step's worth of time at the end of T steps), a barrier, and the
    // O * T counts spread over the threads
    template <class StateOf>
    __device__ __forceinline__ void finish(Job&, int* dif, const Jobs& sw, int c, long, long, int T, int, int, int, int, int tid, int nthr, StateOf) const {
        if (tid < O) { int* row = dif + tid * T; int run = 0; for (int t = 0; t < T; ++t) { run += row[t]; row[t] = run; } }
        __syncthreads();
        for (int i = tid, cells = O * T; i < cells; i += nthr) {
            const int o = i / T, t = i - o * T;
            unsigned long long k = (unsigned long long)dif[i] * (unsigned long long)bins / (unsigned long long)records[o];
            if (k > (unsigned long long)bins) k = (unsigned long long)bins;   // (agree is in [0, records]: the count stays inside its row regardless)
            atomicAdd(&hist[(((size_t)o * sw.C + c) * T + t) * ((size_t)bins + 1) + k], 1ull);
        }
    }
};

// Nowcast and forecast from timed evidence (gnode_sir_mc_philox_sweep_posterior): each job compared with the records at ONE age,
// `now`, and counted by state where it agrees with all of a set's.  lds[o] is SirTimedScores' `dif` of set o SUMMED UP TO CELL
// `now` -- agree[o][now] -- kept as one number because the cell is known: from zeros[o] on, an event at step `it` of a node with
// a record (kind, back), pos = it + back, moves it by
//   v leaves S:   kind 0: -1 iff pos <= now;  kind 1: +1 iff pos <= now;  kind 3: +1 iff pos == now  (the pulse's two ends)
//   v recovers:   kind 1: -1 iff pos <= now;  kind 2: +1 iff pos <= now;  kind 4: +1 iff pos == now
// (back is staged as min(back, T) and now < T: a record at T or beyond never moves it).  No event after step `now` moves it, so
// behind the barrier that closes step `now` -- or behind the last step of a trajectory that ended before -- thread o < O
// compares lds[o] with records[o]: on equality the trajectory is ACCEPTED for set o, one is added to accepted[o][c], uint64
// [O][C], and bit o enters the job's mask, lds[MAXO].  An empty mask ends the job.  At every step now + horizons[j] that the job
// closes, and after its end for the horizons that are left (the final state stays), the workgroup walks the nodes, one lane
// per node, and adds one to counts[o][j][0][v] (v is I) or counts[o][j][1][v] (v is R), uint64 [O][H][2][n], for every set of
// the mask: a wave's adds to one plane are contiguous.  The job never steps past now + horizons[H - 1].
struct SirPosteriorCounts : SirOutputDefaults, SirRecords {
    const int32_t* horizons; int O, now, H;
    unsigned long long* counts;     // [O][H][2][n], accumulated
    unsigned long long* accepted;   // [O][C], accumulated
    static constexpr bool CLOSES = true, LDS_AT_END = true;
    static constexpr int LDS_INTS = GN_SIR_SCORE_MAXO + 1;
    struct Job { int last = 0, hj = 0; uint32_t acc = 0; };   // the last closed step, the next horizon, the sets that accept the job
    __device__ __forceinline__ int steps(int) const { return now + horizons[H - 1] + 1; }
    __device__ __forceinline__ void reset(int* agr, int, int tid, int) const {
        if (tid < GN_SIR_SCORE_MAXO) agr[tid] = tid < O ? zeros[tid] : 0;
        if (tid == 0) agr[GN_SIR_SCORE_MAXO] = 0;
    }
    template <int KIND> __device__ __forceinline__ void event(int* agr, int, int v, int it) const {
        for (int r = rec_ptr[v], end = rec_ptr[v + 1]; r < end; ++r) {
            const uint32_t w = rec[r];
            const int kind = (int)((w >> 4) & 7u), pos = it + (int)(w >> 8);
            const int step = KIND == 0 ? (kind == 1) - (kind == 0) : (kind == 2) - (kind == 1);
            const int d = pos <= now ? step + (pos == now && kind == 3 + KIND) : 0;
            if (d) atomicAdd(&agr[(int)(w & 15u)], d);
        }
    }
    // behind a barrier that follows every event up to step `now`: the sets that accept the job (the same word in every thread)
    __device__ __forceinline__ uint32_t accept(int* agr, int C, int c, int tid) const {
        uint32_t* mask = reinterpret_cast<uint32_t*>(agr + GN_SIR_SCORE_MAXO);
        if (tid < O && agr[tid] == records[tid]) { atomicOr(mask, 1u << tid); atomicAdd(&accepted[(size_t)tid * C + c], 1ull); }
        __syncthreads();
        return *mask;
    }
    // horizon j of an accepted job, off a state that nobody writes meanwhile
    template <class StateOf> __device__ __forceinline__ void count(uint32_t mask, int j, int n, int tid, int nthr, StateOf state_of) const {
        for (int v = tid; v < n; v += nthr) {
            const int st = state_of(v);
            if (st == 0) continue;
            for (uint32_t m = mask; m; m &= m - 1u) {
                const int o = __ffs((int)m) - 1;
                atomicAdd(&counts[(((size_t)o * H + j) * 2 + (st - 1)) * (size_t)n + v], 1ull);
            }
        }
    }
    template <class StateOf>
    __device__ __forceinline__ bool closed(Job& jb, int* agr, const Jobs& sw, int c, int st, int n, int tid, int nthr, StateOf state_of) const {
        jb.last = st;
        if (st == now) { jb.acc = accept(agr, sw.C, c, tid); if (!jb.acc) return false; }
        if (st >= now && jb.hj < H && now + horizons[jb.hj] == st) { count(jb.acc, jb.hj, n, tid, nthr, state_of); ++jb.hj; }
        return true;
    }
    // a job that ended before `now` is judged on its final state, which is its state at `now`, and the horizons that are left take
    // the final state, as SirSums' rows after an early end do
    template <class StateOf>
    __device__ __forceinline__ void finish(Job& jb, int* agr, const Jobs& sw, int c, long, long, int, int, int n, int, int, int tid, int nthr, StateOf state_of) const {
        if (jb.last < now) jb.acc = accept(agr, sw.C, c, tid);
        if (jb.acc) for (; jb.hj < H; ++jb.hj) count(jb.acc, jb.hj, n, tid, nthr, state_of);
    }
};

// Nowcast and forecast from evidence that may be wrong (gnode_sir_mc_philox_sweep_posterior_strata): SirPosteriorCounts with the
// accepted jobs kept apart by the number of records they MISS.  The records, the LDS (agree[o][now] per set and the mask word),
// reset, event, steps and the Job are the base's, unchanged; what is judged at step `now` is d = records[o] - lds[o] instead of
// equality.  With d <= M, M = mismatches in [0, GN_SIR_POST_MAXD), D = M + 1, the job is accepted for set o in STRATUM d: one is
// added to accepted[o][c][d], uint64 [O][C][D], and bit o enters the mask.  No event after step `now` moves lds[o] (pos >= it >
// now), so at every later horizon d is read off it again -- no LDS of its own -- and the walk of the nodes, one lane per node,
// adds to counts[o][d][j][st - 1][v], uint64 [O][D][H][2][n]: one set after the other, d and the plane's base found once per
// set in front of the walk, a wave's adds to one plane contiguous.  Stratum 0 is SirPosteriorCounts' output.
struct SirPosteriorStrata : SirPosteriorCounts {
    int M, D;                       // `counts` is [O][D][H][2][n] and `accepted` [O][C][D] here
    __device__ __forceinline__ uint32_t accept(int* agr, int C, int c, int tid) const {
        uint32_t* mask = reinterpret_cast<uint32_t*>(agr + GN_SIR_SCORE_MAXO);
        if (tid < O) {
            const int d = records[tid] - agr[tid];                 // (agree is in [0, records]: d < 0 cannot be, and accepts nothing)
            if (d >= 0 && d <= M) { atomicOr(mask, 1u << tid); atomicAdd(&accepted[((size_t)tid * C + c) * D + d], 1ull); }
        }
        __syncthreads();
        return *mask;
    }
    template <class StateOf> __device__ __forceinline__ void count(const int* agr, uint32_t mask, int j, int n, int tid, int nthr, StateOf state_of) const {
        for (uint32_t m = mask; m; m &= m - 1u) {
            const int o = __ffs((int)m) - 1, d = records[o] - agr[o];
            unsigned long long* plane = counts + (((size_t)o * D + d) * H + j) * 2 * (size_t)n;
            for (int v = tid; v < n; v += nthr) {
                const int st = state_of(v);
                if (st) atomicAdd(&plane[(size_t)(st - 1) * n + v], 1ull);
            }
        }
    }
    template <class StateOf>
    __device__ __forceinline__ bool closed(Job& jb, int* agr, const Jobs& sw, int c, int st, int n, int tid, int nthr, StateOf state_of) const {
        jb.last = st;
        if (st == now) { jb.acc = accept(agr, sw.C, c, tid); if (!jb.acc) return false; }
        if (st >= now && jb.hj < H && now + horizons[jb.hj] == st) { count(agr, jb.acc, jb.hj, n, tid, nthr, state_of); ++jb.hj; }
        return true;
    }
    template <class StateOf>
    __device__ __forceinline__ void finish(Job& jb, int* agr, const Jobs& sw, int c, long, long, int, int, int n, int, int, int tid, int nthr, StateOf state_of) const {
        if (jb.last < now) jb.acc = accept(agr, sw.C, c, tid);
        if (jb.acc) for (; jb.hj < H; ++jb.hj) count(agr, jb.acc, jb.hj, n, tid, nthr, state_of);
    }
};
// the launch plan and the workspace layouts count these bytes (gnode_sir_plan.h); the posterior's mask word comes on top, as it always has
static_assert(SirScores::LDS_INTS * sizeof(int32_t) == kSirScoreLds && SirTimedScores::LDS_INTS * sizeof(int32_t) == kSirTimedLds &&
              (SirPosteriorCounts::LDS_INTS - 1) * sizeof(int32_t) == kSirPostLds &&
              SirPosteriorStrata::LDS_INTS == SirPosteriorCounts::LDS_INTS, "the policies' static LDS is the plan's");

// --------------------------------------------------------------------------- the host half
// What the four entries share (include/gnode.h documents the arrays) ...
struct SirSweepCall {
    const char* who; gnode_graph_t g;
    const double* init; const int32_t *cand, *shifts; int32_t C, action; const int32_t* phase; int32_t P, L; const double *w, *gamma;
    int64_t sims, sim_offset; int32_t T; uint64_t rng_seed; void* workspace; size_t workspace_bytes; void* stream; int32_t edge_scan;
};
#define SIR_SWEEP_SHAPE(c) (c).g->info.n, (c).g->nnz, (c).g->n_bigrow, (c).T, (c).P, (c).L, (c).C                                             // a layout's arguments
#define SIR_SWEEP_INPUT(c) (c).who, (c).g->info.n, (c).g->nnz, (c).T, (c).P, (c).L, (c).phase, (c).w, (c).gamma, (c).init, (c).C, (c).shifts   // a staging's
// ... and what each adds, one description per output for sir_sweep_impl (gnode_sir.hip): its policy, the static LDS the launch
// plan counts, whether a bad argument is refused before a short workspace (the plain sweep has always asked about the
// workspace first), that no array is missing, its layout, its staging (gnode_sir_plan.h; Staged has thr and uploads(layout)),
// and the filling of the policy's own fields -- the jobs' are the call's.
struct SirSumsOutput {
    using Policy = SirSums; using Layout = SirSweepLayout;
    struct Staged { SirThresholds thr; std::vector<SirUpload> uploads(const Layout&) const { return {}; } };
    static constexpr size_t static_lds = 0; static constexpr bool args_first = false;
    uint64_t* sums; uint32_t* ever;
    bool complete() const { return sums != nullptr; }
    Layout layout(const SirSweepCall& c) const { return sir_sweep_layout(SIR_SWEEP_SHAPE(c)); }
    Staged stage(const SirSweepCall& c) const { return {sir_stage_sweep(SIR_SWEEP_INPUT(c))}; }
    void fill(SirSumsJobs& sw, Policy&, char*, const Layout&) const { sw.sums = (unsigned long long*)sums; sw.ever = ever; }
};
struct SirScoresOutput {
    using Policy = SirScores; using Layout = SirScoreLayout; using Staged = SirScoreStaged;
    static constexpr size_t static_lds = kSirScoreLds; static constexpr bool args_first = true;
    const int8_t* obs; int32_t O, measure, bins; uint64_t* hist;     // the snapshots as the caller holds them, int8 [O][n]
    bool complete() const { return obs && hist; }
    Layout layout(const SirSweepCall& c) const { return sir_score_layout(SIR_SWEEP_SHAPE(c), O); }
    Staged stage(const SirSweepCall& c) const { return sir_stage_score(SIR_SWEEP_INPUT(c), obs, O, measure, bins); }
    void fill(SirJobs&, Policy& o, char* ws, const Layout& W) const {
        o.obs = (const int8_t*)(ws + W.obs); o.marked = (const int32_t*)(ws + W.marked); o.seen = (const int32_t*)(ws + W.seen);
        o.O = O; o.measure = measure; o.bins = bins; o.hist = (unsigned long long*)hist;
    }
};
// the R records of a timed call as four host arrays, and where they are staged
struct SirRecordArrays {
    const int32_t *set, *node, *offset, *kind; int32_t R, O;
    bool complete() const { return R < 1 || (set && node && offset && kind); }
    void fill(SirRecords& r, char* ws, const SirTimedLayout& W) const {
        r.rec_ptr = (const int32_t*)(ws + W.rec_ptr); r.rec = (const uint32_t*)(ws + W.rec); r.zeros = (const int32_t*)(ws + W.zeros);
        r.records = (const int32_t*)(ws + W.records);
    }
};
#define SIR_RECORD_INPUT(r) (r).set, (r).node, (r).offset, (r).kind, (r).R, (r).O
struct SirTimedOutput {
    using Policy = SirTimedScores; using Layout = SirTimedLayout; using Staged = SirTimedStaged;
    static constexpr size_t static_lds = kSirTimedLds; static constexpr bool args_first = true;
    SirRecordArrays rec; int32_t bins; uint64_t* hist;
    bool complete() const { return hist && rec.complete(); }
    Layout layout(const SirSweepCall& c) const { return sir_timed_layout(SIR_SWEEP_SHAPE(c), rec.O, rec.R); }
    Staged stage(const SirSweepCall& c) const { return sir_stage_timed(SIR_SWEEP_INPUT(c), SIR_RECORD_INPUT(rec), bins); }
    void fill(SirJobs&, Policy& o, char* ws, const Layout& W) const { rec.fill(o, ws, W); o.O = rec.O; o.bins = bins; o.hist = (unsigned long long*)hist; }
};
struct SirPosteriorOutput {
    using Policy = SirPosteriorCounts; using Layout = SirPostLayout; using Staged = SirPostStaged;
    static constexpr size_t static_lds = kSirPostLds; static constexpr bool args_first = true;
    SirRecordArrays rec; int32_t now; const int32_t* horizons; int32_t H; uint64_t *counts, *accepted;
    bool complete() const { return counts && accepted && rec.complete() && (H < 1 || horizons); }
    Layout layout(const SirSweepCall& c) const { return sir_post_layout(SIR_SWEEP_SHAPE(c), rec.O, rec.R, H); }
    Staged stage(const SirSweepCall& c) const { return sir_stage_post(SIR_SWEEP_INPUT(c), SIR_RECORD_INPUT(rec), now, horizons, H); }
    void fill(SirJobs&, Policy& o, char* ws, const Layout& W) const {
        rec.fill(o, ws, W); o.horizons = (const int32_t*)(ws + W.horizons); o.O = rec.O; o.now = now; o.H = H;
        o.counts = (unsigned long long*)counts; o.accepted = (unsigned long long*)accepted;
    }
};
// the posterior's arrays and workspace; `mismatches` sizes only the caller's two outputs
struct SirStrataOutput {
    using Policy = SirPosteriorStrata; using Layout = SirPostLayout; using Staged = SirPostStaged;
    static constexpr size_t static_lds = kSirPostLds; static constexpr bool args_first = true;
    SirPosteriorOutput post; int32_t mismatches;
    bool complete() const { return post.complete(); }
    Layout layout(const SirSweepCall& c) const { return post.layout(c); }
    Staged stage(const SirSweepCall& c) const {
        return sir_stage_strata(SIR_SWEEP_INPUT(c), SIR_RECORD_INPUT(post.rec), post.now, post.horizons, post.H, mismatches);
    }
    void fill(SirJobs& sw, Policy& o, char* ws, const Layout& W) const { post.fill(sw, o, ws, W); o.M = mismatches; o.D = mismatches + 1; }
};
// f(policy) for every output: what registers the instances (gn_sir_set_attributes)
template <class F> static void sir_each_output(F&& f) { f(SirSums{}); f(SirScores{}); f(SirTimedScores{}); f(SirPosteriorCounts{}); f(SirPosteriorStrata{}); }
