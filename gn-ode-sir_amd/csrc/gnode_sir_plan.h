// The host side of the Monte-Carlo SIR calls that never touches the device, each stated once: where every array of a call sits
// in the caller's workspace (sir_layout), which kernel path a call takes with what geometry (sir_launch_plan), and the coin
// thresholds staged from the caller's rates and start distribution (sir_stage).  Plain C++, like gnode_graph_plan.h:
// tests/test_sir_plan.py compiles this unit with the system compiler and pins it to the commit before it existed.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

static const size_t kLdsStateLimit = 150 * 1024;   // of the CU's 160 KiB
static const int kFrontierGlobalGrid = 1024;       // workgroups that own a set of global lists (graphs past the LDS form)

enum { SIR_SCALAR = 0, SIR_NODES = 1, SIR_EDGES = 2, SIR_INIT = 3 };   // rate forms (the kernels' NODES / EDGES instances); SIR_INIT only indexes SirLayout::bytes

// Byte offsets into a call's workspace (each 256-byte aligned), and what each form needs of it.
struct SirLayout {
    size_t hist, seeds;   // uint32 [2][T][n] event histograms (up to `seeds`), int32 [4096] seed ids
    size_t rows;       // int32 [max(nnz, 1)]: the counted call's tally; the rest is unused (the scan's row expansion lay here, it is
                       // the handle's src now) and stays because the workspace sizes are pinned
    size_t tail;       // one region, two users that never run together: the scan's state in memory (2048 x 2n bytes, n past the
                       // LDS state) and the frontier's global lists (kFrontierGlobalGrid x 3n int32, lists past the LDS form)
    size_t thr;        // uint64 rate thresholds: [n beta | n gamma] per node, [nnz entries | n gamma] per edge
    size_t start;      // uint64 [2][n] start thresholds thr(pS) | thr(pR): behind the per-edge form, the largest of the rate forms'
    size_t bytes[4];   // the workspace of SIR_SCALAR (= thr), SIR_NODES, SIR_EDGES (= start) and SIR_INIT
};
// static_lds, wherever it appears: the static LDS an instance keeps beyond the few counters all of them have -- what the scored
// sweeps' output policies hold there (kSirScoreLds, kSirTimedLds, kSirPostLds below; 0 for the plain sweep and for every instance
// that is not a sweep).  It moves the boundary of the lists-in-LDS form and of the scan's state in LDS, and with them the size of
// `tail`, and it counts in the workgroups per CU.
SirLayout sir_layout(int n, int64_t nnz, int n_bigrow, int T, size_t static_lds = 0);

// LDS of the frontier kernel: bitmaps + 1 KB of coin queue per wave (+ three uint16 node lists when they fit: n <= 11 232 without long rows)
bool frontier_lists_in_lds(int n, int n_big, size_t static_lds = 0);
size_t frontier_lds_bytes(int n, int n_big, int threads, size_t static_lds = 0);   // the dynamic bytes
int frontier_threads(int n, int n_big, int* per_cu_out, size_t static_lds = 0);   // workgroup size, and workgroups per CU

enum SirPath { SIR_FRONTIER_LDS, SIR_FRONTIER_MEM /* lists in the workspace */, SIR_SCAN_LDS, SIR_SCAN_MEM /* state in the workspace */ };
struct SirLaunch { SirPath path; int threads, grid; size_t lds; };
SirLaunch sir_launch_plan(int n, int n_bigrow, int num_cu, int64_t sims, bool edge_scan, size_t static_lds = 0);
unsigned long long coin_threshold(double p);   // a coin fires iff (64-bit) word < thr, thr = floor(p * 2^32) in [0, 2^32]

// The rates of a call, on the host.  SIR_SCALAR: beta, gamma.  SIR_NODES: beta_nodes, gamma_nodes, fp64 [n] each.  SIR_EDGES:
// w_edges, fp64 [nnz] in CSR position order, with gamma_nodes or (when that is null) the scalar gamma for every node.
struct SirRates { int form = SIR_SCALAR; double beta = 0.0, gamma = 0.0; const double *beta_nodes = nullptr, *gamma_nodes = nullptr, *w_edges = nullptr; };
struct SirThresholds {
    std::string error;                         // non-empty: an input was refused; names `who` and the first offending index
    unsigned long long tb = 0, tg = 0;         // SIR_SCALAR
    std::vector<unsigned long long> rates;     // [infection thresholds: n or nnz | n recovery thresholds]; empty for SIR_SCALAR
    std::vector<unsigned long long> start;     // [n thr(pS) | n thr(pR)]; empty without `init`
};
// Every range, NaN and row-sum check of the host arrays is here.  restate_col (non-null, with SIR_NODES): the column ids of the
// CSR; the per-node rates are then staged as the per-edge form's, thr[p] = thr(beta[col[p]]) -- same coins, same counts.
// init: null, or fp64 [n][3], (pS, pI, pR) per node.
SirThresholds sir_stage(const char* who, int n, int64_t nnz, const SirRates& r, const int32_t* restate_col, const double* init);

// Rates that change over time (gnode_sir_mc_philox_schedule): P >= 1 phases of the per-edge form, phase[t] in [0, P) naming the
// tables that govern step t = 1 .. T-1.  The layout is sir_layout's with the threshold region grown to P tables -- uint64
// [P][nnz] infection thresholds, then uint64 [P][n] recovery thresholds, so that a step's tables are thr + phase * nnz and
// thr_gamma + phase * n -- the start thresholds behind it, and the int32 [T] phase table last.
struct SirScheduleLayout : SirLayout {   // hist .. tail are sir_layout's; thr is too; start moves behind the P tables
    size_t phase;      // int32 [T]
    size_t total;      // the workspace of the scheduled call
};
SirScheduleLayout sir_schedule_layout(int n, int64_t nnz, int n_bigrow, int T, int P, size_t static_lds = 0);
// Every check of the schedule is here: P >= 1, phase[1 .. T-1] in [0, P) (entry 0 is never read), every weight of w [P][nnz]
// and every rate of gamma [P][n] a probability (a NaN fails), the start as sir_stage checks it.  A refusal names `who`, the
// phase and the position.  rates = [P * nnz infection thresholds | P * n recovery thresholds].
SirThresholds sir_stage_schedule(const char* who, int n, int64_t nnz, int T, int P, const int32_t* phase, const double* w, const double* gamma,
                                 const double* init);

// Outbreak sizes for many candidates in one launch (gnode_sir_mc_philox_sweep): C x sims trajectories of the drawn-start
// scheduled form, candidate c reading the phase row from shifts[c] on.  No histogram and no seed list: the layout is
// sir_schedule_layout's from `rows` on -- rows, tail, the P tables, the start thresholds -- then the int32 [L] phase row, the
// int32 [C] candidate ids and the int32 [C] shifts.
struct SirSweepLayout {
    size_t rows, tail, thr, start;   // as in SirScheduleLayout, moved down by the histogram and the seed list
    size_t phase;                    // int32 [L]
    size_t cand, shifts;             // int32 [C] each
    size_t total;                    // the workspace of the sweep
};
SirSweepLayout sir_sweep_layout(int n, int64_t nnz, int n_bigrow, int T, int P, int L, int C);
// The sweep's checks, then sir_stage_schedule over the whole phase row (T = L there): L >= T; every shift (shifts may be null:
// all 0) is >= 0 with shift + T <= L; phase[1 .. L-1] in [0, P).  A refusal names `who` and the offending index.
SirThresholds sir_stage_sweep(const char* who, int n, int64_t nnz, int T, int P, int L, const int32_t* phase, const double* w,
                              const double* gamma, const double* init, int C, const int32_t* shifts);
// One staged array of a call on its way to the device: `bytes` from `from` go to the workspace offset `at`.  What a scored sweep
// staged beyond the thresholds is a list of these (uploads() below), so that the call copies them without knowing the output.
struct SirUpload { size_t at; const void* from; size_t bytes; };

// Monte-Carlo source scores (gnode_sir_mc_philox_sweep_scores, the SCORE instances): the sweep's trajectories, each step of each
// compared with O snapshots.  At most GN_SIR_SCORE_MAXO snapshots per call: the kernels keep two int32 tallies per snapshot in
// static LDS, kSirScoreLds bytes that the launch plan and the layout below count (static_lds above).
#ifndef GN_SIR_SCORE_MAXO
#define GN_SIR_SCORE_MAXO 16
#endif
static const size_t kSirScoreLds = (size_t)2 * GN_SIR_SCORE_MAXO * sizeof(int32_t);
// The sweep's layout (its `tail` sized for the SCORE instances' boundaries), then the snapshots staged node-major, int8 [n][O],
// and the two int32 [O] denominator tables: marked[o], the nodes of snapshot o with code 1 or 2 (the Jaccard measure's |A_o|),
// and seen[o], its observed nodes (the match measure's denominator; seen - marked is its number of zeros).
struct SirScoreLayout : SirSweepLayout {
    size_t obs;                      // int8 [n][O]
    size_t marked, seen;             // int32 [O] each
};
SirScoreLayout sir_score_layout(int n, int64_t nnz, int n_bigrow, int T, int P, int L, int C, int O);
// sir_stage_sweep's checks and those of the snapshots (obs: int8 [O][n] as the caller holds them): 1 <= O <= GN_SIR_SCORE_MAXO,
// bins in [1, 4096], measure 0 or 1, O * C * T * (bins + 1) < 2^31, every code in [-1, 2], every snapshot observing a node.  A
// refusal (thr.error) names `who` and the offending index, and nothing is staged.
struct SirScoreStaged {
    SirThresholds thr;
    std::vector<int8_t> obs;         // [n][O]
    std::vector<int32_t> marked, seen;
    std::vector<SirUpload> uploads(const SirScoreLayout& W) const;
};
SirScoreStaged sir_stage_score(const char* who, int n, int64_t nnz, int T, int P, int L, const int32_t* phase, const double* w,
                               const double* gamma, const double* init, int C, const int32_t* shifts, const int8_t* obs, int O, int measure,
                               int bins);

// Monte-Carlo source scores from timed evidence (gnode_sir_mc_philox_sweep_timed, the TIMED instances): the sweep's trajectories,
// each compared at every age t with the records (node, offset <= 0, kind 0 .. 4) of O evidence sets, at most GN_SIR_SCORE_MAXO per
// call.  The kernels keep a difference array over t, int32 [O][T], in static LDS: GN_SIR_TIMED_CELLS int32 -- 2 048, 8 KiB, so
// 16 sets up to T = 128 and one set up to T = 2 048 -- which the launch plan and the layout below count as kSirTimedLds
// (static_lds above: the lists-in-LDS form ends at n = 9 352 instead of 11 232 with it).
#ifndef GN_SIR_TIMED_CELLS
#define GN_SIR_TIMED_CELLS 2048
#endif
static const size_t kSirTimedLds = (size_t)GN_SIR_TIMED_CELLS * sizeof(int32_t);
// The sweep's layout (its `tail` sized for the TIMED instances' boundaries), then the records staged by node: rec_ptr, and one
// word per record -- set | kind << 4 | min(-offset, T) << 8 -- in ascending node order, the records of one node in the order
// they were given; then zeros[o], the records of kind 0 of set o, and records[o], its size.
struct SirTimedLayout : SirSweepLayout {
    size_t rec_ptr;                  // int32 [n + 1]
    size_t rec;                      // uint32 [R]
    size_t zeros, records;           // int32 [O] each
};
SirTimedLayout sir_timed_layout(int n, int64_t nnz, int n_bigrow, int T, int P, int L, int C, int O, int R);
// sir_stage_sweep's checks and those of the records (four arrays of length R): 1 <= O <= GN_SIR_SCORE_MAXO, O * T <=
// GN_SIR_TIMED_CELLS, bins in [1, 4096], O * C * T * (bins + 1) < 2^31, R >= 1, every set in [0, O), node in [0, n), kind in
// [0, 4] and offset <= 0, every set holding a record.  A refusal (thr.error) names `who` and the offending index, and nothing
// is staged.
struct SirTimedStaged {
    SirThresholds thr;
    std::vector<int32_t> rec_ptr;    // [n + 1]
    std::vector<uint32_t> rec;       // [R]
    std::vector<int32_t> zeros, records;
    std::vector<SirUpload> uploads(const SirTimedLayout& W) const;
};
SirTimedStaged sir_stage_timed(const char* who, int n, int64_t nnz, int T, int P, int L, const int32_t* phase, const double* w,
                               const double* gamma, const double* init, int C, const int32_t* shifts, const int32_t* rec_set,
                               const int32_t* rec_node, const int32_t* rec_offset, const int32_t* rec_kind, int R, int O, int bins);

// Nowcast and forecast from timed evidence (gnode_sir_mc_philox_sweep_posterior, the POST instances): the sweep's trajectories,
// each compared with the records of O evidence sets, at most GN_SIR_SCORE_MAXO per call, at ONE age `now`, and the states of the
// accepted ones counted at now + horizons[j], at most GN_SIR_POST_MAXH horizons.  The kernels keep one int32 per set in static
// LDS -- the difference array summed up to cell `now` -- kSirPostLds bytes for the launch plan and the layout below (static_lds
// above); no O * T limit applies.
#ifndef GN_SIR_POST_MAXH
#define GN_SIR_POST_MAXH 32
#endif
#ifndef GN_SIR_POST_MAXD
#define GN_SIR_POST_MAXD 8           // the strata of sir_stage_strata, below
#endif
static const size_t kSirPostLds = (size_t)GN_SIR_SCORE_MAXO * sizeof(int32_t);
// SirTimedLayout (its `tail` sized for the POST instances' boundaries), then the horizons.
struct SirPostLayout : SirTimedLayout {
    size_t horizons;                 // int32 [H]
};
SirPostLayout sir_post_layout(int n, int64_t nnz, int n_bigrow, int T, int P, int L, int C, int O, int R, int H);
// sir_stage_sweep's checks and those of the records as sir_stage_timed makes them (one record sort for both), without the cells
// of a difference array: 1 <= O <= GN_SIR_SCORE_MAXO, `now` in [0, T), 1 <= H <= GN_SIR_POST_MAXH, horizons[0] >= 0, ascending,
// now + horizons[j] <= T - 1, O * H * 2 * n < 2^31, R >= 1 and every record as there.  A refusal (thr.error) names `who` and the
// offending index, and nothing is staged.
struct SirPostStaged : SirTimedStaged {
    std::vector<int32_t> horizons;   // [H]
    std::vector<SirUpload> uploads(const SirPostLayout& W) const;
};
SirPostStaged sir_stage_post(const char* who, int n, int64_t nnz, int T, int P, int L, const int32_t* phase, const double* w,
                             const double* gamma, const double* init, int C, const int32_t* shifts, const int32_t* rec_set,
                             const int32_t* rec_node, const int32_t* rec_offset, const int32_t* rec_kind, int R, int O, int now,
                             const int32_t* horizons, int H);

// The posterior by the number of missed records (gnode_sir_mc_philox_sweep_posterior_strata, the STRATA instances): a trajectory
// that misses d <= mismatches records of a set is accepted for it in stratum d, at most GN_SIR_POST_MAXD strata.  The workspace,
// the layout and the LDS are the posterior's: the strata size only the caller's outputs, counts [O][D][H][2][n] and accepted
// [O][C][D], D = mismatches + 1.  sir_stage_post's checks and staging, and two more in front of the records': mismatches in
// [0, GN_SIR_POST_MAXD - 1] and O * D * H * 2 * n < 2^31.
SirPostStaged sir_stage_strata(const char* who, int n, int64_t nnz, int T, int P, int L, const int32_t* phase, const double* w,
                               const double* gamma, const double* init, int C, const int32_t* shifts, const int32_t* rec_set,
                               const int32_t* rec_node, const int32_t* rec_offset, const int32_t* rec_kind, int R, int O, int now,
                               const int32_t* horizons, int H, int mismatches);
