// What a graph handle holds, computed on the host: every index structure the kernels walk (gn_plan_graph) and the per-call
// plans of the persistent launches.  Plain C++ -- nothing here touches the device, so tests/test_graph_plan.py compiles this
// unit with the system compiler and pins every array; gnode_graph_create (gnode_ode.hip) uploads the vectors as they are.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#ifndef GN_SIR_BIGROW
#define GN_SIR_BIGROW 512     // Monte-Carlo frontier kernel: rows longer than this are walked by the whole workgroup
#endif
#define HUB_SEG 32           // a hub row's neighbour list is cut into segments of this many edges
#ifndef GN_HUB_T
#define GN_HUB_T 96          // rows longer than this are hubs (measured break-even against the two extra launches per step)
#endif
#define PERS_FLAG_WORDS 2048   // barrier flags in the persistent launches' control block
#define PERS_MAX_ITEMS 8       // segment sums one lane group of k_pers64 may be given
#define PERS_MAX_PARTIALS 128  // partial-sum slots (256 B each) a k_pers64 workgroup may need for its hub rows
#define BWD_NWG 768            // partial-gradient slots of a backward call: 3 workgroups per CU (52 KB of LDS each) on 256 CUs
static const int kPersMaxRows = 256 * 64;   // k_pers64's one resident grid: 256 workgroups x 64 rows

// k_pers64 / k_pers_bwd64 with 16 << i rows per workgroup.  Slot s of `map` = lane group (s % rows) of workgroup s / rows.
struct GnPers64Maps {
    bool present = false;          // false: the graph never takes this variant (too many rows, or its hub rows need too many slots)
    std::vector<int32_t> map;      // per lane-group slot the node it owns, -1 for padding slots
    // hub rows (longer than GN_HUB_T):
    std::vector<int32_t> hub;      // per slot {first partial slot in the workgroup's LDS, segments} of the hub row it owns (-1, 0 otherwise)
    std::vector<int32_t> segptr;   // per slot {first item, items} of the segment sums it computes each step
    std::vector<int32_t> items;    // {first CSR position, one past the last, partial slot, 0}
    int32_t lds = 0;               // the most partial slots one workgroup needs
    int32_t max_items = 0;         // the most items one lane group has
};

struct GnGraphPlan {
    std::string error;             // non-empty: the CSR was refused (nothing else is filled in)
    int32_t max_degree = 0;
    int32_t n_bigrow = 0;          // rows longer than GN_SIR_BIGROW (their list's capacity in the Monte-Carlo kernel)
    std::vector<int32_t> rowhdr;   // [n][20]: {start, end, 0, 0, first 16 column ids (0-padded)} -- the H = 64 step kernel gets a
                                   // row's extent AND its first 16 neighbour ids in ONE round trip instead of two dependent ones
    // hub rows, cut into <= HUB_SEG-edge segments (gnode_hub.hip); all four empty when n_hub == 0
    int32_t n_hub = 0, n_seg = 0;
    std::vector<int32_t> hubidx;        // [n]: hub index of a row, -1 for ordinary rows
    std::vector<int32_t> seg_lo;        // [n_seg]: first CSR position of a segment
    std::vector<int32_t> seg_hi;        // [n_seg]: one past its last
    std::vector<int32_t> hub_seg_ptr;   // [n_hub+1]: segments of hub h are [ptr[h], ptr[h+1])
    GnPers64Maps pers[3];
    // k_persg / k_persg_bwd (H = 8 / 16 / 32 x workgroups of 1 .. 4 waves): lane-group slot -> node (-1 padding), all variants
    // in one array at pgoff[][] (-1: variant absent); per variant the most neighbour ids of ordinary rows and the most hub
    // segments one workgroup has to stage in LDS
    std::vector<int32_t> pgmap;
    int32_t pgoff[3][4], pgids[3][4], pgsegs[3][4];
    // edge tables of the DMP, mean-field and Monte-Carlo scan kernels, per CSR position p
    std::vector<int32_t> src;      // [nnz]: the row p lies in
    std::vector<int32_t> rev;      // [nnz]: the position of the opposite entry (col[p], src[p]), -1 where the pattern has none;
                                   // a self-loop is its own reverse.  Defined by a binary search that takes a row's columns
                                   // to ascend; in a row that does not it is whatever that search finds, as it always was
    bool symmetric = true;         // no rev entry is -1 (true for nnz == 0)
};

// Checks the CSR (monotone rowptr from 0 to nnz, col in [0, n)) and plans it.  rowptr [n+1], col [nnz], n >= 1.
GnGraphPlan gn_plan_graph(const int32_t* rowptr, const int32_t* col, int32_t n, int64_t nnz);

// The host scalars of a handle that the per-call planners read.
struct GnGraphInfo {
    int32_t n;
    int32_t num_cu;                // compute units of the handle's device: persistent grids are sized from the handle
    int32_t n_hub;
    bool pers[3];                  // GnPers64Maps::present
    int32_t persitems[3];          // GnPers64Maps::max_items
    int32_t pgoff[3][4], pgids[3][4], pgsegs[3][4];
};
GnGraphInfo gn_graph_info(const GnGraphPlan& plan, int32_t n, int32_t num_cu);

// How the workgroups of one k_pers64 launch are dealt to samples.  A "group" = the workgroups that own one sample's rows:
//   nt          16-row tiles per workgroup (blockDim = 256 * nt); wgs = ceil(n / (16 nt)) workgroups per group
//   span == 1   a group sits on ONE XCD, gpx groups side by side on each XCD (tickets [gi * wgs, (gi + 1) * wgs))
//   span  > 1   a group takes `span` whole XCDs, `per` tickets on each
//   concurrent  groups alive at once (>= B: one round)
struct PersPlan { int nt, wgs, span, gpx, per, slots, n_xcc, rounds, concurrent, fstride; };
// false: this (graph, batch, horizon) does not take the persistent path (too many rows for one resident grid, ...)
bool gn_pers64_plan(const GnGraphInfo& g, long B, int n_steps, PersPlan* p);
bool gn_pers_bwd64_plan(const GnGraphInfo& g, long B, int n_steps, PersPlan* p);

struct PersgPlan { int wgs, wps, nw, map_off, idcap, segcap; size_t lds; };   // nw: waves per workgroup (64 / LPR rows each)
// false: this (graph, rows, H, horizon) keeps the one-launch-per-step forms (more rows than one resident grid of one workgroup
// per CU holds, a window of rows whose neighbour ids / hub segments do not fit a workgroup's LDS, other hidden sizes)
bool gn_persg_plan(const GnGraphInfo& g, long rows, int H, int n_steps, PersgPlan* p);
// dynamic LDS of k_persg / k_persg_bwd (the carve-up is pg_carve, gnode_persg.hip)
size_t pg_lds_bytes(int H, int idcap, int segcap);
