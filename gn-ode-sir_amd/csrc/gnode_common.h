// Shared host-side helpers of libgnode_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstdint>
#include <vector>
#include "gnode.h"
#include "gnode_graph_plan.h"

// The device copy of a graph's plan (gnode_graph_plan.h defines and documents every array; gnode_graph_create uploads them).
struct gnode_graph_s {
    GnGraphInfo info;   // n, num_cu, n_hub and the other host scalars the per-call planners read
    int64_t nnz;
    int32_t max_degree, n_bigrow, n_seg;
    int32_t device;     // the HIP device the arrays live on (current device at gnode_graph_create)
    int32_t* rowptr;    // [n+1]
    int32_t* col;       // [nnz]
    int32_t *src, *rev; // [nnz] each: the row of a CSR position and the position of its opposite entry
    bool symmetric;     // every entry has its opposite: DMP and the weighted mean-field serve such graphs only
    int32_t* rowhdr;
    int32_t *hubidx, *seg_lo, *seg_hi, *hub_seg_ptr;     // null when n_hub == 0
    int32_t *persmap[3], *pershub[3], *perssegptr[3], *perssegitem[3];   // GnPers64Maps, null for an absent variant
    int32_t perslds[3];
    int32_t* pgmap;     // null when no k_persg variant exists
    std::vector<void*> owned;   // every device allocation of the handle: the pointers above point into these
};

// Hub sums of `ntables` (1 or 2) tables for a batch of B samples need this much of the CALLER's workspace (0 for a graph
// without hub rows); gn_hub_gather carves its segment partials and hub sums from it: no allocation, no
// synchronisation, nothing retained in the handle.
size_t gn_hub_scratch_bytes(const gnode_graph_s* g, long B, int H, int ntables);
int gn_hub_gather(const gnode_graph_s* g, long B, int H, const float* T0, const float* T1, void* scratch, const float** A0,
                  const float** A1, hipStream_t st);
int gn_hub_segments(const gnode_graph_s* g, long B, int H, const float* T0, void* scratch, const float** P0, hipStream_t st);
int gn_hub_segments2(const gnode_graph_s* g, long B, int H, const float* T0, const float* T1, void* scratch, const float** P0,
                     const float** P1, hipStream_t st);

// per-device one-time setup (dynamic-LDS attributes of every kernel that may need more than 64 KB), run by
// gnode_graph_create for the current device; each translation unit contributes its kernels
int gn_device_setup_once(int dev);      // idempotent, locked; returns a gnode_status
int gn_ode_set_attributes();
int gn_bwd_set_attributes();
int gn_bwd_tiny_set_attributes();
int gn_sir_set_attributes();
int gn_dmp_set_attributes();
int gn_dmp_schedule_set_attributes();
int gn_dmp_schedule_bwd_set_attributes();
int gn_dmp_source_set_attributes();
int gn_dmp_source_batch_set_attributes();
int gn_dmp_source_events_set_attributes();
int gn_dmp_outbreak_set_attributes();
int gn_dmp_source_events_schedule_set_attributes();
int gn_dmp_outbreak_schedule_set_attributes();
int gn_rhs_vjp_set_attributes();

// The training forward's KEPT ACTIVATIONS (H = 64): per grid point k three tables of rows + 1 rows of 64 floats --
//   Z_S(y_k); Z_I(y_k); P_S(y_k) = (A Z_I(y_k)) * Z_S(y_k) * (1 - Z_S(y_k)).
// Z_I(y_k) IS step k's gather table (the row behind it is the table's zero row), so keeping it costs the forward nothing;
// Z_S and P_S are one streamed slab each per step (P_S takes the place of the A Z_I row a forward without `keep` parks in the
// trajectory's 4th slab).  The adjoint backward reads them back instead of gathering a second table and recomputing three
// 64x64 products and 192 sigmoids per row and interval; P_S is the ONLY form in which it needs A Z_I, so it reads one slab
// row where A Z_I and Z_S(y_i) would be two.  The one-launch (tiny-graph) forms keep and use Z_S, Z_I only.
__host__ __device__ static inline size_t gn_keep_stride(long rows) { return ((size_t)rows + 1) * 64; }
static inline size_t gn_keep_floats(long rows, int n_steps) { return (size_t)3 * (n_steps + 1) * gn_keep_stride(rows); }
template <class T> __host__ __device__ static inline T* gn_keep_zs(T* keep, long rows, int k) { return keep + (size_t)(3 * k) * gn_keep_stride(rows); }
template <class T> __host__ __device__ static inline T* gn_keep_zi(T* keep, long rows, int k) { return keep + (size_t)(3 * k + 1) * gn_keep_stride(rows); }
template <class T> __host__ __device__ static inline T* gn_keep_ps(T* keep, long rows, int k) { return keep + (size_t)(3 * k + 2) * gn_keep_stride(rows); }

void gnode_set_error(const char* fmt, ...);

// Zero `bytes` (a multiple of 4) at `p` (4-byte aligned) on the stream, with a KERNEL: hipMemsetAsync becomes a memset node when a
// caller captures the call into a HIP graph, and on this ROCm such nodes were not re-executed reliably on the second and later
// replays (round 3: the trainer's replayed step summed stale gradient slots).  Kernel nodes replay in order.
int gn_zero_async(void* p, size_t bytes, hipStream_t st);
// several regions in ONE launch (each 4-byte aligned, a multiple of 4 bytes): the start-up zero-fills of a backward call are
// launch latency, not bytes, on the small graphs the reference trains on
struct GnZeroRegions { void* p[6]; size_t bytes[6]; int n; };
int gn_zero_regions_async(const GnZeroRegions& r, hipStream_t st);

// opt-in launch profiler (gnode_profile_enable): bracket a launch of `kind` with HIP events when it is sampled
bool gn_prof_begin(int kind, hipStream_t st);
void gn_prof_end(int kind, hipStream_t st);

#define GN_CHECK_ARG(cond, ...)                 \
    do {                                        \
        if (!(cond)) {                          \
            gnode_set_error(__VA_ARGS__);       \
            return GNODE_ERR_ARG;               \
        }                                       \
    } while (0)

#define GN_HIP(call)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            gnode_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return GNODE_ERR_HIP;                                                           \
        }                                                                                   \
    } while (0)

#define GN_LAUNCH_CHECK() GN_HIP(hipGetLastError())

static inline size_t gn_align(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// lanes per row of the lane-group kernels: H/4 rounded up to a power of two
static inline int gn_lpr(int H) {
    int need = H / 4, l = 1;
    while (l < need) l <<= 1;
    return l;
}

// switch over it to a compile-time LPR; a file's largest instance is LMAX (32 or 64), which larger values also take
#define GN_LPR_DISPATCH(LMAX, lpr, ...)                            \
    switch (lpr) {                                                 \
        case 1: { constexpr int LPR = 1; __VA_ARGS__; } break;     \
        case 2: { constexpr int LPR = 2; __VA_ARGS__; } break;     \
        case 4: { constexpr int LPR = 4; __VA_ARGS__; } break;     \
        case 8: { constexpr int LPR = 8; __VA_ARGS__; } break;     \
        case 16: { constexpr int LPR = 16; __VA_ARGS__; } break;   \
        case 32: { constexpr int LPR = 32; __VA_ARGS__; } break;   \
        default: { constexpr int LPR = LMAX; __VA_ARGS__; } break; \
    }

// out_rows (the grid points written to S / I / R; null = every one) must be ascending grid indices in [0, G)
static inline int gn_check_out_rows(const char* fn, const int32_t* out_rows, int n_out, int G) {
    if (out_rows)
        for (int i = 0; i < n_out; ++i)
            GN_CHECK_ARG(out_rows[i] >= 0 && out_rows[i] < G && (i == 0 || out_rows[i] > out_rows[i - 1]),
                         "%s: out_rows must be ascending grid indices in [0,%d)", fn, G);
    return 0;
}
// the output row of each of the G grid points, or -1 (out_rows checked)
static inline std::vector<int> gn_out_slots(const int32_t* out_rows, int n_out, int G) {
    std::vector<int> slot(G, -1);
    for (int i = 0; i < (out_rows ? n_out : G); ++i) slot[out_rows ? out_rows[i] : i] = i;
    return slot;
}
// the persistent launches' give-up word in the control block at `ctl` (forward and backward workspaces): *code_host = 0 or
// the code, with the error message naming `who`; synchronises the stream
int gn_read_give_up(const void* ctl, int H, void* stream, int32_t* code_host, const char* who);
