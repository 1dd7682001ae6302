// GN-ODE hot path for MI355X (gfx950): C-ABI host code (graph handle, RHS, forward) and the
// generic-H kernels (any H % 4 == 0): node MLP, CSR pull-gather, SIR derivative, Euler/RK4
// update and fused read-out, one sub-wave lane group of H/4 lanes per node row with 16-byte
// lane accesses.  H = 64 runs the fused MFMA kernels of gnode_h64.hip.
//
// Reference semantics restated (file:line into the reference tree):
//   ODEfunc.forward      ode_nn_ngraph_sim.py:58-96   (multi: ode_nn_ngraphs.py:54-83)
//   ODEBlock.forward     ode_nn_ngraph_sim.py:148-188 (multi: ode_nn_ngraphs.py:124-152)
//   odeint(euler)        torchdiffeq 0.2.2 fixed grid (call site :168)
//   get_sir_t_nodes_torch ode_nn.py:249-261 (fused as an output-row list)
//
// Compiled with -ffp-contract=off: the elementwise SIR update rounds exactly
// like the reference's separate torch ops; FMAs are written explicitly where
// they are wanted (the generic node-MLP inner product).
#include "gnode_common.h"
#include "gnode_gather.h"
#include "gnode_generic.h"
#include "gnode_h64.h"
#include <algorithm>

// --------------------------------------------------------------------------- error state
static thread_local char g_err[512] = "";
void gnode_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* gnode_last_error(void) { return g_err; }

__global__ __launch_bounds__(256) void k_zero_words(uint32_t* __restrict__ p, size_t nwords) {
    const size_t stride = (size_t)gridDim.x * 256 * 4;
    for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < nwords; i += stride) {
        if (i + 4 <= nwords && ((uintptr_t)(p + i) & 15u) == 0) *reinterpret_cast<uint4*>(p + i) = make_uint4(0u, 0u, 0u, 0u);
        else for (size_t j = i; j < nwords && j < i + 4; ++j) p[j] = 0u;
    }
}
int gn_zero_async(void* p, size_t bytes, hipStream_t st) {
    GN_CHECK_ARG(bytes % 4 == 0 && ((uintptr_t)p & 3u) == 0, "gn_zero_async: unaligned region");
    if (bytes == 0) return 0;
    const size_t nwords = bytes / 4;
    const unsigned grid = (unsigned)std::min<size_t>((nwords / 4 + 255) / 256 + 1, 2048);
    hipLaunchKernelGGL(k_zero_words, dim3(grid), dim3(256), 0, st, (uint32_t*)p, nwords);
    GN_LAUNCH_CHECK();
    return 0;
}
__global__ __launch_bounds__(256) void k_zero_regions(GnZeroRegions r) {
    uint32_t* p = (uint32_t*)r.p[blockIdx.y];
    const size_t nwords = r.bytes[blockIdx.y] / 4;
    const size_t stride = (size_t)gridDim.x * 256 * 4;
    for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < nwords; i += stride) {
        if (i + 4 <= nwords && ((uintptr_t)(p + i) & 15u) == 0) *reinterpret_cast<uint4*>(p + i) = make_uint4(0u, 0u, 0u, 0u);
        else for (size_t j = i; j < nwords && j < i + 4; ++j) p[j] = 0u;
    }
}
int gn_zero_regions_async(const GnZeroRegions& r, hipStream_t st) {
    size_t mx = 0;
    for (int k = 0; k < r.n; ++k) {
        GN_CHECK_ARG(r.bytes[k] % 4 == 0 && ((uintptr_t)r.p[k] & 3u) == 0, "gn_zero_regions_async: unaligned region");
        mx = std::max(mx, r.bytes[k]);
    }
    if (r.n <= 0 || mx == 0) return 0;
    const unsigned gx = (unsigned)std::min<size_t>((mx / 16 + 255) / 256 + 1, 1024);
    hipLaunchKernelGGL(k_zero_regions, dim3(gx, (unsigned)r.n), dim3(256), 0, st, r);
    GN_LAUNCH_CHECK();
    return 0;
}
extern "C" int gnode_version(void) { return 226; }   // 226: gnode_sir_mc_philox_nodes, gnode_sir_nodes_workspace_bytes; 225: gnode_backward_discrete_keep_f32, gnode_backward_discrete_path; 224: gnode_backward_discrete_f32; 223: gnode_backward_dx_f32, gnode_backward_rk4_dx_f32; 222: gnode_rhs_vjp_f32, gnode_backward_rk4_f32; 221: gnode_backward_status, persistent launches for hidden 8 / 16 / 32 (gnode_forward_path kind 3); 220: forward takes flags + reports what sol / keep carry (sol_info), backward checks it; persistent one-launch path for mid-size graphs; 200: workspace sizes take the graph handle (hub scratch is carved from the caller's workspace); 210: forward / backward take the optional kept-activation buffer

// --------------------------------------------------------------------------- instrumentation
// HIP-event pairs around every launch of the two step kernels while enabled
// (bench.py's roofline leg: average launch duration measured on the launch stream).
// PROCESS-WIDE state, documented as such in gnode.h: a measuring harness switches it on around a single-threaded
// region; it is off by default and the launch paths then touch none of it.
#include <vector>
struct ProfKind { std::vector<hipEvent_t> ev; size_t used = 0; };
static bool g_prof_on = false;
static const int kProfKinds = 4;   // 0 = step (gather/update) kernel, 1 = node-MLP kernel, 2 = backward interval kernel, 3 = Monte-Carlo kernel
static ProfKind g_prof[kProfKinds];

static const int kProfEvery = 7;   // bracket one launch in 7 (odd: output and non-output intervals alternate): the events themselves cost GPU time
static long g_prof_seq[kProfKinds] = {0, 0, 0, 0};
static bool prof_begin(int kind, hipStream_t st);
static void prof_mark(int kind, hipStream_t st) {
    if (!g_prof_on) return;
    ProfKind& k = g_prof[kind];
    if (k.used == k.ev.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        k.ev.push_back(e);
    }
    (void)hipEventRecord(k.ev[k.used++], st);
}

// begin(): returns true when this launch is sampled; the caller then calls prof_mark again after the launch
static bool prof_begin(int kind, hipStream_t st) {
    if (!g_prof_on) return false;
    if ((g_prof_seq[kind]++ % kProfEvery) != 0) return false;
    prof_mark(kind, st);
    return true;
}
bool gn_prof_begin(int kind, hipStream_t st) { return prof_begin(kind, st); }      // for the other translation units
void gn_prof_end(int kind, hipStream_t st) { prof_mark(kind, st); }

extern "C" int gnode_profile_enable(int on) {
    g_prof_on = on != 0;
    for (int k = 0; k < kProfKinds; ++k) { g_prof_seq[k] = 0; g_prof[k].used = 0; }
    return 0;
}

extern "C" int gnode_profile_read_kind(int32_t kind, double* ms_out, int64_t* launches_out) {
    GN_CHECK_ARG(kind >= 0 && kind < kProfKinds, "gnode_profile_read_kind: kind %d out of range", kind);
    double ms = 0.0;
    int64_t cnt = 0;
    ProfKind& pk = g_prof[kind];
    for (size_t i = 0; i + 1 < pk.used; i += 2) {
        GN_HIP(hipEventSynchronize(pk.ev[i + 1]));
        float t = 0.f;
        GN_HIP(hipEventElapsedTime(&t, pk.ev[i], pk.ev[i + 1]));
        ms += t;
        cnt += 1;
    }
    if (ms_out) *ms_out = ms;
    if (launches_out) *launches_out = cnt;
    return 0;
}

extern "C" int gnode_profile_read(double* gather_ms, int64_t* gather_launches, double* mlp_ms, int64_t* mlp_launches) {
    double ms[2] = {0.0, 0.0};
    int64_t cnt[2] = {0, 0};
    for (int k = 0; k < 2; ++k) {
        ProfKind& pk = g_prof[k];
        for (size_t i = 0; i + 1 < pk.used; i += 2) {
            GN_HIP(hipEventSynchronize(pk.ev[i + 1]));
            float t = 0.f;
            GN_HIP(hipEventElapsedTime(&t, pk.ev[i], pk.ev[i + 1]));
            ms[k] += t;
            cnt[k] += 1;
        }
    }
    if (gather_ms) *gather_ms = ms[0];
    if (gather_launches) *gather_launches = cnt[0];
    if (mlp_ms) *mlp_ms = ms[1];
    if (mlp_launches) *mlp_launches = cnt[1];
    return 0;
}

// --------------------------------------------------------------------------- K0: encoder
// y0 = cat(relu(Linear(1,H)(S0)), ..(I0), ..(R0), beta_gamma)   ode_nn_ngraph_sim.py:149-168
// x [rows, 3+H]; Y [3][rows][H]; beta/gamma [rows]; optional sol0 [4*rows, H].
template <int LPR>
__global__ __launch_bounds__(256) void k_encode(const float* __restrict__ x, const float* __restrict__ w1,
                                                const float* __restrict__ b1, float* __restrict__ Y,
                                                float* __restrict__ beta, float* __restrict__ gamma,
                                                float* __restrict__ sol0, long rows, int H) {
    const int sub = threadIdx.x % LPR;
    const long r = (long)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
    if (r >= rows || 4 * sub >= H) return;
    const float* xr = x + r * (3 + H);
    const float s0 = xr[0], i0 = xr[1], r0 = xr[2];
    const float4 w = ld4(w1 + 4 * sub), b = ld4(b1 + 4 * sub);
    auto enc = [&](float v) {
        return make_float4(fmaxf(fmaf(w.x, v, b.x), 0.f), fmaxf(fmaf(w.y, v, b.y), 0.f),
                           fmaxf(fmaf(w.z, v, b.z), 0.f), fmaxf(fmaf(w.w, v, b.w), 0.f));
    };
    const size_t slab = (size_t)rows * H, off = (size_t)r * H + 4 * sub;
    const float4 yS = enc(s0), yI = enc(i0), yR = enc(r0);
    st4(Y + off, yS); st4(Y + slab + off, yI); st4(Y + 2 * slab + off, yR);
    if (sub == 0) { beta[r] = xr[3]; gamma[r] = xr[4]; }
    if (sol0) {
        st4(sol0 + off, yS); st4(sol0 + slab + off, yI); st4(sol0 + 2 * slab + off, yR);
        const float* bg = xr + 3 + 4 * sub;
        st4(sol0 + 3 * slab + off, make_float4(bg[0], bg[1], bg[2], bg[3]));
    }
}

// Everything before the first Euler step of the generic-H fused path in ONE launch: encoder (k_encode), read-out at grid
// point 0 (k_readout) and Z_I(y_0) (k_mlp_generic's arithmetic in k_step_generic's lane-group form: same fma chain from the
// bias, same sigmoid -> the same bits), plus the zero-fill of the persistent launch's control block when one follows.
template <int LPR>
__global__ __launch_bounds__(256) void k_prologue_generic(const float* __restrict__ x, const float* __restrict__ w1,
                                                          const float* __restrict__ b1, const float* __restrict__ W,
                                                          const float* __restrict__ bias, const float* __restrict__ w3,
                                                          const float* __restrict__ b3, const float* __restrict__ w2,
                                                          const float* __restrict__ b2, float* __restrict__ Y,
                                                          float* __restrict__ beta, float* __restrict__ gamma,
                                                          float* __restrict__ sol0, float* __restrict__ ZI, float* __restrict__ S0,
                                                          float* __restrict__ I0, float* __restrict__ R0, long rows, int H,
                                                          uint32_t* __restrict__ zero_words, int n_zero_words) {
    extern __shared__ float Wt[];                 // [H][H] transposed: Wt[k][j] = W[j][k]
    for (int idx = threadIdx.x; idx < H * H; idx += 256) Wt[(size_t)(idx % H) * H + idx / H] = W[idx];
    if (zero_words && blockIdx.x == 0)
        for (int i = threadIdx.x; i < n_zero_words; i += 256) zero_words[i] = 0u;
    __syncthreads();
    const int sub = threadIdx.x % LPR;
    const long r = (long)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
    const bool inrow = r < rows, active = 4 * sub < H, ok = inrow && active;     // (every lane stays: the mat-vec and the read-out shuffle)
    const float4 z0 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 yS = z0, yI = z0, yR = z0;
    const size_t slab = (size_t)rows * H, off = (size_t)(inrow ? r : 0) * H + 4 * sub;
    if (ok) {
        const float* xr = x + r * (3 + H);
        const float s0 = xr[0], i0 = xr[1], r0 = xr[2];
        const float4 w = ld4(w1 + 4 * sub), b = ld4(b1 + 4 * sub);
        auto enc = [&](float v) {
            return make_float4(fmaxf(fmaf(w.x, v, b.x), 0.f), fmaxf(fmaf(w.y, v, b.y), 0.f),
                               fmaxf(fmaf(w.z, v, b.z), 0.f), fmaxf(fmaf(w.w, v, b.w), 0.f));
        };
        yS = enc(s0); yI = enc(i0); yR = enc(r0);
        st4(Y + off, yS); st4(Y + slab + off, yI); st4(Y + 2 * slab + off, yR);
        if (sub == 0) { beta[r] = xr[3]; gamma[r] = xr[4]; }
        if (sol0) {
            st4(sol0 + off, yS); st4(sol0 + slab + off, yI); st4(sol0 + 2 * slab + off, yR);
            const float* bg = xr + 3 + 4 * sub;
            st4(sol0 + 3 * slab + off, make_float4(bg[0], bg[1], bg[2], bg[3]));
        }
    }
    if (S0) {
        float pS, pI, pR;
        gn_readout<XorSum<LPR>>(yS, yI, yR, W3Rows{w3, H, sub, active}, b3, w2, b2[0], pS, pI, pR);
        if (sub == 0 && inrow) { S0[r] = pS; I0[r] = pI; R0[r] = pR; }
    }
    const float4 bias4 = active ? ld4(bias + 4 * sub) : z0;
    const float4 zi = group_mlp<LPR>(yI, Wt, bias4, sub, active, H);
    if (ok) st4(ZI + off, zi);
}

// --------------------------------------------------------------------------- K1: node MLP  Z = sigmoid(Y W^T + b)
// Generic FMA path (any H % 4 == 0, H <= 128): W^T staged in LDS, one LPR-lane
// group per row, each lane 4 output features.
template <int LPR>
__global__ __launch_bounds__(256) void k_mlp_generic(const float* __restrict__ X, const float* __restrict__ W,
                                                     const float* __restrict__ bias, float* __restrict__ Z,
                                                     long nrows, int H) {
    extern __shared__ float lds[];
    float* Wt = lds;                      // [H][H] transposed: Wt[k][j] = W[j][k]
    float* Xs = lds + (size_t)H * H;      // [256/LPR][H]
    for (int idx = threadIdx.x; idx < H * H; idx += 256) {
        int j = idx / H, k = idx % H;
        Wt[(size_t)k * H + j] = W[idx];
    }
    const int sub = threadIdx.x % LPR, g = threadIdx.x / LPR;
    const long r = (long)blockIdx.x * (256 / LPR) + g;
    const bool active = (r < nrows) && (4 * sub < H);
    if (active) st4(Xs + (size_t)g * H + 4 * sub, ld4(X + (size_t)r * H + 4 * sub));
    __syncthreads();
    if (!active) return;
    float4 acc = ld4(bias + 4 * sub);
    const float* xr = Xs + (size_t)g * H;
    for (int k = 0; k < H; ++k) {
        const float xv = xr[k];
        const float4 w = ld4(Wt + (size_t)k * H + 4 * sub);
        acc.x = fmaf(xv, w.x, acc.x); acc.y = fmaf(xv, w.y, acc.y);
        acc.z = fmaf(xv, w.z, acc.z); acc.w = fmaf(xv, w.w, acc.w);
    }
    st4(Z + (size_t)r * H + 4 * sub,
        make_float4(gn_sigmoid(acc.x), gn_sigmoid(acc.y), gn_sigmoid(acc.z), gn_sigmoid(acc.w)));
}

// --------------------------------------------------------------------------- K2: gather + SIR derivative (+ Euler update + read-out)
// AI[r] = sum_{c in adj(node)} Z_I[base + c] in ascending column order (the CPU
// scatter_add_ order of ode_nn_ngraph_sim.py:73), then :75-77.  One LPR-lane
// group per row; the group fetches LPR column indices with one coalesced load and
// broadcasts them by lane shuffle, so neighbour-row loads are issued back to back.
template <int LPR>
__device__ __forceinline__ float4 gather_row(const int* __restrict__ rowptr, const int* __restrict__ col,
                                             const float* __restrict__ ZI_base, int node, int sub, bool active, int H) {
    // small lane groups have registers to spare: more rows in flight, fewer dependent round trips per row
    return gn_gather1<(LPR <= 4 ? 16 : 8)>(col, rowptr[node], rowptr[node + 1], ZI_base, H, sub, active);
}

struct StepOut {
    float* S; float* I; float* R;   // this step's output rows [rows] or null
    float* sol;                     // sol[g+1] base ([4*rows,H]) or null
};

// MODE 0: derivative only (dY <- f(Y)), MODE 1: Euler update in place (+ outputs)
template <int LPR, int MODE>
__global__ __launch_bounds__(256) void k_gather(const int* __restrict__ rowptr, const int* __restrict__ col, int n,
                                                long rows, int H, float* __restrict__ Y, const float* __restrict__ Z,
                                                const float* __restrict__ beta, const float* __restrict__ gamma,
                                                int bg_stride, float dt, float* __restrict__ dY,
                                                const float* __restrict__ w3, const float* __restrict__ b3,
                                                const float* __restrict__ w2, const float* __restrict__ b2, StepOut out,
                                                const int* __restrict__ hubidx, const float* __restrict__ AIhub, int n_hub) {
    const int sub = threadIdx.x % LPR;
    const int node = blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
    if (node >= n) return;                       // whole lane group leaves together
    const bool active = 4 * sub < H;
    const long base = (long)blockIdx.y * n;      // block-diagonal: sample b owns rows [b*n, (b+1)*n)
    const long r = base + node;
    const size_t slab = (size_t)rows * H, off = (size_t)r * H + 4 * sub;
    const float* ZS = Z;
    const float* ZI = Z + slab;

    const int hub = hubidx ? hubidx[node] : -1;  // long rows were summed by the hub kernels (gnode_hub.hip)
    float4 ai;
    if (hub >= 0) ai = active ? ld4(AIhub + ((size_t)blockIdx.y * n_hub + hub) * H + 4 * sub) : make_float4(0.f, 0.f, 0.f, 0.f);
    else ai = gather_row<LPR>(rowptr, col, ZI + (size_t)base * H, node, sub, active, H);
    float4 zs = make_float4(0.f, 0.f, 0.f, 0.f), zi = zs;
    if (active) { zs = ld4(ZS + off); zi = ld4(ZI + off); }
    const float nb = -beta[(size_t)r * bg_stride], gm = gamma[(size_t)r * bg_stride];
    float4 dS, dI, dR;
    gn_rhs_row(nb, gm, ai, zs, zi, dS, dI, dR);
    if (MODE == 0) {
        if (active) { st4(dY + off, dS); st4(dY + slab + off, dI); st4(dY + 2 * slab + off, dR); }
        return;
    }
    float4 yS = make_float4(0.f, 0.f, 0.f, 0.f), yI = yS, yR = yS;
    if (active) {
        yS = ld4(Y + off); yI = ld4(Y + slab + off); yR = ld4(Y + 2 * slab + off);
        yS = gn_euler4(yS, dt, dS);
        yI = gn_euler4(yI, dt, dI);
        yR = gn_euler4(yR, dt, dR);
        st4(Y + off, yS); st4(Y + slab + off, yI); st4(Y + 2 * slab + off, yR);
        if (out.sol) { st4(out.sol + off, yS); st4(out.sol + slab + off, yI); st4(out.sol + 2 * slab + off, yR); }
    }
    if (out.S) {
        float pS, pI, pR;
        gn_readout<XorSum<LPR>>(yS, yI, yR, W3Rows{w3, H, sub, active}, b3, w2, b2[0], pS, pI, pR);
        if (sub == 0) { out.S[r] = pS; out.I[r] = pI; out.R[r] = pR; }
    }
}

// Fused Euler step for generic H (the multi-graph launcher trains with H = 8): the same launch
// structure as k_step64 -- gather, Z_S from Y_S, update, read-out, next step's Z_I -- with the node
// MLP as a lane-group mat-vec: the row's H values live 4 per lane, x_k is broadcast inside the group
// by shuffle and multiplied with W^T (staged in LDS, [k][j]).
// HUBS (compile time, as k_step64): graphs without long rows carry none of that code and none of its registers -- the hub branch
// keeps 32 partial rows in flight at the small lane-group sizes (168 VGPRs against 120)
template <int LPR, bool HUBS>
__global__ __launch_bounds__(256) void k_step_generic(const int* __restrict__ rowptr, const int* __restrict__ col, int n,
                                                      long rows, int H, float* Y,
                                                      const float* __restrict__ ZI, float* __restrict__ ZI_next,
                                                      const float* __restrict__ W, const float* __restrict__ bias,
                                                      const float* __restrict__ beta, const float* __restrict__ gamma,
                                                      float dt, const float* __restrict__ w3, const float* __restrict__ b3,
                                                      const float* __restrict__ w2, const float* __restrict__ b2,
                                                      StepOut out, const int* __restrict__ hubidx,
                                                      const float* __restrict__ HubP /* hub rows: per-segment partial sums [B][n_seg][H] */,
                                                      const int* __restrict__ hub_seg_ptr, int n_seg) {
    extern __shared__ float Wt[];                 // [H][H] transposed: Wt[k][j] = W[j][k]
    for (int idx = threadIdx.x; idx < H * H; idx += 256) Wt[(size_t)(idx % H) * H + idx / H] = W[idx];
    __syncthreads();
    const int sub = threadIdx.x % LPR;
    const int node = blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
    if (node >= n) return;                        // whole lane group leaves together (no barrier after this point)
    const bool active = 4 * sub < H;
    const long base = (long)blockIdx.y * n, r = base + node;
    const size_t slab = (size_t)rows * H, off = (size_t)r * H + 4 * sub;
    const float4 z0 = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 bias4 = active ? ld4(bias + 4 * sub) : z0;

    // own-row loads first: they travel under the gather's dependent id -> row round trips instead of after them
    float4 yS = z0, yI = z0, yR = z0, zi = z0;
    if (active) { yS = ld4(Y + off); yI = ld4(Y + slab + off); yR = ld4(Y + 2 * slab + off); zi = ld4(ZI + off); }
    const float nb = -beta[r], gm = gamma[r];
    const int hub = HUBS ? hubidx[node] : -1;
    float4 ai;
    if (HUBS && hub >= 0) {
        // long rows: their 32-edge segments were summed by k_hub_seg; add the partials up in segment order (what a separate
        // reduction launch used to do -- at this size a launch costs as much as the step), 8 in flight
        ai = z0;
        const float* pp = HubP + (size_t)blockIdx.y * n_seg * H + 4 * sub;
        const int s1 = hub_seg_ptr[hub + 1];
        // (one lane group walks a hub's partials: a 12 777-edge row is 400 of them, and at 8 in flight that single chain was 30 us of
        //  a 76 us step at H = 8 -- 32 in flight for the small lane groups, which have the registers; same order, same bits)
#ifndef GN_HUB_PF
#define GN_HUB_PF 32
#endif
        constexpr int PF = LPR <= 4 ? GN_HUB_PF : 8;
        for (int sg = hub_seg_ptr[hub]; sg < s1; sg += PF) {
            float4 u[PF];
#pragma unroll
            for (int q = 0; q < PF; ++q) u[q] = (active && sg + q < s1) ? ld4(pp + (size_t)(sg + q) * H) : z0;
#pragma unroll
            for (int q = 0; q < PF; ++q) { ai.x += u[q].x; ai.y += u[q].y; ai.z += u[q].z; ai.w += u[q].w; }
        }
    } else ai = gather_row<LPR>(rowptr, col, ZI + (size_t)base * H, node, sub, active, H);
    const float4 zs = group_mlp<LPR>(yS, Wt, bias4, sub, active, H);
    float4 dS, dI, dR;
    gn_rhs_row(nb, gm, ai, zs, zi, dS, dI, dR);
    yS = gn_euler4(yS, dt, dS);
    yI = gn_euler4(yI, dt, dI);
    yR = gn_euler4(yR, dt, dR);
    if (active) {                                 // in place, or trajectory point k -> k+1 (the trajectory is the state)
        float* Yo = out.sol ? out.sol : Y;
        st4(Yo + off, yS); st4(Yo + slab + off, yI); st4(Yo + 2 * slab + off, yR);
    }
    if (out.S) {
        float pS, pI, pR;
        gn_readout<XorSum<LPR>>(yS, yI, yR, W3Rows{w3, H, sub, active}, b3, w2, b2[0], pS, pI, pR);
        if (sub == 0) { out.S[r] = pS; out.I[r] = pI; out.R[r] = pR; }
    }
    const float4 zn = group_mlp<LPR>(yI, Wt, bias4, sub, active, H);     // Z_I of the next step
    if (active) st4(ZI_next + off, zn);
}

// Stand-alone read-out of a state (grid point 0, and every point under RK4).
template <int LPR>
__global__ __launch_bounds__(256) void k_readout(const float* __restrict__ Y, long rows, int H,
                                                 const float* __restrict__ w3, const float* __restrict__ b3,
                                                 const float* __restrict__ w2, const float* __restrict__ b2,
                                                 float* __restrict__ S, float* __restrict__ I, float* __restrict__ R) {
    const int sub = threadIdx.x % LPR;
    const long r = (long)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
    if (r >= rows) return;
    const bool active = 4 * sub < H;
    const size_t slab = (size_t)rows * H, off = (size_t)r * H + 4 * sub;
    float4 yS = make_float4(0.f, 0.f, 0.f, 0.f), yI = yS, yR = yS;
    if (active) { yS = ld4(Y + off); yI = ld4(Y + slab + off); yR = ld4(Y + 2 * slab + off); }
    float pS, pI, pR;
    gn_readout<XorSum<LPR>>(yS, yI, yR, W3Rows{w3, H, sub, active}, b3, w2, b2[0], pS, pI, pR);
    if (sub == 0) { S[r] = pS; I[r] = pI; R[r] = pR; }
}

// out = y + a * (c1*k1 + c2*k2 + c3*k3 + c4*k4)   (RK4 3/8-rule stage combinations)
__global__ __launch_bounds__(256) void k_lincomb(float* __restrict__ out, const float* __restrict__ y, float a,
                                                 const float* __restrict__ k1, float c1, const float* __restrict__ k2,
                                                 float c2, const float* __restrict__ k3, float c3,
                                                 const float* __restrict__ k4, float c4, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        float4 v = ld4(k1 + 4 * i);
        float4 s = make_float4(c1 * v.x, c1 * v.y, c1 * v.z, c1 * v.w);
        if (k2) { v = ld4(k2 + 4 * i); s.x += c2 * v.x; s.y += c2 * v.y; s.z += c2 * v.z; s.w += c2 * v.w; }
        if (k3) { v = ld4(k3 + 4 * i); s.x += c3 * v.x; s.y += c3 * v.y; s.z += c3 * v.z; s.w += c3 * v.w; }
        if (k4) { v = ld4(k4 + 4 * i); s.x += c4 * v.x; s.y += c4 * v.y; s.z += c4 * v.z; s.w += c4 * v.w; }
        v = ld4(y + 4 * i);
        st4(out + 4 * i, make_float4(v.x + a * s.x, v.y + a * s.y, v.z + a * s.z, v.w + a * s.w));
    }
}

// sol[g][3rd slab] = sol[0][3rd slab] for g = 1 .. G-1: the beta-gamma slab rides along unchanged
// (its derivative is 0, ode_nn_ngraph_sim.py:96); one launch instead of one copy per step.
__global__ __launch_bounds__(256) void k_fill_bg(float* __restrict__ sol, size_t slab4, int G) {
    const float* src = sol + 3 * slab4 * 4;                  // slab4 = floats per slab / 4
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < slab4; i += (size_t)gridDim.x * 256) {
        const float4 v = ld4(src + 4 * i);
        for (int g = 1; g < G; ++g) st4(sol + ((size_t)g * 4 + 3) * slab4 * 4 + 4 * i, v);
    }
}

// --------------------------------------------------------------------------- host side
static int check_H(int H) {
    if (H < 4 || H > 128 || (H % 4) != 0) {
        gnode_set_error("unsupported hidden size H=%d (need 4 <= H <= 128, H %% 4 == 0)", H);
        return GNODE_ERR_ARG;
    }
    return 0;
}

static int launch_mlp(const gnode_graph_s* g, const float* X, const float* W, const float* b, float* Z, long nrows, int H, hipStream_t st) {
    if (nrows == 0) return 0;
    const bool sampled = prof_begin(1, st);
    if (H == 64) {
        if (int e = gn_launch_mlp64(g, X, W, b, Z, nrows, st)) return e;
    } else if (H == 128) {
        if (int e = gn_launch_mlp128(g, X, W, b, Z, nrows, st)) return e;    // matrix cores (gnode_h128.hip)
    } else {
        GN_CHECK_ARG(H <= 128, "generic node-MLP path supports H <= 128 (got %d)", H);
        const int lpr = gn_lpr(H);
        const int rpw = 256 / lpr;
        const size_t lds = ((size_t)H * H + (size_t)rpw * H) * sizeof(float);
        GN_LPR_DISPATCH(64, lpr, hipLaunchKernelGGL(k_mlp_generic<LPR>, dim3((unsigned)((nrows + rpw - 1) / rpw)), dim3(256), lds, st, X, W, b, Z, nrows, H));
    }
    if (sampled) prof_mark(1, st);
    GN_LAUNCH_CHECK();
    return 0;
}

int gn_launch_mlp_any(const gnode_graph_s* g, const float* X, const float* W, const float* b, float* Z, long nrows, int H,
                      hipStream_t st) {
    return launch_mlp(g, X, W, b, Z, nrows, H, st);
}

// dynamic LDS above 64 KB (H = 128 on the generic node-MLP: 68 KB) needs the attribute once per device
int gn_ode_set_attributes() {
    GN_HIP(hipFuncSetAttribute((const void*)k_mlp_generic<32>, hipFuncAttributeMaxDynamicSharedMemorySize, 72 * 1024));
    return 0;
}

// dY or in-place Euler update from (Y, Z)
static int launch_gather(gnode_graph_t g, int mode, long rows, int H, float* Y, const float* Z, const float* beta,
                         const float* gamma, int bg_stride, float dt, float* dY, const gnode_params* p, StepOut out,
                         void* hub_scratch, hipStream_t st) {
    const int lpr = gn_lpr(H), rpw = 256 / lpr;
    const long B = rows / g->info.n;
    dim3 grid((unsigned)((g->info.n + rpw - 1) / rpw), (unsigned)B);
    const float *w3 = p ? p->linear3_weight : nullptr, *b3 = p ? p->linear3_bias : nullptr;
    const float *w2 = p ? p->linearS2_weight : nullptr, *b2 = p ? p->linearS2_bias : nullptr;
    const float* AIhub = nullptr;
    if (int e = gn_hub_gather(g, B, H, Z + (size_t)rows * H, nullptr, hub_scratch, &AIhub, nullptr, st)) return e;
    const bool sampled = mode == 1 && prof_begin(0, st);
    if (mode == 0) {
        GN_LPR_DISPATCH(64, lpr, hipLaunchKernelGGL((k_gather<LPR, 0>), grid, dim3(256), 0, st, g->rowptr, g->col, g->info.n, rows, H,
                                                    Y, Z, beta, gamma, bg_stride, dt, dY, w3, b3, w2, b2, out, g->hubidx, AIhub, g->info.n_hub));
    } else {
        GN_LPR_DISPATCH(64, lpr, hipLaunchKernelGGL((k_gather<LPR, 1>), grid, dim3(256), 0, st, g->rowptr, g->col, g->info.n, rows, H,
                                                    Y, Z, beta, gamma, bg_stride, dt, dY, w3, b3, w2, b2, out, g->hubidx, AIhub, g->info.n_hub));
    }
    if (sampled) prof_mark(0, st);
    GN_LAUNCH_CHECK();
    return 0;
}

static int launch_readout(const float* Y, long rows, int H, const gnode_params* p, float* S, float* I, float* R,
                          hipStream_t st) {
    const int lpr = gn_lpr(H), rpw = 256 / lpr;
    GN_LPR_DISPATCH(64, lpr, hipLaunchKernelGGL(k_readout<LPR>, dim3((unsigned)((rows + rpw - 1) / rpw)), dim3(256), 0, st, Y,
                                                rows, H, p->linear3_weight, p->linear3_bias, p->linearS2_weight,
                                                p->linearS2_bias, S, I, R));
    GN_LAUNCH_CHECK();
    return 0;
}

// --------------------------------------------------------------------------- graph handle
// Per-device one-time setup, done when the first graph handle is created on a device (never on a launch path, so
// never inside a stream capture): dynamic-LDS attributes of every kernel that can ask for more than 64 KB, and the
// device's CU count.  The only process-wide state besides the opt-in profiler: write-once per device, under a lock.
#include <mutex>
static std::mutex g_dev_mu;
static bool g_dev_done[64] = {};
static int g_dev_cu[64] = {};
int gn_device_setup_once(int dev) {
    GN_CHECK_ARG(dev >= 0 && dev < 64, "device index %d out of range", dev);
    std::lock_guard<std::mutex> lk(g_dev_mu);
    if (g_dev_done[dev]) return 0;
    hipDeviceProp_t prop;
    GN_HIP(hipGetDeviceProperties(&prop, dev));
    g_dev_cu[dev] = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (int e = gn_ode_set_attributes()) return e;
    if (int e = gn_h64_set_attributes()) return e;
    if (int e = gn_pers64_set_attributes()) return e;
    if (int e = gn_pers_bwd64_set_attributes()) return e;
    if (int e = gn_persg_set_attributes()) return e;
    if (int e = gn_h128_set_attributes()) return e;
    if (int e = gn_bwd_set_attributes()) return e;
    if (int e = gn_bwd_tiny_set_attributes()) return e;
    if (int e = gn_sir_set_attributes()) return e;
    if (int e = gn_dmp_set_attributes()) return e;
    if (int e = gn_dmp_schedule_set_attributes()) return e;
    if (int e = gn_dmp_schedule_bwd_set_attributes()) return e;
    if (int e = gn_dmp_source_set_attributes()) return e;
    if (int e = gn_dmp_source_batch_set_attributes()) return e;
    if (int e = gn_dmp_source_events_set_attributes()) return e;
    if (int e = gn_dmp_outbreak_set_attributes()) return e;
    if (int e = gn_dmp_source_events_schedule_set_attributes()) return e;
    if (int e = gn_dmp_outbreak_schedule_set_attributes()) return e;
    if (int e = gn_rhs_vjp_set_attributes()) return e;
    g_dev_done[dev] = true;
    return 0;
}

// One device allocation of the handle (at least min_words words), filled with `v` and recorded in g->owned.
static hipError_t graph_upload(gnode_graph_s* g, int32_t** dst, const int32_t* v, size_t words, size_t min_words = 0) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, sizeof(int32_t) * std::max(words, min_words));
    if (e != hipSuccess) return e;
    g->owned.push_back(p);
    *dst = (int32_t*)p;
    return words ? hipMemcpy(p, v, sizeof(int32_t) * words, hipMemcpyHostToDevice) : hipSuccess;
}
static hipError_t graph_upload(gnode_graph_s* g, int32_t** dst, const std::vector<int32_t>& v, size_t min_words = 0) {
    return graph_upload(g, dst, v.data(), v.size(), min_words);
}

// Every array of the plan that some kernel reads, one allocation each (gnode_graph_plan.h says what they hold).
static hipError_t graph_upload_plan(gnode_graph_s* g, const GnGraphPlan& P, const int32_t* rowptr_host, const int32_t* col_host) {
#define UP(...) do { const hipError_t e_ = graph_upload(g, __VA_ARGS__); if (e_ != hipSuccess) return e_; } while (0)
    UP(&g->rowptr, rowptr_host, (size_t)g->info.n + 1);
    UP(&g->col, col_host, (size_t)g->nnz, 1);
    UP(&g->src, P.src, 1);
    UP(&g->rev, P.rev, 1);
    UP(&g->rowhdr, P.rowhdr);
    if (P.n_hub > 0) {
        UP(&g->hubidx, P.hubidx);
        UP(&g->seg_lo, P.seg_lo);
        UP(&g->seg_hi, P.seg_hi);
        UP(&g->hub_seg_ptr, P.hub_seg_ptr);
    }
    for (int i = 0; i < 3; ++i) {
        const GnPers64Maps& M = P.pers[i];
        if (!M.present) continue;
        UP(&g->persmap[i], M.map, 4);
        UP(&g->pershub[i], M.hub, 4);
        UP(&g->perssegptr[i], M.segptr, 4);
        UP(&g->perssegitem[i], M.items, 4);
        g->perslds[i] = M.lds;
    }
    if (!P.pgmap.empty()) UP(&g->pgmap, P.pgmap);
#undef UP
    return hipSuccess;
}

extern "C" int gnode_graph_destroy(gnode_graph_t g) {
    if (!g) return 0;
    for (void* p : g->owned) (void)hipFree(p);
    delete g;
    return 0;
}

extern "C" int gnode_graph_create(const int32_t* rowptr_host, const int32_t* col_host, int32_t n, int64_t nnz,
                                  gnode_graph_t* out) {
    GN_CHECK_ARG(rowptr_host && out && n > 0 && nnz >= 0, "gnode_graph_create: null pointer or empty graph");
    GN_CHECK_ARG(col_host || nnz == 0, "gnode_graph_create: col is null");
    const GnGraphPlan plan = gn_plan_graph(rowptr_host, col_host, n, nnz);
    GN_CHECK_ARG(plan.error.empty(), "%s", plan.error.c_str());
    int dev = 0;
    GN_HIP(hipGetDevice(&dev));
    if (int e = gn_device_setup_once(dev)) return e;
    gnode_graph_s* g = new gnode_graph_s();
    g->info = gn_graph_info(plan, n, g_dev_cu[dev]);
    g->nnz = nnz; g->max_degree = plan.max_degree; g->n_bigrow = plan.n_bigrow; g->n_seg = plan.n_seg;
    g->symmetric = plan.symmetric;
    g->device = dev;
    const hipError_t e = graph_upload_plan(g, plan, rowptr_host, col_host);
    if (e != hipSuccess) {
        gnode_set_error("gnode_graph_create: uploading the graph failed: %s", hipGetErrorString(e));
        gnode_graph_destroy(g);
        return GNODE_ERR_HIP;
    }
    *out = g;
    return 0;
}

extern "C" int gnode_graph_info(gnode_graph_t g, int32_t* n, int64_t* nnz, int32_t* max_degree) {
    GN_CHECK_ARG(g, "gnode_graph_info: null graph");
    if (n) *n = g->info.n;
    if (nnz) *nnz = g->nnz;
    if (max_degree) *max_degree = g->max_degree;
    return 0;
}

// --------------------------------------------------------------------------- RHS
extern "C" size_t gnode_rhs_workspace_bytes(gnode_graph_t g, int64_t rows, int32_t H) {
    if (!g || rows <= 0 || H < 4 || H > 128 || H % 4) return 0;
    return gn_align((size_t)2 * rows * H * sizeof(float)) + gn_hub_scratch_bytes(g, rows / g->info.n, H, 1);
}

extern "C" int gnode_rhs_f32(gnode_graph_t g, const float* x, const float* W, const float* b, float* dx, int64_t rows,
                             int32_t H, void* workspace, size_t workspace_bytes, void* stream) {
    GN_CHECK_ARG(g && x && W && b && dx && workspace, "gnode_rhs_f32: null pointer");
    if (int e = check_H(H)) return e;
    GN_CHECK_ARG(H >= 2, "gnode_rhs_f32: H >= 2 required (beta, gamma live in columns 0, 1)");
    GN_CHECK_ARG(rows > 0 && rows % g->info.n == 0, "gnode_rhs_f32: rows=%lld is not a multiple of graph n=%d",
                 (long long)rows, g->info.n);
    if (workspace_bytes < gnode_rhs_workspace_bytes(g, rows, H)) {
        gnode_set_error("gnode_rhs_f32: workspace %zu < %zu", workspace_bytes, gnode_rhs_workspace_bytes(g, rows, H));
        return GNODE_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    float* Z = (float*)workspace;
    void* hub_scratch = (char*)workspace + gn_align((size_t)2 * rows * H * sizeof(float));
    const size_t slab = (size_t)rows * H;
    if (int e = launch_mlp(g, x, W, b, Z, 2 * rows, H, st)) return e;   // R' is dead work in the reference: skipped
    StepOut none = {nullptr, nullptr, nullptr, nullptr};
    if (int e = launch_gather(g, 0, rows, H, const_cast<float*>(x), Z, x + 3 * slab, x + 3 * slab + 1, H, 0.f, dx,
                              nullptr, none, hub_scratch, st))
        return e;
    if (int e = gn_zero_async(dx + 3 * slab, slab * sizeof(float), st)) return e;   // 4th slab derivative = 0 (:96)
    return 0;
}

// --------------------------------------------------------------------------- forward
// Which form the forward takes (FwdPath): the H = 64 Euler forward prefers ONE persistent launch wherever its plan fits --
// down to karate: it measured faster than the one-workgroup kernels, 0.11 vs 0.17 ms for 39 steps, and its adjoint sweep
// 0.18 vs 0.35 ms -- then one workgroup per sample (tiny graphs in batches too large for one resident grid), then one launch
// per step.  H = 8 / 16 / 32 take their persistent launch where the batch fits one resident grid.
FwdPlan gn_forward_plan(const gnode_graph_s* g, long rows, int H, int method, int n_steps, int n_emit, bool with_sol, int flags) {
    FwdPlan pl{};
    pl.path = FwdPath::per_step;
    pl.h64 = H == 64 && method == 0;
    pl.n_emit = n_emit;
    const bool persist = n_steps >= 1 && !(flags & GNODE_FWD_PER_STEP);
    if (method == 0 && H <= 32 && persist && gn_persg_plan(g->info, rows, H, n_steps, &pl.persg)) pl.path = FwdPath::persg;
    else if (pl.h64 && persist && gn_pers64_plan(g->info, rows / g->info.n, n_steps, &pl.pers)) pl.path = FwdPath::pers64;
    else if (pl.h64 && n_steps >= 1 && gn_tiny64_ok(g->info.n, n_steps, n_emit, !with_sol)) pl.path = FwdPath::tiny;
    return pl;
}

// The forward workspace as byte offsets, in order: Y [3 slabs, element-contiguous] | Z [2 slabs; on the H = 64 path
// [table 0][zero row][table 1][zero row]: rows shorter than the step kernel's gather width read a zero row instead of
// branching per neighbour] | beta | gamma | projected R [rows][4] | (rk4) k1..k4, ytmp [3 slabs each] | the control block
// of the persistent launches (tickets, barrier flags, give-up word; with one launch per H = 64 step its first
// GN_STEP_TICKET_WORDS words are k_step64's tile counters instead) | `fixed`: the hub scratch (gn_hub_scratch_bytes).
struct FwdLayout { size_t Y, Z, beta, gamma, pr, rk, ctl, fixed; };
static_assert(sizeof(PersCtl) >= GN_STEP_TICKET_WORDS * sizeof(unsigned), "k_step64's tile counters live in the control block");
static FwdLayout forward_layout(int64_t rows, int32_t H, int32_t method) {
    const size_t slab = gn_align((size_t)rows * H * sizeof(float)), vec = gn_align((size_t)rows * sizeof(float));
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += bytes; return at; };
    FwdLayout L;
    L.Y = take(3 * slab); L.Z = take(2 * slab + 512); L.beta = take(vec); L.gamma = take(vec);
    L.pr = take(gn_align((size_t)rows * 4 * sizeof(float)));
    L.rk = take(method == 1 ? 15 * slab : 0);
    L.ctl = take(gn_pers64_ctl_bytes());
    L.fixed = off;
    return L;
}

extern "C" size_t gnode_forward_workspace_bytes(gnode_graph_t g, int64_t rows, int32_t H, int32_t method) {
    if (!g || rows <= 0 || H < 4 || H > 128 || H % 4) return 0;
    return forward_layout(rows, H, method).fixed + gn_hub_scratch_bytes(g, rows / g->info.n, H, 1);
}

// One forward call as the path launchers see it.
struct FwdCall {
    gnode_graph_s* g;
    const gnode_params* p;
    const float* dt_host;
    int n_steps, H;
    long rows;
    size_t slab;                        // rows * H floats
    float *S, *I, *R, *sol, *keep;
    const int* slot;                    // [n_steps + 1]: output row of each grid point, or -1
    float *Y, *Z, *beta, *gamma, *rk; char* ctl; void* hub_scratch;   // workspace (forward_layout)
    float* PR;                          // H = 64 inference (no trajectory): R's 4-float projection, else null
    float *zi_cur, *zi_nxt;             // gather tables of the current and the next step
    hipStream_t st;
    // grid point gi's row of an output (S, I or R), or null when gi is not emitted
    float* out(float* O, int gi) const { return slot[gi] >= 0 ? O + (size_t)slot[gi] * rows : nullptr; }
};

// sol[g][3rd slab] = sol[0][3rd slab] for g = 1 .. G-1 (the H = 64 paths keep A Z_I(y_k) there instead)
static int fill_bg(const FwdCall& c) {
    if (!c.sol || c.n_steps < 1) return 0;
    const size_t slab4 = c.slab / 4;
    hipLaunchKernelGGL(k_fill_bg, dim3((unsigned)std::min<size_t>((slab4 + 255) / 256, 2048)), dim3(256), 0, c.st, c.sol, slab4,
                       c.n_steps + 1);
    GN_LAUNCH_CHECK();
    return 0;
}

// Grid point 0: the encoder, beta / gamma, trajectory point 0, the read-out and (Euler below H = 128) the first gather table
// Z_I(y_0).  The persistent launches' control block is zeroed by the prologue's first workgroup: one launch less in front of them.
static int forward_prologue(const FwdCall& c, const FwdPlan& pl, const float* x, int method) {
    const gnode_params* p = c.p;
    const int H = c.H, lpr = gn_lpr(H), rpw = 256 / lpr;
    const dim3 grid((unsigned)((c.rows + rpw - 1) / rpw));
    if (pl.h64 && c.n_steps > 0) {      // encoder, beta/gamma, trajectory point 0, read-out, projected R and Z_I(y_0): one launch
        // (one launch per step: the head of the same block holds k_step64's tile counters, and each step zeroes the next one's)
        const bool steps = pl.path == FwdPath::per_step;
        return gn_launch_prologue64(x, p, c.Y, c.beta, c.gamma, c.sol, c.zi_cur, c.zi_nxt, c.PR, c.out(c.S, 0), c.out(c.I, 0),
                                    c.out(c.R, 0), c.rows, pl.path == FwdPath::pers64 || steps ? c.ctl : nullptr,
                                    steps ? GN_STEP_TICKET_WORDS * sizeof(unsigned) : gn_pers64_ctl_bytes(), c.st);
    }
    if (method == 0 && H < 128 && c.n_steps > 0) {     // generic H: encoder, read-out and Z_I(y_0) in one launch
        uint32_t* ctl = pl.path == FwdPath::persg ? (uint32_t*)c.ctl : nullptr;
        GN_LPR_DISPATCH(64, lpr, hipLaunchKernelGGL(k_prologue_generic<LPR>, grid, dim3(256), (size_t)H * H * sizeof(float), c.st, x,
                                                    p->linearS1_weight, p->linearS1_bias, p->odefunc_linear_weight,
                                                    p->odefunc_linear_bias, p->linear3_weight, p->linear3_bias, p->linearS2_weight,
                                                    p->linearS2_bias, c.Y, c.beta, c.gamma, c.sol, c.zi_cur, c.out(c.S, 0),
                                                    c.out(c.I, 0), c.out(c.R, 0), c.rows, H, ctl, (int)(gn_pers64_ctl_bytes() / 4)));
        GN_LAUNCH_CHECK();
        return 0;
    }
    // encoder, then the read-out (H = 128, rk4, no steps: the steps form their own node-MLP tables)
    GN_LPR_DISPATCH(64, lpr, hipLaunchKernelGGL(k_encode<LPR>, grid, dim3(256), 0, c.st, x, p->linearS1_weight, p->linearS1_bias,
                                                c.Y, c.beta, c.gamma, c.sol, c.rows, H));
    GN_LAUNCH_CHECK();
    if (c.slot[0] >= 0) return launch_readout(c.Y, c.rows, H, p, c.out(c.S, 0), c.out(c.I, 0), c.out(c.R, 0), c.st);
    return 0;
}

// mid-size graphs, H = 64: ONE persistent launch, every workgroup keeps its rows in registers for all steps (gnode_pers64.hip)
static int forward_pers64(const FwdCall& c, const FwdPlan& pl) {
    const gnode_params* p = c.p;
    const bool sampled = prof_begin(0, c.st);
    if (int e = gn_launch_pers64(c.g, pl.pers, c.rows, c.Y, c.PR, c.zi_cur, c.zi_nxt, p->odefunc_linear_weight, p->odefunc_linear_bias,
                                 c.beta, c.gamma, c.dt_host, c.slot + 1, c.n_steps, p, c.S, c.I, c.R, c.sol, c.keep, c.ctl, true, c.st))
        return e;
    if (sampled) prof_mark(0, c.st);
    return 0;
}

// small hidden sizes, batches that fit one resident grid: ONE persistent launch (gnode_persg.hip)
static int forward_persg(const FwdCall& c, const FwdPlan& pl) {
    const bool sampled = prof_begin(0, c.st);
    if (int e = gn_launch_persg(c.g, pl.persg, c.rows, c.H, c.Y, c.zi_cur, c.zi_nxt, c.beta, c.gamma, c.dt_host, c.slot + 1, c.n_steps,
                                c.p, c.S, c.I, c.R, c.sol, c.ctl, true, c.st))
        return e;
    if (sampled) prof_mark(0, c.st);
    return fill_bg(c);
}

// tiny graphs, H = 64: the whole integration in one launch (one workgroup per sample, state in LDS)
static int forward_tiny(const FwdCall& c) {
    const gnode_params* p = c.p;
    if (int e = gn_launch_tiny64(c.g, c.rows, c.Y, c.zi_cur, c.PR, p->odefunc_linear_weight, p->odefunc_linear_bias, c.beta, c.gamma,
                                 c.dt_host, c.slot + 1, c.n_steps, p, c.S, c.I, c.R, c.sol, c.keep, c.st))
        return e;
    return fill_bg(c);
}

// Euler, one launch per step: H = 64 fused (gnode_h64.hip), generic H fused, H = 128 node MLP + gather
static int forward_euler_steps(FwdCall c, const FwdPlan& pl) {
    const gnode_params* p = c.p;
    const size_t slab = c.slab;
    const long rows = c.rows;
    const int H = c.H, lpr = gn_lpr(H), rpw = 256 / lpr;
    for (int k = 0; k < c.n_steps; ++k) {
        const float dt = c.dt_host[k];
        float* sol_next = c.sol ? c.sol + (size_t)(k + 1) * 4 * slab : nullptr;
        // with a trajectory the fused kernels read point k and write point k+1 (no separate state copy)
        float* Ycur = c.sol ? c.sol + (size_t)k * 4 * slab : c.Y;
        if (pl.h64) {
            // training: the 4th slab of sol[k] (k >= 1; its odeint content is the constant beta-gamma slab of sol[0])
            // receives A Z_I(y_k), which the adjoint backward would otherwise gather again
            Step64Out out = {c.out(c.S, k + 1), c.out(c.I, k + 1), c.out(c.R, k + 1), sol_next,
                             c.keep ? (k >= 1 ? gn_keep_ps(c.keep, rows, k) : nullptr)          // with `keep`: P_S(y_k) there instead
                                    : ((c.sol && k >= 1) ? c.sol + (size_t)k * 4 * slab + 3 * slab : nullptr),
                             c.keep ? gn_keep_zs(c.keep, rows, k) : nullptr};
            const bool sampled = prof_begin(0, c.st);
            if (int e = gn_launch_step64(c.g, rows, Ycur, c.zi_cur, c.zi_nxt, p->odefunc_linear_weight,
                                         p->odefunc_linear_bias, c.beta, c.gamma, dt, p, c.PR, out, c.hub_scratch,
                                         (unsigned*)c.ctl + 16 * (k & 1), (unsigned*)c.ctl + 16 * ((k + 1) & 1), c.st))
                return e;
            if (sampled) prof_mark(0, c.st);
            if (c.keep) { c.zi_cur = c.zi_nxt; c.zi_nxt = gn_keep_zi(c.keep, rows, std::min(k + 2, c.n_steps)); }
            else std::swap(c.zi_cur, c.zi_nxt);
        } else if (H < 128) {
            // generic H: one fused launch per step (gather + both node MLPs as lane-group mat-vecs); H = 128 takes the
            // two-launch branch below, whose node MLP runs on the matrix cores (a VALU mat-vec is 12x off the bound there)
            StepOut out = {c.out(c.S, k + 1), c.out(c.I, k + 1), c.out(c.R, k + 1), sol_next};
            const float* HubP = nullptr;          // segment partials of the hub rows; the step kernel adds them up itself
            if (int e = gn_hub_segments(c.g, rows / c.g->info.n, H, c.zi_cur, c.hub_scratch, &HubP, c.st)) return e;
            dim3 grid((unsigned)((c.g->info.n + rpw - 1) / rpw), (unsigned)(rows / c.g->info.n));
            const size_t lds = (size_t)H * H * sizeof(float);
            const bool sampled = prof_begin(0, c.st);
            // (H < 128 here: W^T is at most 61 KB of dynamic LDS, below the 64 KB that would need an attribute)
            const bool hubs = c.g->info.n_hub > 0;
            GN_LPR_DISPATCH(64, lpr, hipLaunchKernelGGL((hubs ? k_step_generic<LPR, true> : k_step_generic<LPR, false>), grid, dim3(256), lds,
                                                        c.st, c.g->rowptr, c.g->col, c.g->info.n, rows, H, Ycur, c.zi_cur, c.zi_nxt,
                                                        p->odefunc_linear_weight, p->odefunc_linear_bias, c.beta, c.gamma, dt,
                                                        p->linear3_weight, p->linear3_bias, p->linearS2_weight, p->linearS2_bias, out,
                                                        c.g->hubidx, HubP, c.g->hub_seg_ptr, c.g->n_seg));
            if (sampled) prof_mark(0, c.st);
            GN_LAUNCH_CHECK();
            std::swap(c.zi_cur, c.zi_nxt);
        } else {
            if (int e = launch_mlp(c.g, c.Y, p->odefunc_linear_weight, p->odefunc_linear_bias, c.Z, 2 * rows, H, c.st)) return e;
            StepOut out = {c.out(c.S, k + 1), c.out(c.I, k + 1), c.out(c.R, k + 1), sol_next};
            if (int e = launch_gather(c.g, 1, rows, H, c.Y, c.Z, c.beta, c.gamma, 1, dt, nullptr, p, out, c.hub_scratch, c.st)) return e;
        }
    }
    return pl.h64 ? 0 : fill_bg(c);        // (H = 64: those slabs hold A Z_I(y_k) instead, see above)
}

// torchdiffeq 'rk4' = 3/8 rule, one step at a time
static int forward_rk4(const FwdCall& c) {
    const gnode_params* p = c.p;
    const size_t slab = c.slab;
    const long rows = c.rows;
    const int H = c.H;
    float *Y = c.Y, *Z = c.Z;
    float* k1 = c.rk; float* k2 = c.rk + 3 * slab; float* k3 = c.rk + 6 * slab; float* k4 = c.rk + 9 * slab;
    float* yt = c.rk + 12 * slab;
    const size_t n4 = 3 * slab / 4;
    const int eg = (int)std::min<size_t>((n4 + 255) / 256, 2048);
    StepOut none = {nullptr, nullptr, nullptr, nullptr};
    auto f = [&](float* y, float* kout) -> int {
        if (int e = launch_mlp(c.g, y, p->odefunc_linear_weight, p->odefunc_linear_bias, Z, 2 * rows, H, c.st)) return e;
        return launch_gather(c.g, 0, rows, H, y, Z, c.beta, c.gamma, 1, 0.f, kout, nullptr, none, c.hub_scratch, c.st);
    };
    const float third = 1.0f / 3.0f;
    for (int k = 0; k < c.n_steps; ++k) {
        const float dt = c.dt_host[k];
        if (int e = f(Y, k1)) return e;
        hipLaunchKernelGGL(k_lincomb, dim3(eg), dim3(256), 0, c.st, yt, Y, dt, k1, third, nullptr, 0.f, nullptr, 0.f, nullptr, 0.f, n4);
        if (int e = f(yt, k2)) return e;
        hipLaunchKernelGGL(k_lincomb, dim3(eg), dim3(256), 0, c.st, yt, Y, dt, k1, -third, k2, 1.f, nullptr, 0.f, nullptr, 0.f, n4);
        if (int e = f(yt, k3)) return e;
        hipLaunchKernelGGL(k_lincomb, dim3(eg), dim3(256), 0, c.st, yt, Y, dt, k1, 1.f, k2, -1.f, k3, 1.f, nullptr, 0.f, n4);
        if (int e = f(yt, k4)) return e;
        hipLaunchKernelGGL(k_lincomb, dim3(eg), dim3(256), 0, c.st, Y, Y, dt, k1, 0.125f, k2, 0.375f, k3, 0.375f, k4, 0.125f, n4);
        GN_LAUNCH_CHECK();
        if (c.sol) GN_HIP(hipMemcpyAsync(c.sol + (size_t)(k + 1) * 4 * slab, Y, 3 * slab * sizeof(float), hipMemcpyDeviceToDevice, c.st));
        if (c.slot[k + 1] >= 0)
            if (int e = launch_readout(Y, rows, H, p, c.out(c.S, k + 1), c.out(c.I, k + 1), c.out(c.R, k + 1), c.st)) return e;
    }
    return fill_bg(c);
}

extern "C" int gnode_forward_f32(gnode_graph_t g, const float* x, const gnode_params* p, const float* dt_host,
                                 int32_t n_steps, int32_t method, const int32_t* out_rows_host, int32_t n_out, float* S,
                                 float* I, float* R, float* sol, float* keep, size_t keep_bytes, int64_t rows, int32_t H,
                                 void* workspace, size_t workspace_bytes, void* stream, int32_t flags, int32_t* sol_info_host) {
    GN_CHECK_ARG(g && x && p && S && I && R && workspace, "gnode_forward_f32: null pointer");
    GN_CHECK_ARG(n_steps >= 0 && (n_steps == 0 || dt_host), "gnode_forward_f32: bad n_steps/dt");
    GN_CHECK_ARG(method == 0 || method == 1, "gnode_forward_f32: method must be 0 (euler) or 1 (rk4)");
    if (int e = check_H(H)) return e;
    GN_CHECK_ARG(H >= 2, "gnode_forward_f32: H >= 2 required (beta, gamma live in columns 3, 4 of x)");
    GN_CHECK_ARG(rows > 0 && rows % g->info.n == 0, "gnode_forward_f32: rows=%lld is not a multiple of graph n=%d",
                 (long long)rows, g->info.n);
    GN_CHECK_ARG(p->odefunc_linear_weight && p->odefunc_linear_bias && p->linearS1_weight && p->linearS1_bias &&
                     p->linear3_weight && p->linear3_bias && p->linearS2_weight && p->linearS2_bias,
                 "gnode_forward_f32: null parameter pointer");
    if (workspace_bytes < gnode_forward_workspace_bytes(g, rows, H, method)) {
        gnode_set_error("gnode_forward_f32: workspace %zu < %zu", workspace_bytes,
                        gnode_forward_workspace_bytes(g, rows, H, method));
        return GNODE_ERR_WORKSPACE;
    }
    const int G = n_steps + 1;
    if (out_rows_host) GN_CHECK_ARG(n_out >= 0, "gnode_forward_f32: n_out < 0");
    if (int e = gn_check_out_rows("gnode_forward_f32", out_rows_host, n_out, G)) return e;
    const FwdPlan pl = gn_forward_plan(g, rows, H, method, n_steps, out_rows_host ? n_out : G, sol != nullptr, flags);
    // kept activations: only the fused H = 64 training path fills them (elsewhere the backward recomputes)
    const size_t keep_need = gnode_forward_keep_bytes(g, rows, H, n_steps, pl.n_emit);
    if (!(keep && sol && method == 0 && keep_need > 0)) keep = nullptr;
    if (keep && keep_bytes < keep_need) {
        gnode_set_error("gnode_forward_f32: keep buffer %zu < %zu", keep_bytes, keep_need);
        return GNODE_ERR_WORKSPACE;
    }
    if (sol_info_host) {                         // what this call leaves in `sol` / `keep`: gnode_backward_f32 checks it
        const bool tiny = pl.path == FwdPath::tiny;
        *sol_info_host = !sol ? 0 : ((keep ? GNODE_SOL_KEEP : (pl.h64 && n_steps >= 1 && !tiny ? GNODE_SOL_AI : 0)) |
                                     (tiny ? GNODE_SOL_TINY : 0));
    }
    const FwdLayout L = forward_layout(rows, H, method);
    char* ws = (char*)workspace;
    const std::vector<int> slot = gn_out_slots(out_rows_host, n_out, G);
    FwdCall c{g, p, dt_host, n_steps, H, (long)rows, (size_t)rows * H, S, I, R, sol, keep, slot.data(),
              (float*)(ws + L.Y), (float*)(ws + L.Z), (float*)(ws + L.beta), (float*)(ws + L.gamma), (float*)(ws + L.rk),
              ws + L.ctl, ws + L.fixed, (pl.h64 && !sol) ? (float*)(ws + L.pr) : nullptr, nullptr, nullptr, (hipStream_t)stream};
    c.zi_cur = c.Z;
    c.zi_nxt = c.Z + c.slab + (pl.h64 ? 64 : 0);           // H = 64: each table is followed by its zero row
    if (keep) { c.zi_cur = gn_keep_zi(keep, rows, 0); c.zi_nxt = gn_keep_zi(keep, rows, 1); }   // step k gathers table k, fills k+1
    if (int e = forward_prologue(c, pl, x, method)) return e;
    switch (pl.path) {
        case FwdPath::pers64: return forward_pers64(c, pl);
        case FwdPath::persg: return forward_persg(c, pl);
        case FwdPath::tiny: return forward_tiny(c);
        default: return method == 0 ? forward_euler_steps(c, pl) : forward_rk4(c);
    }
}

extern "C" int gnode_forward_path(gnode_graph_t g, int64_t rows, int32_t H, int32_t method, int32_t n_steps, int32_t n_out,
                                  int32_t with_sol, int32_t flags, int32_t* plan_host) {
    if (!g || rows <= 0 || rows % g->info.n) return -1;
    const FwdPlan pl = gn_forward_plan(g, rows, H, method, n_steps, n_out, with_sol != 0, flags);
    if (pl.path == FwdPath::pers64 && plan_host) {
        const PersPlan& q = pl.pers;
        plan_host[0] = q.nt; plan_host[1] = q.wgs; plan_host[2] = q.span; plan_host[3] = q.gpx; plan_host[4] = q.concurrent;
    }
    return (int)pl.path;
}

// diagnostic build (GN_PERS_PROF): per-phase 100 MHz ticks of the last persistent launch on this workspace
extern "C" int gnode_forward_phase_ticks(int64_t rows, int32_t H, int32_t method, const void* workspace, uint64_t* ticks8_host) {
    const PersCtl* ctl = (const PersCtl*)((const char*)workspace + forward_layout(rows, H, method).ctl);
    GN_HIP(hipMemcpy(ticks8_host, ctl->prof, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

int gn_read_give_up(const void* ctl_ptr, int H, void* stream, int32_t* code_host, const char* who) {
    *code_host = 0;
    if (H != 64 && H > 32) return 0;             // (no persistent launch at other hidden sizes)
    unsigned err[2] = {0, 0};
    const PersCtl* ctl = (const PersCtl*)ctl_ptr;
    GN_HIP(hipMemcpyAsync(err, ctl->error, sizeof(err), hipMemcpyDeviceToHost, (hipStream_t)stream));
    GN_HIP(hipStreamSynchronize((hipStream_t)stream));
    *code_host = (int32_t)err[0];
    if (err[0]) gnode_set_error("%s: a workgroup gave up waiting for epoch %u of its group", who, err[1]);
    return 0;
}

extern "C" int gnode_forward_status(int64_t rows, int32_t H, int32_t method, const void* workspace, void* stream, int32_t* code_host) {
    GN_CHECK_ARG(workspace && code_host && rows > 0, "gnode_forward_status: null pointer");
    return gn_read_give_up((const char*)workspace + forward_layout(rows, H, method).ctl, H, stream, code_host, "persistent forward");
}

extern "C" size_t gnode_forward_keep_bytes(gnode_graph_t g, int64_t rows, int32_t H, int32_t n_steps, int32_t n_out) {
    (void)n_out;                                   // both H = 64 forms (tiled and one-launch) keep the same tables
    if (!g || rows <= 0 || H != 64 || n_steps < 1) return 0;
    return gn_keep_floats((long)rows, n_steps) * sizeof(float);
}

bool gn_sol_carries_ai(const gnode_graph_s* g, long rows, int H, int n_steps, int n_out, int flags) {
    return H == 64 && n_steps >= 1 && gn_forward_plan(g, rows, H, 0, n_steps, n_out, true, flags).path != FwdPath::tiny;
}

extern "C" int gnode_sol_carries_neighbour_sums(gnode_graph_t g, int64_t rows, int32_t H, int32_t n_steps, int32_t n_out, int32_t flags) {
    if (!g || rows <= 0 || rows % g->info.n) return 0;
    return gn_sol_carries_ai(g, rows, H, n_steps, n_out, flags) ? 1 : 0;
}
