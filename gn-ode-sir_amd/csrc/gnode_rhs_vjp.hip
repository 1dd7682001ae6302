// The RHS value and its vector-Jacobian product in one pass over the graph, and the RK4 (3/8 rule) adjoint built on it.
//
// ODEfunc.forward (ode_nn_ngraph_sim.py:58-96, multi: ode_nn_ngraphs.py:54-83) with Z = sigmoid(y W^T + b) on the S and I
// slabs and AI = A Z_I.  For a cotangent v (slabs S | I | R | beta-gamma):
//     u = beta (v_I - v_S)
//     dZ_S = u * AI                 dZ_I = A (u * Z_S) + gamma (v_R - v_I)        (A symmetric: the same CSR serves)
//     dpre = dZ * Z (1 - Z)
//     g_y[S, I] = dpre W            g_y[R] = 0 (Z_R is dead in the reference)
//     g_y[beta-gamma] = (sum_h (v_I - v_S) AI Z_S,  sum_h (v_R - v_I) Z_I,  0, ...)
//     gW = dpre^T y                 gb = sum_rows dpre
// Pass 1: the node MLP (gn_launch_mlp_any) and the table q = u * Z_S.  Pass 2 (k_rhs_vjp): per row tile, both neighbour
// tables (Z_I and q) in one walk of each row (hub rows from the two-table segment sums of gnode_hub.hip), dpre, f, g_y and
// the beta-gamma column gradients; dpre and y tiles are staged in LDS for g_y = dpre W and for the workgroup's gW / gb
// partials, which go to a fixed slot per workgroup, scaled and accumulated in place (slot += w * partial): deterministic,
// no float atomics, and the RK4 driver folds its 4 stages x all intervals into one final reduction.
//
// f is computed with the same operations in the same order as gnode_rhs_f32 (same node MLP, same ascending gathers, same
// SIR expressions under -ffp-contract=off): the same bits.
#include "gnode_common.h"
#include "gnode_bwd.h"
#include "gnode_gather.h"
#include "gnode_row.h"
#include <algorithm>

// --------------------------------------------------------------------------- pass 1: q = beta (v_I - v_S) * Z_S
__global__ __launch_bounds__(256) void k_vjp_q(const float* __restrict__ vSI, const float* __restrict__ ZS,
                                               const float* __restrict__ bg, float* __restrict__ q, long rows, int H) {
    const size_t slab = (size_t)rows * H, n4 = slab / 4;
    const int h4 = H / 4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const float bt = bg[(i / h4) * H];
        const float4 vS = ld4(vSI + 4 * i), vI = ld4(vSI + slab + 4 * i), z = ld4(ZS + 4 * i);
        st4(q + 4 * i, gn_q4(bt, vI, vS, z));
    }
}

// --------------------------------------------------------------------------- pass 2
struct VjpArgs {
    const int* rowptr; const int* col; int n; long rows; int H;
    const float* y;        // S | I slabs (I at + rows*H)
    const float* bg;       // beta-gamma rows [rows][H] (col 0 beta, col 1 gamma)
    const float* Z;        // Z_S | Z_I
    const float* q;        // u * Z_S
    const float* vSI;      // cotangent S | I slabs
    const float* vR;       // cotangent R slab
    const float* W;        // [H][H] (out, in)
    const int* hubidx; const float* AIhub; const float* GQhub; int n_hub;
    float* fSI;            // f's S | I slabs, or null
    float* fR;             // f's R slab, or null
    float* f4;             // f's beta-gamma slab (written 0), or null
    float* gySI;           // g_y's S | I slabs, or null
    float* gyR;            // g_y's R slab (written 0), or null
    float* gybg;           // g_y's beta-gamma slab, or null
    float* part;           // [grid][part_stride] gW at +0, gb at +H*H; or null
    int part_stride;
    float w;               // part += w * partial
    float* gx;             // BGX instance: rows of 3+H floats, columns 3, 4 += w * (d/dbeta, d/dgamma)
};

// BGX: the beta-gamma column gradients are accumulated into A.gx (the RK4 adjoint's input gradient) instead of gybg
template <int LPR, bool QUAD, bool BGX = false>
__global__ __launch_bounds__(256) void k_rhs_vjp(VjpArgs A) {
    extern __shared__ float lds[];
    constexpr int G = 256 / LPR;
    const int H = A.H;
    const bool mat = A.gySI != nullptr || A.part != nullptr;       // uniform over the launch
    float* Wl = lds;                                                // [H][H]  W[j][k]   (only with g_y)
    float* Dt = Wl + (A.gySI ? (size_t)H * H : 0);                  // [2][G][H] dpre tile (S, I)
    float* Yt = Dt + (size_t)2 * G * H;                             // [2][G][H] y tile    (S, I)
    if (A.gySI)
        for (int idx = threadIdx.x; idx < H * H; idx += 256) Wl[idx] = A.W[idx];
    const int sub = threadIdx.x % LPR, grp = threadIdx.x / LPR;
    const bool lane_ok = 4 * sub < H;
    const size_t slab = (size_t)A.rows * H;
    const int nE = H * H;
    // gW entries per thread.  H dividing 256 (4, 8, ..., 128): the thread owns columns 4c .. 4c+3 of rows j = j0 + R a
    // (Q = H/4 column quads, R = 256/Q rows side by side, a < MAXA), so that per tile row ONE float4 of y and MAXA dpre
    // values (LDS broadcasts) feed 4 MAXA FMAs.  Other H: entries e = tid + 256 m (m < MAXM), one y and one dpre value per FMA.
    constexpr int MAXM = (LPR * LPR / 16) < 1 ? 1 : (LPR * LPR / 16);
    constexpr int MAXA = (LPR * LPR / 64) < 1 ? 1 : (LPR * LPR / 64);
    constexpr int MAXE = (4 * MAXA > MAXM) ? 4 * MAXA : MAXM;
    constexpr bool quad = QUAD;                                      // the launcher passes 256 % H == 0
    const int Q = H / 4, qc = threadIdx.x % Q, j0 = threadIdx.x / Q, R = 256 / Q;
    float accW[MAXE];
#pragma unroll
    for (int m = 0; m < MAXE; ++m) accW[m] = 0.f;
    float accb = 0.f;
    const int M = (nE + 255) / 256;
    const float* ZI = A.Z + slab;
    for (long r0 = (long)blockIdx.x * G; r0 < A.rows; r0 += (long)gridDim.x * G) {
        const long r = r0 + grp;
        const bool row_ok = r < A.rows;
        const bool ok = lane_ok && row_ok;
        const long b = row_ok ? r / A.n : 0;
        const int node = row_ok ? (int)(r - b * A.n) : 0;
        const size_t off = (size_t)r * H + 4 * sub;
        float4 ai = zero4(), gq = zero4();
        const int hub = (row_ok && A.hubidx) ? A.hubidx[node] : -1;
        if (hub >= 0 && lane_ok) {
            ai = ld4(A.AIhub + ((size_t)b * A.n_hub + hub) * H + 4 * sub);
            gq = ld4(A.GQhub + ((size_t)b * A.n_hub + hub) * H + 4 * sub);
        }
        const int start = (row_ok && hub < 0) ? A.rowptr[node] : 0, end = (row_ok && hub < 0) ? A.rowptr[node + 1] : 0;
        const size_t base = (size_t)b * A.n * H;
        gn_gather2<4>(A.col, start, end, ZI + base, A.q + base, H, sub, lane_ok, ai, gq);
        float4 zs = zero4(), zi = zero4(), vS = zero4(), vI = zero4(), vR = zero4(), yS = zero4(), yI = zero4();
        float bt = 0.f, gm = 0.f;
        if (ok) {
            zs = ld4(A.Z + off); zi = ld4(ZI + off);
            vS = ld4(A.vSI + off); vI = ld4(A.vSI + slab + off); vR = ld4(A.vR + off);
            if (A.part) { yS = ld4(A.y + off); yI = ld4(A.y + slab + off); }
        }
        if (row_ok) { bt = A.bg[(size_t)r * H]; gm = A.bg[(size_t)r * H + 1]; }
        if (A.fSI && ok) {
            // gnode_rhs_f32's expressions (k_gather), operation for operation
            const float nb = -bt;
            float4 dS, dI, dR;
            gn_rhs_row(nb, gm, ai, zs, zi, dS, dI, dR);
            st4(A.fSI + off, dS); st4(A.fSI + slab + off, dI);
            if (A.fR) st4(A.fR + off, dR);
        }
        if (A.f4 && ok) st4(A.f4 + off, zero4());
        if (A.gyR && ok) st4(A.gyR + off, zero4());
        if (A.gybg) {
            // d/dbeta: sum_h (v_I - v_S) AI Z_S;  d/dgamma: sum_h (v_R - v_I) Z_I   (every lane of the group takes part)
            float c0 = (vI.x - vS.x) * ai.x * zs.x + (vI.y - vS.y) * ai.y * zs.y + (vI.z - vS.z) * ai.z * zs.z +
                       (vI.w - vS.w) * ai.w * zs.w;
            float c1 = (vR.x - vI.x) * zi.x + (vR.y - vI.y) * zi.y + (vR.z - vI.z) * zi.z + (vR.w - vI.w) * zi.w;
            c0 = group_sum<LPR>(c0);
            c1 = group_sum<LPR>(c1);
            if (ok) st4(A.gybg + off, sub == 0 ? make_float4(c0, c1, 0.f, 0.f) : zero4());
        }
        if constexpr (BGX) {
            const float2 c = gn_bg_row<XorSum<LPR>>(vS, vI, vR, ai, zs, zi);       // idle lanes and rows hold zeros
            if (row_ok && sub == 0) gn_bg_accumulate(A.gx, (size_t)r, H, A.w, c);
        }
        if (!mat) continue;
        float4 dS, dI;
        // gn_dpre_row inline: the call reschedules this kernel
#define GN_VJP_DPRE(c)                                                     \
        {                                                                  \
            const float u = bt * (vI.c - vS.c);                            \
            dS.c = (u * ai.c) * (zs.c * (1.0f - zs.c));                    \
            dI.c = (gq.c + gm * (vR.c - vI.c)) * (zi.c * (1.0f - zi.c));   \
        }
        GN_VJP_DPRE(x) GN_VJP_DPRE(y) GN_VJP_DPRE(z) GN_VJP_DPRE(w)
#undef GN_VJP_DPRE
        __syncthreads();                       // previous tile fully consumed (also covers the W stage)
        if (lane_ok) {                         // idle lanes of a group (H/4 not a power of two) would write into the next row
            st4(Dt + (size_t)grp * H + 4 * sub, ok ? dS : zero4());
            st4(Dt + ((size_t)G + grp) * H + 4 * sub, ok ? dI : zero4());
            if (A.part) {
                st4(Yt + (size_t)grp * H + 4 * sub, yS);
                st4(Yt + ((size_t)G + grp) * H + 4 * sub, yI);
            }
        }
        __syncthreads();
        if (A.gySI) {
            // g_y = dpre W  (this lane: 4 columns of its own row, both slabs)
            float4 gS = zero4(), gI = zero4();
            const float* pS = Dt + (size_t)grp * H;
            const float* pI = Dt + ((size_t)G + grp) * H;
            for (int j = 0; j < H; ++j) {
                const float4 wv = lane_ok ? ld4(Wl + (size_t)j * H + 4 * sub) : zero4();
                const float s = pS[j], i = pI[j];
                gS.x = fmaf(s, wv.x, gS.x); gS.y = fmaf(s, wv.y, gS.y); gS.z = fmaf(s, wv.z, gS.z); gS.w = fmaf(s, wv.w, gS.w);
                gI.x = fmaf(i, wv.x, gI.x); gI.y = fmaf(i, wv.y, gI.y); gI.z = fmaf(i, wv.z, gI.z); gI.w = fmaf(i, wv.w, gI.w);
            }
            if (ok) { st4(A.gySI + off, gS); st4(A.gySI + slab + off, gI); }
        }
        if (A.part) {
            // gW[j][k] += sum_rows dpre[r][j] * y[r][k]   (thread owns entries e = tid + 256 m), gb[j] += sum_rows dpre[r][j]
            if (quad) {
#pragma unroll 2
                for (int rr = 0; rr < 2 * G; ++rr) {
                    const float4 yq = ld4(Yt + (size_t)rr * H + 4 * qc);
                    const float* d = Dt + (size_t)rr * H;
#pragma unroll
                    for (int a = 0; a < MAXA; ++a) {
                        const int j = j0 + R * a;
                        if (j < H) {
                            const float dj = d[j];
                            accW[4 * a] = fmaf(dj, yq.x, accW[4 * a]); accW[4 * a + 1] = fmaf(dj, yq.y, accW[4 * a + 1]);
                            accW[4 * a + 2] = fmaf(dj, yq.z, accW[4 * a + 2]); accW[4 * a + 3] = fmaf(dj, yq.w, accW[4 * a + 3]);
                        }
                    }
                }
            } else {
#pragma unroll
                for (int m = 0; m < MAXM; ++m) {
                    if (m < M) {
                        const int e = threadIdx.x + 256 * m;
                        if (e < nE) {
                            const int j = e / H, k = e % H;
                            float s = 0.f;
#pragma unroll 1
                            for (int rr = 0; rr < 2 * G; ++rr) s = fmaf(Dt[(size_t)rr * H + j], Yt[(size_t)rr * H + k], s);
                            accW[m] += s;
                        }
                    }
                }
            }
            if (threadIdx.x < H) {
#pragma unroll 4
                for (int rr = 0; rr < 2 * G; ++rr) accb += Dt[(size_t)rr * H + threadIdx.x];
            }
        }
    }
    if (!A.part) return;
    float* part = A.part + (size_t)blockIdx.x * A.part_stride;
    if (quad) {
#pragma unroll
        for (int a = 0; a < MAXA; ++a) {
            const int j = j0 + R * a;
            if (j < H) {
                float* pp = part + (size_t)j * H + 4 * qc;
                pp[0] += A.w * accW[4 * a]; pp[1] += A.w * accW[4 * a + 1];
                pp[2] += A.w * accW[4 * a + 2]; pp[3] += A.w * accW[4 * a + 3];
            }
        }
    } else {
#pragma unroll
        for (int m = 0; m < MAXM; ++m) {
            if (m < M) {
                const int e = threadIdx.x + 256 * m;
                if (e < nE) part[e] += A.w * accW[m];
            }
        }
    }
    if (threadIdx.x < H) part[nE + threadIdx.x] += A.w * accb;
}

// --------------------------------------------------------------------------- RK4 stage combinations
// torchdiffeq 0.2.2's rk4_alt_step_func on the augmented state with h = -dt; the adjoint's rate is -V, so h * (-V) = dt * V
// (negation is exact).  Over the S and I slabs (n4 float4s); mode 2, 3, 4 form stage `mode`'s (y, a), mode 5 the update
// of a (`as` = a in place).
__global__ __launch_bounds__(256) void k_rk4_stage(int mode, size_t n4, float dt, const float* __restrict__ y,
                                                   const float* a, const float* __restrict__ k1, const float* __restrict__ k2,
                                                   const float* __restrict__ k3, const float* __restrict__ V1,
                                                   const float* __restrict__ V2, const float* __restrict__ V3,
                                                   const float* __restrict__ V4, float* __restrict__ ys, float* as) {
    const float third = 1.0f / 3.0f, h = -dt;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const size_t o = 4 * i;
        const float4 av = ld4(a + o);
        float4 yo = zero4(), ao;
        if (mode == 2) {
            const float4 yv = ld4(y + o), c1 = ld4(k1 + o), u1 = ld4(V1 + o);
#define S2(c) yo.c = yv.c + h * c1.c * third; ao.c = av.c + dt * u1.c * third;
            S2(x) S2(y) S2(z) S2(w)
#undef S2
        } else if (mode == 3) {
            const float4 yv = ld4(y + o), c1 = ld4(k1 + o), c2 = ld4(k2 + o), u1 = ld4(V1 + o), u2 = ld4(V2 + o);
#define S3(c) yo.c = yv.c + h * (c2.c - c1.c * third); ao.c = av.c + dt * (u2.c - u1.c * third);
            S3(x) S3(y) S3(z) S3(w)
#undef S3
        } else if (mode == 4) {
            const float4 yv = ld4(y + o), c1 = ld4(k1 + o), c2 = ld4(k2 + o), c3 = ld4(k3 + o);
            const float4 u1 = ld4(V1 + o), u2 = ld4(V2 + o), u3 = ld4(V3 + o);
#define S4(c) yo.c = yv.c + h * (c1.c - c2.c + c3.c); ao.c = av.c + dt * (u1.c - u2.c + u3.c);
            S4(x) S4(y) S4(z) S4(w)
#undef S4
        } else {
            const float4 u1 = ld4(V1 + o), u2 = ld4(V2 + o), u3 = ld4(V3 + o), u4 = ld4(V4 + o);
#define S5(c) ao.c = av.c + (u1.c + 3.0f * (u2.c + u3.c) + u4.c) * dt * 0.125f;
            S5(x) S5(y) S5(z) S5(w)
#undef S5
        }
        if (mode != 5) st4(ys + o, yo);
        st4(as + o, ao);
    }
}

// --------------------------------------------------------------------------- host
// workgroups of pass 2 (= partial slots it writes): a fixed function of (rows, H)
static int vjp_grid(long rows, int H) {
    const int rpw = 256 / gn_lpr(H);
    return (int)std::min<long>(BWD_NWG, std::max<long>(1, (rows + rpw - 1) / rpw));
}

static size_t vjp_lds_bytes(int H, bool gy) {
    const int rpw = 256 / gn_lpr(H);
    return ((gy ? (size_t)H * H : 0) + (size_t)4 * rpw * H) * sizeof(float);
}

// W and the two tiles at H = 128: 80 KB of LDS
int gn_rhs_vjp_set_attributes() {
    GN_HIP(hipFuncSetAttribute((const void*)k_rhs_vjp<32, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    GN_HIP(hipFuncSetAttribute((const void*)k_rhs_vjp<32, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    GN_HIP(hipFuncSetAttribute((const void*)k_rhs_vjp<32, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    GN_HIP(hipFuncSetAttribute((const void*)k_rhs_vjp<32, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    return 0;
}

struct VjpOut {
    float* fSI = nullptr; float* fR = nullptr; float* f4 = nullptr;
    float* gySI = nullptr; float* gyR = nullptr; float* gybg = nullptr;
    float* part = nullptr; int part_stride = 0; float w = 1.f;
    float* gx = nullptr;      // accumulate w * (d/dbeta, d/dgamma) into gx columns 3, 4 (rows of 3+H floats)
};

// f and the VJP of (vSI, vR) at (y = S | I slabs, bg): node MLP, q table, hub sums, pass 2.  Z: 2 slabs, q: 1 slab of
// scratch; hub_scratch: gn_hub_scratch_bytes(g, B, H, 2).
static int vjp_launch(const gnode_graph_s* g, long rows, int H, const float* y, const float* bg, const float* vSI,
                      const float* vR, const float* W, const float* b, float* Z, float* q, void* hub_scratch, const VjpOut& o,
                      hipStream_t st) {
    const bool need_q = o.gySI || o.part;
    if (!(o.fSI || o.f4 || o.gySI || o.gyR || o.gybg || o.part || o.gx)) return 0;
    const size_t slab = (size_t)rows * H;
    if (int e = gn_launch_mlp_any(g, y, W, b, Z, 2 * rows, H, st)) return e;      // Z_S | Z_I (Z_R is dead work)
    if (need_q) {
        const unsigned qgrid = (unsigned)std::min<size_t>((slab / 4 + 255) / 256, 2048);
        hipLaunchKernelGGL(k_vjp_q, dim3(qgrid), dim3(256), 0, st, vSI, Z, bg, q, rows, H);
        GN_LAUNCH_CHECK();
    }
    const float* qt = need_q ? q : Z + slab;          // (without g_y / gW / gb the second table is never used)
    const float *AIhub = nullptr, *GQhub = nullptr;
    if (int e = gn_hub_gather(g, rows / g->info.n, H, Z + slab, qt, hub_scratch, &AIhub, &GQhub, st)) return e;
    VjpArgs A;
    A.rowptr = g->rowptr; A.col = g->col; A.n = g->info.n; A.rows = rows; A.H = H;
    A.y = y; A.bg = bg; A.Z = Z; A.q = qt; A.vSI = vSI; A.vR = vR; A.W = W;
    A.hubidx = g->hubidx; A.AIhub = AIhub; A.GQhub = GQhub; A.n_hub = g->info.n_hub;
    A.fSI = o.fSI; A.fR = o.fR; A.f4 = o.f4; A.gySI = o.gySI; A.gyR = o.gyR; A.gybg = o.gybg;
    A.part = o.part; A.part_stride = o.part_stride; A.w = o.w; A.gx = o.gx;
    const int lpr = gn_lpr(H);
    const size_t lds = vjp_lds_bytes(H, o.gySI != nullptr);
    const dim3 grid(vjp_grid(rows, H));
    if (o.gx) {
        if (256 % H == 0) GN_LPR_DISPATCH(32, lpr, hipLaunchKernelGGL((k_rhs_vjp<LPR, true, true>), grid, dim3(256), lds, st, A))
        else GN_LPR_DISPATCH(32, lpr, hipLaunchKernelGGL((k_rhs_vjp<LPR, false, true>), grid, dim3(256), lds, st, A))
    } else {
        if (256 % H == 0) GN_LPR_DISPATCH(32, lpr, hipLaunchKernelGGL((k_rhs_vjp<LPR, true>), grid, dim3(256), lds, st, A))
        else GN_LPR_DISPATCH(32, lpr, hipLaunchKernelGGL((k_rhs_vjp<LPR, false>), grid, dim3(256), lds, st, A))
    }
    GN_LAUNCH_CHECK();
    return 0;
}

static size_t slabs_bytes(int64_t rows, int32_t H, int k) { return gn_align((size_t)k * rows * H * sizeof(float)); }

static size_t rhs_vjp_fixed_bytes(int64_t rows, int32_t H) {
    // Z[2], q[1] slabs + the partial slots + the reduced-gradient dump for outputs not asked for
    return slabs_bytes(rows, H, 2) + slabs_bytes(rows, H, 1) +
           gn_align((size_t)vjp_grid(rows, H) * (H * H + H) * sizeof(float)) + gn_align((size_t)(H * H + H) * sizeof(float));
}

extern "C" size_t gnode_rhs_vjp_workspace_bytes(gnode_graph_t g, int64_t rows, int32_t H) {
    if (!g || rows <= 0 || H < 4 || H > 128 || H % 4 || rows % g->info.n) return 0;
    return rhs_vjp_fixed_bytes(rows, H) + gn_hub_scratch_bytes(g, rows / g->info.n, H, 2);
}

extern "C" int gnode_rhs_vjp_f32(gnode_graph_t g, const float* y, const float* W, const float* b, const float* v, float* f_out,
                                 float* gy_out, float* gW_out, float* gb_out, int64_t rows, int32_t H, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    GN_CHECK_ARG(g && y && W && b && v && workspace, "gnode_rhs_vjp_f32: null pointer");
    GN_CHECK_ARG(H >= 4 && H <= 128 && H % 4 == 0, "gnode_rhs_vjp_f32: need 4 <= H <= 128, H %% 4 == 0 (got %d)", H);
    GN_CHECK_ARG(rows > 0 && rows % g->info.n == 0, "gnode_rhs_vjp_f32: rows=%lld is not a multiple of graph n=%d",
                 (long long)rows, g->info.n);
    if (workspace_bytes < gnode_rhs_vjp_workspace_bytes(g, rows, H)) {
        gnode_set_error("gnode_rhs_vjp_f32: workspace %zu < %zu", workspace_bytes, gnode_rhs_vjp_workspace_bytes(g, rows, H));
        return GNODE_ERR_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t slab = (size_t)rows * H;
    char* ws = (char*)workspace;
    float* Z = (float*)ws;
    float* q = (float*)(ws + slabs_bytes(rows, H, 2));
    char* after_q = ws + slabs_bytes(rows, H, 2) + slabs_bytes(rows, H, 1);      // (the layout of rhs_vjp_fixed_bytes)
    float* part = (float*)after_q;
    const int nwg = vjp_grid(rows, H);
    float* dump = (float*)(after_q + gn_align((size_t)nwg * (H * H + H) * sizeof(float)));
    void* hub_scratch = ws + rhs_vjp_fixed_bytes(rows, H);
    const bool want_p = gW_out || gb_out;
    if (want_p)
        if (int e = gn_zero_async(part, (size_t)nwg * (H * H + H) * sizeof(float), st)) return e;
    VjpOut o;
    if (f_out) { o.fSI = f_out; o.fR = f_out + 2 * slab; o.f4 = f_out + 3 * slab; }
    if (gy_out) { o.gySI = gy_out; o.gyR = gy_out + 2 * slab; o.gybg = gy_out + 3 * slab; }
    if (want_p) { o.part = part; o.part_stride = H * H + H; o.w = 1.f; }
    if (int e = vjp_launch(g, rows, H, y, y + 3 * slab, v, v + 2 * slab, W, b, Z, q, hub_scratch, o, st)) return e;
    if (want_p) {
        // outputs not asked for are reduced into the workspace's dump area
        float* dW = gW_out ? gW_out : dump;
        float* db = gb_out ? gb_out : dump + H * H;
        if (int e = gn_launch_reduce_parts(part, nwg, H, dW, db, st)) return e;
    }
    return 0;
}

// --------------------------------------------------------------------------- RK4 adjoint
// torchdiffeq 0.2.2 odeint_adjoint(..., method='rk4') on the fixed grid: per interval i = G-1 .. 1 one
// 3/8-rule step of size h = -dt from t_i to t_{i-1} of the augmented system (f(y), -a^T df/dy, -a^T df/dtheta), y reset to
// sol[i-1] and dL/dsol[i-1] added after it.  The beta-gamma slab's adjoint feeds nothing and is not carried; g_y[R] = 0, so
// a_R is constant inside an interval and only the S and I slabs of the stage states are formed.
static size_t rk4_fixed_bytes(int64_t rows, int32_t H) {
    const PartLayout L{H};
    // a[3], y stage[2], a stage[2], k1..k3[2 each], V1..V4[2 each], Z[2], q[1] slabs + the partial slots
    return slabs_bytes(rows, H, 3) + 2 * slabs_bytes(rows, H, 2) + 7 * slabs_bytes(rows, H, 2) + slabs_bytes(rows, H, 2) +
           slabs_bytes(rows, H, 1) + gn_align((size_t)BWD_NWG * L.total() * sizeof(float));
}

extern "C" size_t gnode_backward_rk4_workspace_bytes(gnode_graph_t g, int64_t rows, int32_t H) {
    if (!g || rows <= 0 || H < 4 || H > 128 || H % 4 || rows % g->info.n) return 0;
    return rk4_fixed_bytes(rows, H) + gn_hub_scratch_bytes(g, rows / g->info.n, H, 2);
}

extern "C" int gnode_backward_rk4_dx_f32(gnode_graph_t g, const float* x, const gnode_params* p, const float* dt_host,
                                         int32_t n_steps, const int32_t* out_rows_host, int32_t n_out, const float* sol,
                                         const float* gS, const float* gI, const float* gR, const gnode_params* grads,
                                         int64_t rows, int32_t H, void* workspace, size_t workspace_bytes, void* stream,
                                         float* gx) {
    GN_CHECK_ARG(g && x && p && sol && gS && gI && gR && workspace, "gnode_backward_rk4_f32: null pointer");
    GN_CHECK_ARG(grads || gx, "gnode_backward_rk4_dx_f32: neither grads nor gx requested");
    GN_CHECK_ARG(n_steps >= 0 && (n_steps == 0 || dt_host), "gnode_backward_rk4_f32: bad n_steps/dt");
    GN_CHECK_ARG(H >= 4 && H <= 128 && H % 4 == 0, "gnode_backward_rk4_f32: need 4 <= H <= 128, H %% 4 == 0 (got %d)", H);
    GN_CHECK_ARG(rows > 0 && rows % g->info.n == 0, "gnode_backward_rk4_f32: rows=%lld is not a multiple of graph n=%d",
                 (long long)rows, g->info.n);
    GN_CHECK_ARG(p->odefunc_linear_weight && p->odefunc_linear_bias && p->linear3_weight && p->linear3_bias &&
                     p->linearS2_weight && p->linearS2_bias && p->linearS1_weight && p->linearS1_bias,
                 "gnode_backward_rk4_f32: null parameter pointer");
    GN_CHECK_ARG(!grads || (grads->odefunc_linear_weight && grads->odefunc_linear_bias && grads->linearS1_weight &&
                     grads->linearS1_bias && grads->linear3_weight && grads->linear3_bias && grads->linearS2_weight &&
                     grads->linearS2_bias), "gnode_backward_rk4_f32: null gradient pointer");
    if (workspace_bytes < gnode_backward_rk4_workspace_bytes(g, rows, H)) {
        gnode_set_error("gnode_backward_rk4_f32: workspace %zu < %zu", workspace_bytes, gnode_backward_rk4_workspace_bytes(g, rows, H));
        return GNODE_ERR_WORKSPACE;
    }
    const int G = n_steps + 1;
    if (int e = gn_check_out_rows("gnode_backward_rk4_f32", out_rows_host, n_out, G)) return e;
    const std::vector<int> slot = gn_out_slots(out_rows_host, n_out, G);
    hipStream_t st = (hipStream_t)stream;
    const PartLayout L{H};
    const size_t slab = (size_t)rows * H, s2 = slabs_bytes(rows, H, 2);
    char* ws = (char*)workspace;
    char* cur = ws;
    auto take = [&](size_t bytes) { float* r = (float*)cur; cur += bytes; return r; };
    float* a = take(slabs_bytes(rows, H, 3));
    float* ys = take(s2);
    float* as = take(s2);
    float* k[3] = {take(s2), take(s2), take(s2)};
    float* V[4] = {take(s2), take(s2), take(s2), take(s2)};
    float* Z = take(s2);
    float* q = take(slabs_bytes(rows, H, 1));
    float* part = take(gn_align((size_t)BWD_NWG * L.total() * sizeof(float)));
    void* hub_scratch = ws + rk4_fixed_bytes(rows, H);
    {
        GnZeroRegions zr;
        zr.n = 2;
        zr.p[0] = a; zr.bytes[0] = 3 * slab * sizeof(float);
        zr.p[1] = part; zr.bytes[1] = (size_t)BWD_NWG * L.total() * sizeof(float);
        if (int e = gn_zero_regions_async(zr, st)) return e;
    }
    // the stage VJPs accumulate columns 3, 4 in place and the encoder writes 0-2: the rest stays 0
    if (gx)
        if (int e = gn_zero_async(gx, (size_t)rows * (3 + H) * sizeof(float), st)) return e;
    int slots_used = 1;
    auto head = [&](int gi) -> int {
        const int s = slot[gi];
        if (s < 0) return 0;
        return gn_launch_head_bwd(rows, H, sol + (size_t)gi * 4 * slab, gS + (size_t)s * rows, gI + (size_t)s * rows,
                                  gR + (size_t)s * rows, p, a, part, &slots_used, st);
    };
    if (int e = head(G - 1)) return e;
    const float* bg = sol + 3 * slab;                 // beta, gamma: grid point 0's 4th slab (constant along the trajectory)
    const float* W = p->odefunc_linear_weight;
    const float* bb = p->odefunc_linear_bias;
    const size_t n4 = 2 * slab / 4;
    const unsigned cgrid = (unsigned)std::min<size_t>((n4 + 255) / 256, 2048);
    const int nwg = vjp_grid(rows, H);
    for (int i = G - 1; i >= 1; --i) {
        const float dt = dt_host[i - 1];
        const float* yi = sol + (size_t)i * 4 * slab;
        const float wts[4] = {dt * 0.125f, dt * 0.375f, dt * 0.375f, dt * 0.125f};
        for (int s = 0; s < 4; ++s) {
            VjpOut o;
            if (s < 3) o.fSI = k[s];                  // k4 is never needed: y is reset to sol[i-1] after the step
            o.gySI = V[s];
            o.part = part; o.part_stride = L.total(); o.w = wts[s];
            o.gx = gx;
            if (int e = vjp_launch(g, rows, H, s == 0 ? yi : ys, bg, s == 0 ? a : as, a + 2 * slab, W, bb, Z, q, hub_scratch,
                                   o, st))
                return e;
            hipLaunchKernelGGL(k_rk4_stage, dim3(cgrid), dim3(256), 0, st, s < 3 ? s + 2 : 5, n4, dt, yi, a, k[0], k[1], k[2],
                               V[0], V[1], V[2], V[3], ys, s < 3 ? as : a);
            GN_LAUNCH_CHECK();
        }
        slots_used = std::max(slots_used, nwg);
        if (int e = head(i - 1)) return e;
    }
    if (int e = gn_launch_enc_bwd(rows, H, a, sol, x, part, &slots_used, st, gx, p->linearS1_weight)) return e;
    return grads ? gn_launch_reduce_all(part, slots_used, H, grads, st) : 0;
}

extern "C" int gnode_backward_rk4_f32(gnode_graph_t g, const float* x, const gnode_params* p, const float* dt_host,
                                      int32_t n_steps, const int32_t* out_rows_host, int32_t n_out, const float* sol,
                                      const float* gS, const float* gI, const float* gR, const gnode_params* grads,
                                      int64_t rows, int32_t H, void* workspace, size_t workspace_bytes, void* stream) {
    GN_CHECK_ARG(grads, "gnode_backward_rk4_f32: null pointer");
    return gnode_backward_rk4_dx_f32(g, x, p, dt_host, n_steps, out_rows_host, n_out, sol, gS, gI, gR, grads, rows, H, workspace,
                                     workspace_bytes, stream, nullptr);
}
