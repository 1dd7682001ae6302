// The DMP recurrence, stated once for the marginals and their reverse sweep (gnode_dmp.hip), for the source scores
// (gnode_dmp_source.hip) and for the outbreak sizes (gnode_dmp_outbreak.hip): the four dmp_* functions below and nothing else.  They work on values and on pointers that are
// already the sample's own, in global memory or in LDS.  The library is built with -ffp-contract=off, so they round as
// written wherever they are inlined; their operand order is the reference's.
#pragma once
#include "gnode_common.h"

// t = 1 (dmp.py:104-121): theta_1 = 1 - w phi_0 + 1e-10, phi_0 = Pi0[src] (what 1 - Ps0 is when Pr0 = 0), Ps_e^{prev} = Ps0[src]
__device__ __forceinline__ void dmp_edge_start(float ps0_u, float pi0_u, float w_e, float& theta, float& phi, float& ps) {
    theta = (1.0f - w_e * pi0_u) + 1e-10f;
    phi = pi0_u;
    ps = ps0_u;
}

// P_k: theta of the reverses of row k's edges [lo, hi), in ascending position from 1
__device__ __forceinline__ float dmp_row_product(const int* rev, const float* theta, int lo, int hi) {
    float p = 1.0f;
    for (int e = lo; e < hi; ++e) p = p * theta[rev[e]];
    return p;
}

// the marginals of node k at this step from P_k and the previous step's Pi_k, Pr_k
__device__ __forceinline__ void dmp_node_update(float P_k, float ps0_k, float pi_prev, float pr_prev, float gamma_k, float& ps,
                                                float& pi, float& pr) {
    ps = ps0_k * P_k;
    pr = pr_prev + gamma_k * pi_prev;
    pi = 1.0f - ps - pr;
}

// Ps_e and phi_e of this step (in place), theta_e of the NEXT step; `theta` is a reference so that it is loaded where it is used
__device__ __forceinline__ void dmp_edge_update(float P_u, float theta_rev, float ps0_u, float w_e, float gamma_u, float& phi,
                                                float& ps, const float& theta, float& theta_next) {
    const float mul = P_u / theta_rev;
    const float ps_new = ps0_u * mul;
    const float ph = (1.0f - w_e) * (1.0f - gamma_u) * phi - (ps_new - ps);
    phi = ph;
    ps = ps_new;
    theta_next = theta - w_e * ph;
}

// The fp64 sums of gnode_dmp_source.hip and gnode_dmp_outbreak.hip, in a fixed order.  The sum of the 64 lanes' values in lane 0:
// a fixed tree, 32 16 8 4 2 1 (every lane of the wave is active where this is called)
__device__ __forceinline__ double dmp_wave_sum(double v) {
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off, 64);
    return v;
}
__device__ __forceinline__ double dmp_sum_in_order(const double* v, int count) {
    double s = 0.0;
    for (int i = 0; i < count; ++i) s = s + v[i];
    return s;
}

__host__ __device__ static inline size_t dmp_align16(size_t x) { return (x + 15) / 16 * 16; }
static constexpr size_t kDmpLdsLimit = 160 * 1024;      // what a gfx950 workgroup may declare
