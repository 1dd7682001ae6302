// Lane-group helpers of the generic-H kernels (a row of H features lives 4 per lane in a group of LPR = H/4 lanes):
// the node MLP as a lane-group mat-vec.  Shared by gnode_ode.hip (one launch per
// Euler step) and gnode_persg.hip (the whole integration in one launch).
#pragma once
#include "gnode_row.h"

// Node MLP of one row: sigmoid(W x + b).  x_k is broadcast inside the group by shuffle and multiplied with W^T (staged in LDS,
// Wt[k][j] = W[j][k]); every lane of the wave must call it (shuffles), `active` guards the LDS reads.
template <int LPR>
__device__ __forceinline__ float4 group_mlp(float4 x, const float* __restrict__ Wt, float4 bias4, int sub, bool active,
                                            int H) {
    float4 acc = bias4;
    const float xv[4] = {x.x, x.y, x.z, x.w};
    for (int kk = 0; 4 * kk < H; ++kk) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float xk = __shfl(xv[c], kk, LPR);
            if (active) {
                const float4 w = ld4(Wt + (size_t)(4 * kk + c) * H + 4 * sub);
                acc.x = fmaf(xk, w.x, acc.x); acc.y = fmaf(xk, w.y, acc.y);
                acc.z = fmaf(xk, w.z, acc.z); acc.w = fmaf(xk, w.w, acc.w);
            }
        }
    }
    return make_float4(gn_sigmoid(acc.x), gn_sigmoid(acc.y), gn_sigmoid(acc.z), gn_sigmoid(acc.w));
}

