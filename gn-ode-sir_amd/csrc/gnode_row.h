// The model's per-row arithmetic, shared by the GN-ODE kernels.  A row of H features is held 4 per lane by a group of
// lanes.  Paths that must agree bit for bit (persistent against per-step, fused against unfused, the RHS VJP's f against
// gnode_rhs_f32) agree because they compute these definitions.  A few sites keep an inline copy because calling the
// helper reschedules their instructions; each names the helper it mirrors operation for operation, and must change with it.
#pragma once
#include <hip/hip_runtime.h>

// 1 / (1 + exp(-x)) with the hardware exp2/rcp (v_exp_f32, v_rcp_f32: 1 ulp each).  __frcp_rn would expand to the
// IEEE-exact division sequence (~10 VALU instructions per value) for nothing: the result is within 2e-7 either way.
__device__ __forceinline__ float gn_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float dot4(float4 a, float4 b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, a.w * b.w))); }

// ---- sums over the lanes that hold one row, result in every lane.  The two add in different orders, so each caller
// names the one it uses; a template that sums takes it as its Sum parameter.
template <int LPR>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int m = LPR / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, LPR);
    return v;
}
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
// a 16-lane group is exactly one DPP row: mirror, half-mirror, xor2, xor1
__device__ __forceinline__ float row_sum16(float v) {
    v += dpp_f<0x140>(v);   // row_mirror        i <-> 15-i
    v += dpp_f<0x141>(v);   // row_half_mirror   i <-> 7-i within each half
    v += dpp_f<0x4E>(v);    // quad_perm [2,3,0,1]
    v += dpp_f<0xB1>(v);    // quad_perm [1,0,3,2]
    return v;
}
template <int LPR>
struct XorSum { static __device__ __forceinline__ float sum(float v) { return group_sum<LPR>(v); } };
struct DppSum16 { static __device__ __forceinline__ float sum(float v) { return row_sum16(v); } };

// ---- the SIR right-hand side of one row (ode_nn_ngraph_sim.py:75-77), nb = -beta:
// dS = nb (AI Z_S), dR = gamma Z_I, dI = -dS - dR
__device__ __forceinline__ void gn_rhs_row(float nb, float gm, float4 ai, float4 zs, float4 zi, float4& dS, float4& dI,
                                           float4& dR) {
    dS.x = nb * (ai.x * zs.x); dS.y = nb * (ai.y * zs.y); dS.z = nb * (ai.z * zs.z); dS.w = nb * (ai.w * zs.w);
    dR.x = gm * zi.x; dR.y = gm * zi.y; dR.z = gm * zi.z; dR.w = gm * zi.w;
    dI.x = -dS.x - dR.x; dI.y = -dS.y - dR.y; dI.z = -dS.z - dR.z; dI.w = -dS.w - dR.w;
}
// one Euler step of a float4 of state: y += dt d
__device__ __forceinline__ float4 gn_euler4(float4 y, float dt, float4 d) {
    return make_float4(y.x + dt * d.x, y.y + dt * d.y, y.z + dt * d.z, y.w + dt * d.w);
}
// what the persistent H = 64 forward keeps for the backward under `keep`: P_S = AI Z_S (1 - Z_S)
__device__ __forceinline__ float4 gn_kept_ps(float4 ai, float4 zs) {
    return make_float4(ai.x * (zs.x * (1.0f - zs.x)), ai.y * (zs.y * (1.0f - zs.y)), ai.z * (zs.z * (1.0f - zs.z)),
                       ai.w * (zs.w * (1.0f - zs.w)));
}

// ---- read-out head of one row: Linear(4,1)(relu(Linear(H,4)(y))) for S, I, R (ode_nn_ngraph_sim.py:172-182), then the
// 3-way softmax (:184-187).  w3 gives the lane's 4 columns of linear3's row k: W3Rows reads them from memory, a float4[4]
// holds them in registers.  b3[k], w2[k] and b2 come from memory or registers alike: the same operations, so the same bits.
// Every lane of the group returns the same values.
struct W3Rows {          // linear3 in memory, rows of `stride` floats; idle lanes take 0
    const float* w3;
    int stride, sub;
    bool active;
};
__device__ __forceinline__ float4 w3_col(const W3Rows& s, int k) {
    return s.active ? ld4(s.w3 + (size_t)k * s.stride + 4 * s.sub) : zero4();
}
__device__ __forceinline__ float4 w3_col(const float4 (&w3)[4], int k) { return w3[k]; }
template <class Sum, class W3, class B3, class W2>
__device__ __forceinline__ void gn_readout(float4 yS, float4 yI, float4 yR, const W3& w3, const B3& b3,
                                           const W2& w2, float b2, float& pS, float& pI, float& pR) {
    float qS = b2, qI = b2, qR = b2;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float4 w = w3_col(w3, k);
        float s = dot4(w, yS), i = dot4(w, yI), r = dot4(w, yR);
        s = Sum::sum(s) + b3[k];
        i = Sum::sum(i) + b3[k];
        r = Sum::sum(r) + b3[k];
        qS = fmaf(w2[k], fmaxf(s, 0.f), qS);
        qI = fmaf(w2[k], fmaxf(i, 0.f), qI);
        qR = fmaf(w2[k], fmaxf(r, 0.f), qR);
    }
    const float m = fmaxf(qS, fmaxf(qI, qR));
    const float eS = __expf(qS - m), eI = __expf(qI - m), eR = __expf(qR - m);
    const float inv = __builtin_amdgcn_rcpf(eS + eI + eR);
    pS = eS * inv; pI = eI * inv; pR = eR * inv;
}

// ---- the adjoint's pieces of one row (gnode_bwd.hip's header has the sweep), u = the adjoint a (or the RHS VJP's v)
// q table: beta (u_I - u_S) Z_S, gathered through A^T into dZ_I
__device__ __forceinline__ float4 gn_q4(float bt, float4 uI, float4 uS, float4 z) {
    return make_float4(bt * (uI.x - uS.x) * z.x, bt * (uI.y - uS.y) * z.y, bt * (uI.z - uS.z) * z.z, bt * (uI.w - uS.w) * z.w);
}
// dpre = dZ * Z (1 - Z) with dZ_S = v AI, v = beta (u_I - u_S), and dZ_I = gq + gamma (u_R - u_I), gq = A^T q
#define GN_DPRE_ROW(c, DS)                                                  \
    {                                                                       \
        const float v = bt * (uI.c - uS.c);                                 \
        dS.c = DS;                                                          \
        dI.c = (gq.c + gm * (uR.c - uI.c)) * (zi.c * (1.0f - zi.c));        \
    }
__device__ __forceinline__ void gn_dpre_row(float bt, float gm, float4 uS, float4 uI, float4 uR, float4 ai, float4 gq, float4 zs,
                                            float4 zi, float4& dS, float4& dI) {
    GN_DPRE_ROW(x, (v * ai.x) * (zs.x * (1.0f - zs.x))) GN_DPRE_ROW(y, (v * ai.y) * (zs.y * (1.0f - zs.y)))
    GN_DPRE_ROW(z, (v * ai.z) * (zs.z * (1.0f - zs.z))) GN_DPRE_ROW(w, (v * ai.w) * (zs.w * (1.0f - zs.w)))
}
// the same over kept activations: ps = P_S = AI Z_S (1 - Z_S) as the forward stored it, so dS = v * P_S (other rounding)
__device__ __forceinline__ void gn_dpre_row_kept(float bt, float gm, float4 uS, float4 uI, float4 uR, float4 ps, float4 gq,
                                                 float4 zi, float4& dS, float4& dI) {
    GN_DPRE_ROW(x, v * ps.x) GN_DPRE_ROW(y, v * ps.y) GN_DPRE_ROW(z, v * ps.z) GN_DPRE_ROW(w, v * ps.w)
}
#undef GN_DPRE_ROW
// the adjoint of the beta-gamma slab (ODEBlock input gradient): this lane's 4 columns of
//   d/dbeta = sum_h (u_I - u_S) AI Z_S        d/dgamma = sum_h (u_R - u_I) Z_I
__device__ __forceinline__ float2 gn_bg_part(float4 uS, float4 uI, float4 uR, float4 ai, float4 zs, float4 zi) {
    const float c0 = (uI.x - uS.x) * ai.x * zs.x + (uI.y - uS.y) * ai.y * zs.y + (uI.z - uS.z) * ai.z * zs.z +
                     (uI.w - uS.w) * ai.w * zs.w;
    const float c1 = (uR.x - uI.x) * zi.x + (uR.y - uI.y) * zi.y + (uR.z - uI.z) * zi.z + (uR.w - uI.w) * zi.w;
    return make_float2(c0, c1);
}
// ... summed over the lanes that hold the row (fixed order; every lane of the group must take part, idle lanes with zeros),
// result in every lane
template <class Sum>
__device__ __forceinline__ float2 gn_bg_row(float4 uS, float4 uI, float4 uR, float4 ai, float4 zs, float4 zi) {
    const float2 c = gn_bg_part(uS, uI, uR, ai, zs, zi);
    return make_float2(Sum::sum(c.x), Sum::sum(c.y));
}
// gx[row][3], gx[row][4] += w * (d/dbeta, d/dgamma): one lane per row, rows of 3 + H floats (the layout of x)
__device__ __forceinline__ void gn_bg_accumulate(float* __restrict__ gx, size_t row, int H, float w, float2 c) {
    float* p = gx + row * (size_t)(3 + H) + 3;
    p[0] += w * c.x;
    p[1] += w * c.y;
}

// per-lane-group accumulators of the read-out head's parameter gradients
struct HeadAcc {
    float4 dw3[4];
    float db3[4], dw2[4], db2;
};

// VJP of the read-out head softmax(linearS2(relu(linear3(y_X)))) at one row (ode_nn_ngraph_sim.py:172-187): a_X += dL/dy_X.
// Its reciprocal is 1 / (...), not the forward's v_rcp_f32.
template <class Sum>
__device__ __forceinline__ void gn_head_vjp(const float4 (&y)[3], const float (&gout)[3], const float4 (&w3v)[4],
                                           const float* __restrict__ b3, const float* __restrict__ w2,
                                           const float* __restrict__ b2, float4& aS, float4& aI, float4& aR, HeadAcc& acc) {
    float p3[3][4], q[3];
#pragma unroll
    for (int X = 0; X < 3; ++X) {
        q[X] = b2[0];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            p3[X][k] = Sum::sum(dot4(w3v[k], y[X])) + b3[k];
            q[X] = fmaf(w2[k], fmaxf(p3[X][k], 0.f), q[X]);
        }
    }
    const float m = fmaxf(q[0], fmaxf(q[1], q[2]));
    const float e0 = __expf(q[0] - m), e1 = __expf(q[1] - m), e2 = __expf(q[2] - m);
    const float inv = 1.0f / (e0 + e1 + e2);
    const float pr[3] = {e0 * inv, e1 * inv, e2 * inv};
    const float gp = gout[0] * pr[0] + gout[1] * pr[1] + gout[2] * pr[2];
    float4* av[3] = {&aS, &aI, &aR};
#pragma unroll
    for (int X = 0; X < 3; ++X) {
        const float dq = pr[X] * (gout[X] - gp);
        float4 dy = zero4();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float dp3 = p3[X][k] > 0.f ? dq * w2[k] : 0.f;
            dy.x = fmaf(dp3, w3v[k].x, dy.x); dy.y = fmaf(dp3, w3v[k].y, dy.y);
            dy.z = fmaf(dp3, w3v[k].z, dy.z); dy.w = fmaf(dp3, w3v[k].w, dy.w);
            acc.dw3[k].x = fmaf(dp3, y[X].x, acc.dw3[k].x); acc.dw3[k].y = fmaf(dp3, y[X].y, acc.dw3[k].y);
            acc.dw3[k].z = fmaf(dp3, y[X].z, acc.dw3[k].z); acc.dw3[k].w = fmaf(dp3, y[X].w, acc.dw3[k].w);
            acc.db3[k] += dp3;
            acc.dw2[k] = fmaf(dq, fmaxf(p3[X][k], 0.f), acc.dw2[k]);
        }
        acc.db2 += dq;
        av[X]->x += dy.x; av[X]->y += dy.y; av[X]->z += dy.z; av[X]->w += dy.w;
    }
}

