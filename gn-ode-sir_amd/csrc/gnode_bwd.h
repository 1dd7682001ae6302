// Shared pieces of the adjoint backward (gnode_bwd.hip, gnode_bwd_tiny.hip).
#pragma once
#include "gnode_common.h"

// BWD_NWG, the partial-gradient slots of a call: gnode_graph_plan.h (the adjoint sweep's plan is bound by it)

// partial-buffer layout per workgroup (floats)
struct PartLayout {
    int H;
    __host__ __device__ int oW() const { return 0; }
    __host__ __device__ int ob() const { return H * H; }
    __host__ __device__ int ow3() const { return H * H + H; }
    __host__ __device__ int ob3() const { return H * H + 5 * H; }
    __host__ __device__ int ow2() const { return H * H + 5 * H + 4; }
    __host__ __device__ int ob2() const { return H * H + 5 * H + 8; }
    __host__ __device__ int ow1() const { return H * H + 5 * H + 9; }
    __host__ __device__ int ob1() const { return H * H + 6 * H + 9; }
    __host__ __device__ int total() const { return H * H + 7 * H + 9; }
};

// Whole adjoint sweep of a batch of tiny graphs (n <= 64, H = 64) in ONE launch; writes partial slot b for sample b.
bool gn_tiny_bwd64_ok(const gnode_graph_s* g, long rows, int H, int n_steps);
int gn_launch_tiny_bwd64(const gnode_graph_s* g, long rows, const float* x, const gnode_params* p, const float* dt_host,
                         int n_steps, const int32_t* out_rows_host, int n_out, const float* sol, const float* gS,
                         const float* gI, const float* gR, float* part,
                         const float* keep /* the forward's kept activations, or null = recompute */, hipStream_t st);

// Pieces of gnode_backward_f32's generic path, shared with the RK4 adjoint (gnode_rhs_vjp.hip).  Each raises *slots_used to
// the partial slots it wrote.
// head backward at one grid point: a[3 slabs] += its VJP, linear3 / linearS2 partials into slots of PartLayout{H}
int gn_launch_head_bwd(long rows, int H, const float* Ysol, const float* gS, const float* gI, const float* gR,
                       const gnode_params* p, float* a, float* part, int* slots_used, hipStream_t st);
// encoder backward on a_0: linearS1 partials; with gx, also dL/d(S0, I0, R0) into its columns 0-2 (w1 = linearS1.weight)
int gn_launch_enc_bwd(long rows, int H, const float* a, const float* sol0, const float* x, float* part, int* slots_used,
                      hipStream_t st, float* gx = nullptr, const float* w1 = nullptr);
// fixed-order sum of slots [0, nwg) of PartLayout{H} into the 8 gradients (overwritten)
int gn_launch_reduce_all(const float* part, int nwg, int H, const gnode_params* grads, hipStream_t st);
// the same for slots of [H*H gW | H gb] into dW, db
int gn_launch_reduce_parts(const float* part, int nwg, int H, float* dW, float* db, hipStream_t st);
// node MLP Z = sigmoid(X W^T + b) of nrows rows (gnode_ode.hip)
int gn_launch_mlp_any(const gnode_graph_s* g, const float* X, const float* W, const float* b, float* Z, long nrows, int H,
                      hipStream_t st);

// H = 128: a += dt dpre W, gW, gb on the matrix cores (gnode_h128.hip); raises *slots_used to its grid size
int gn_launch_bwd_mlp128(const gnode_graph_s* g, const float* dpre, const float* Ysol, const float* W, float dt, float* a, long rows,
                         float* part, int* slots_used, hipStream_t st);
