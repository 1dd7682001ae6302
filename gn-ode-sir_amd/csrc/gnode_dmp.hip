// Dynamic message passing baseline for SIR on MI355X (gfx950) -- SURVEY 8f rank 4.
//
// Restates DMP_SIR of the reference (dmp.py:74-170): messages live on the directed edges e = (src -> tar) of the
// weighted adjacency in COO row-major order (dmp.py:67-72 = the CSR positions of the graph handle);
//   theta_e   <- theta_e - w_e phi_e
//   P_k        = prod_{e: tar(e) = k} theta_e                 (torch_scatter scatter(reduce='mul'), :93-100)
//   Ps_e       = Ps0[src] * P[src] / theta_{rev(e)}           (the cavity product, :96-99)
//   phi_e     <- (1 - w_e)(1 - gamma_src) phi_e - (Ps_e - Ps_e^{prev})
//   marginals  Ps_k = Ps0_k P_k,  Pr_k += gamma_k Pi_k,  Pi_k = 1 - Ps_k - Pr_k       (:124-129, :141-145)
// Undirected graphs only (every shipped graph is `.to_undirected()`, ode_nn.py:402): the edges INTO k are then the
// reverses of row k's edges, so one CSR serves both directions and P_k multiplies theta_{rev(e)} over row k in
// ascending order -- the order the reference's CPU scatter uses.  fp32 like the reference's FloatTensors.
//
// This unit is the constant-rates instance of gnode_dmp_batch.h, which states the kernels of both forms, the workspace, the
// preamble and the launches of the marginals and of their reverse sweep once: the five entries below (gnode_dmp_f32 and
// gnode_dmp_init_f32 are B = 1 of the forward, gnode_dmp_backward_f32 of the reverse), the sizes that choose the form for every
// rates policy, and gnode_dmp_f32's seed kernel.  The recurrence is gnode_dmp.h's.
#include "gnode_dmp_batch.h"

using DmpConstant = DmpBatchConstantRates;

extern "C" size_t gnode_dmp_batch_lds_bytes(gnode_graph_t g) {
    if (!g) return 0;
    return 5 * dmp_align16((size_t)g->nnz * 4) + 3 * dmp_align16((size_t)g->info.n * 4);      // theta x2, phi, ps, rev | P, Pi, Pr
}
extern "C" size_t gnode_dmp_batch_backward_lds_bytes(gnode_graph_t g) {
    if (!g) return 0;                   // theta_bar x2, phi_bar, q_bar, q_tot, gamma_part, rev | pi_bar, pr_bar
    return 7 * dmp_align16((size_t)g->nnz * 4) + 2 * dmp_align16((size_t)g->info.n * 4);
}

// gnode_dmp_f32's start: the state of a 0/1 seed vector is (1 - seed, seed, 0) (dmp.py's _set_seeds), exact in fp32.  It IS
// output row 0, and the run reads it back from there as its `init`.
__global__ __launch_bounds__(256) void k_dmp_seed_out0(const float* __restrict__ seed, int n, float* __restrict__ out0) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < n) dmp_store3(out0, k, 1.0f - seed[k], seed[k], 0.0f);
}

int gn_dmp_set_attributes() {
    if (int e = dmp_batch_set_attributes<DmpConstant>()) return e;
    return dmp_grad_set_attributes<DmpConstant>();
}

// A solo call is always the general form (dmp_run), and both solo entries ask for the seed vector's room: 6 eb + 4 nb + 256.  The
// forward's workspace does not depend on the horizon under constant rates: kDmpAnyHorizon where dmp_carve asks for one.
extern "C" size_t gnode_dmp_workspace_bytes(gnode_graph_t g) { return g ? dmp_carve<DmpConstant>(g, 1, kDmpAnyHorizon, true, true, nullptr).bytes : 0; }
extern "C" size_t gnode_dmp_init_workspace_bytes(gnode_graph_t g) { return gnode_dmp_workspace_bytes(g); }   // (the seed vector rests)
extern "C" size_t gnode_dmp_batch_workspace_bytes(gnode_graph_t g, int32_t B) {
    return g && B >= 1 ? dmp_carve<DmpConstant>(g, (size_t)B, kDmpAnyHorizon, !dmp_batch_one_workgroup(g), false, nullptr).bytes : 0;
}
extern "C" size_t gnode_dmp_batch_backward_workspace_bytes(gnode_graph_t g, int32_t B, int32_t maxTime) {
    return g && B >= 1 && maxTime >= 2 ? dmp_grad_carve<DmpConstant>(g, (size_t)B, (size_t)maxTime, !dmp_grad_one_workgroup(g), nullptr).bytes : 0;
}
extern "C" size_t gnode_dmp_backward_workspace_bytes(gnode_graph_t g, int32_t maxTime) {      // a solo call is the general form
    return g && maxTime >= 2 ? dmp_grad_carve<DmpConstant>(g, 1, (size_t)maxTime, true, nullptr).bytes : 0;
}

extern "C" int gnode_dmp_f32(gnode_graph_t g, const float* weights, const float* gamma, const int32_t* seeds_host,
                             int32_t n_seeds, int32_t maxTime, float* out, void* workspace, size_t workspace_bytes,
                             void* stream) {
    return dmp_run<DmpConstant>("gnode_dmp_f32", g, weights, 0, gamma, 0, nullptr, seeds_host, n_seeds, 1, maxTime, out, true, workspace,
                                workspace_bytes, stream);
}

extern "C" int gnode_dmp_init_f32(gnode_graph_t g, const float* weights, const float* gamma, const float* init, int32_t maxTime,
                                  float* out, void* workspace, size_t workspace_bytes, void* stream) {
    GN_CHECK_ARG(init, "gnode_dmp_init_f32: null pointer");
    return dmp_run<DmpConstant>("gnode_dmp_init_f32", g, weights, 0, gamma, 0, init, nullptr, 0, 1, maxTime, out, true, workspace,
                                workspace_bytes, stream);
}

extern "C" int gnode_dmp_batch_f32(gnode_graph_t g, const float* weights, int64_t w_stride, const float* gamma, int64_t gamma_stride,
                                   const float* init, int32_t B, int32_t maxTime, float* out, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    GN_CHECK_ARG(init, "gnode_dmp_batch_f32: null pointer");
    return dmp_run<DmpConstant>("gnode_dmp_batch_f32", g, weights, (long)w_stride, gamma, (long)gamma_stride, init, nullptr, 0, B, maxTime, out,
                                false, workspace, workspace_bytes, stream);
}

extern "C" int gnode_dmp_batch_backward_f32(gnode_graph_t g, const float* weights, int64_t w_stride, const float* gamma, int64_t gamma_stride,
                                            const float* init, int32_t B, int32_t maxTime, const float* out, const float* grad_out,
                                            float* grad_w, float* grad_gamma, float* grad_init, void* workspace, size_t workspace_bytes,
                                            void* stream) {
    return dmp_grad_run<DmpConstant>("gnode_dmp_batch_backward_f32", g, weights, (long)w_stride, gamma, (long)gamma_stride, init, B, maxTime, out,
                                     grad_out, grad_w, grad_gamma, grad_init, false, workspace, workspace_bytes, stream);
}

extern "C" int gnode_dmp_backward_f32(gnode_graph_t g, const float* weights, const float* gamma, const float* init, int32_t maxTime,
                                      const float* out, const float* grad_out, float* grad_w, float* grad_gamma, float* grad_init,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    return dmp_grad_run<DmpConstant>("gnode_dmp_backward_f32", g, weights, 0, gamma, 0, init, 1, maxTime, out, grad_out, grad_w, grad_gamma,
                                     grad_init, true, workspace, workspace_bytes, stream);
}
