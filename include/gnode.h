/*
 * gnode.h -- C ABI of libgnode_hip.so: the MI355X (gfx950) GN-ODE integration path.
 *
 * The reference (sissykosm/GN-ODE-SIR) is pure Python and has no FFI of its own;
 * each entry point below names the reference interface it replaces (file:line
 * into the reference tree).  INTEGRATION.md shows the ctypes stubs a maintainer
 * of the reference would add to bind them.
 *
 * Conventions
 *   - every function returns 0 on success, a negative gnode_status otherwise;
 *     gnode_last_error() returns a thread-local message for the last failure.
 *   - "device" pointers are caller-owned HBM allocations (the Python host hands
 *     over torch tensors' data_ptr()); the library never frees or retains them
 *     past the call.  "host" pointers are ordinary memory, read before return.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *     All work is enqueued on it.  gnode_rhs_f32, gnode_forward_f32,
 *     gnode_backward_f32, gnode_rhs_vjp_f32, gnode_backward_rk4_f32, their _dx forms, gnode_backward_discrete_f32, gnode_backward_discrete_keep_f32 and gnode_l1_loss_f32 allocate nothing, synchronise nothing and keep nothing in
 *     the graph handle: every byte of scratch (including the partial sums of long
 *     "hub" rows) is carved from the caller's workspace, so they can be captured
 *     into a hipGraph on first use and one handle may serve several streams (each
 *     with its own workspace).  Functions that DO synchronise `stream` say so below
 *     (gnode_graph_create, gnode_sir_mc_philox with more than 32 seeds,
 *     gnode_sir_mc_philox_nodes, gnode_sir_mc_philox_edges, gnode_sir_mc_philox_traj_edges, gnode_sir_mc_philox_traj with more than 32 seeds or rate arrays, gnode_sir_mc_philox_init, gnode_sir_mc_coins, gnode_dmp_f32, gnode_dmp_init_f32, gnode_dmp_batch_f32, gnode_dmp_batch_backward_f32, gnode_dmp_backward_f32, gnode_dmp_source_scores_f32, gnode_dmp_source_batch_scores_f32, gnode_dmp_source_events_scores_f32, gnode_dmp_source_events_scores_schedule_f32, gnode_dmp_outbreak_sizes_schedule_f32, gnode_meanfield_f64, gnode_meanfield_init_f64, gnode_meanfield_rates_f64, gnode_meanfield_rates_steps_f64).
 *   - process-wide state: (1) a per-device "set up once" table (compute-unit count,
 *     dynamic-LDS kernel attributes), written under a lock by the first
 *     gnode_graph_create on a device and read-only afterwards; (2) the opt-in
 *     launch profiler of gnode_profile_enable (off by default; while it is on, use
 *     the library from one thread); (3) the thread-local error string.  Nothing
 *     else: no environment variable is read, no kernel variant is selected at
 *     run time other than by the arguments.
 *   - all floating point is IEEE fp32 (the reference builds its model under
 *     torch.float32, ode_nn_ngraph_sim.py:433); indices are int32.
 *   - row layout is the reference's own: a batch of B samples on one graph of n
 *     nodes is `rows = B*n` rows, row r = b*n + node (ode_nn_ngraph_sim.py:149),
 *     the adjacency is applied block-diagonally (:68-69) WITHOUT ever building
 *     the block-diagonal index.  A multi-graph batch (ode_nn_ngraphs.py:179-196)
 *     is one graph handle holding the concatenated CSR and B = 1.
 */
#ifndef GNODE_H
#define GNODE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    GNODE_OK = 0,
    GNODE_ERR_ARG = -1,      /* bad argument (null pointer, shape mismatch, unsupported H) */
    GNODE_ERR_HIP = -2,      /* a HIP runtime call failed */
    GNODE_ERR_WORKSPACE = -3 /* caller workspace too small */
} gnode_status;

typedef struct gnode_graph_s* gnode_graph_t;

/* Parameters of ODEBlock + ODEfunc, device pointers, names = reference state_dict
 * keys (ode_nn_ngraph_sim.py:48,123,126,131). */
typedef struct {
    const float* odefunc_linear_weight; /* [H,H] row-major (out,in) */
    const float* odefunc_linear_bias;   /* [H]   */
    const float* linearS1_weight;       /* [H,1] */
    const float* linearS1_bias;         /* [H]   */
    const float* linear3_weight;        /* [4,H] */
    const float* linear3_bias;          /* [4]   */
    const float* linearS2_weight;       /* [1,4] */
    const float* linearS2_bias;         /* [1]   */
} gnode_params;

const char* gnode_last_error(void);
int gnode_version(void);

/* ---- graph ---------------------------------------------------------------
 * Replaces the per-RHS `scipy.sparse.block_diag` + `torch.LongTensor(idx).to(device)`
 * of ode_nn_ngraph_sim.py:68-71 (ode_nn_ngraphs.py:65-71) and the adjacency
 * built by create_graph, ode_nn.py:413.  rowptr[n+1] / col[nnz] are HOST int32
 * CSR arrays (symmetric, sorted columns, values ignored); the handle owns its
 * device copy.  Synchronous (copies before returning). */
int gnode_graph_create(const int32_t* rowptr_host, const int32_t* col_host, int32_t n, int64_t nnz,
                       gnode_graph_t* out);
int gnode_graph_destroy(gnode_graph_t g);
int gnode_graph_info(gnode_graph_t g, int32_t* n, int64_t* nnz, int32_t* max_degree);

/* ---- RHS -----------------------------------------------------------------
 * ODEfunc.forward(t, x): ode_nn_ngraph_sim.py:58-96 (multi: ode_nn_ngraphs.py:54-83).
 * x, dx: device [4*rows, H], slabs S | I | R | beta-gamma (col 0 beta, col 1 gamma).
 * 4 <= H <= 128, H % 4 == 0 (else GNODE_ERR_ARG, and the workspace size is 0).
 * workspace: device, >= gnode_rhs_workspace_bytes(g, rows, H) (the size depends on the
 * graph: long rows are summed through scratch carved from the workspace). */
size_t gnode_rhs_workspace_bytes(gnode_graph_t g, int64_t rows, int32_t H);
int gnode_rhs_f32(gnode_graph_t g, const float* x, const float* W, const float* b, float* dx,
                  int64_t rows, int32_t H, void* workspace, size_t workspace_bytes, void* stream);

/* ---- forward -------------------------------------------------------------
 * ODEBlock.forward(x): ode_nn_ngraph_sim.py:148-188 (multi: ode_nn_ngraphs.py:124-152)
 * = encoder + odeint(method='euler' | 'rk4') over the grid + read-out + softmax,
 * optionally fused with get_sir_t_nodes_torch (ode_nn.py:249-261).
 *   x          device [rows, 3+H]; 4 <= H <= 128, H % 4 == 0 (else GNODE_ERR_ARG, and the
 *              workspace size is 0)
 *   dt_host    host  [n_steps] fp32 step sizes t[k+1]-t[k] (grid has n_steps+1 points)
 *   method     0 = euler, 1 = rk4 (torchdiffeq's 3/8 rule)
 *   out_rows_host  host [n_out] ascending grid indices to emit, or NULL = all
 *                  n_steps+1 points (n_out ignored)
 *   S, I, R    device [n_out, rows] each (the reference's [G, rows, 1])
 *   sol        NULL, or device [n_steps+1, 4*rows, H]: the trajectory odeint
 *              returns (needed by the adjoint backward, never by inference).
 *              Slabs S, I, R of every grid point are odeint's.  The 4th slab
 *              (beta, gamma; derivative 0, so odeint repeats sol[0]'s at every grid
 *              point) is odeint's at grid point 0 everywhere; at H = 64 (every form but the
 *              one-workgroup-per-sample launch, gnode_forward_path() == 1) grid points
 *              1 .. n_steps-1 carry A*Z_I(y_k) there instead -- the neighbour sums
 *              the adjoint backward would otherwise gather a second time -- when no
 *              `keep` buffer is given, and are left UNWRITTEN when one is (the sums then
 *              live in `keep`, in the form the backward uses); the last grid point's is
 *              always left unwritten; other H repeat beta, gamma.
 *   keep       NULL, or device buffer of keep_bytes >= gnode_forward_keep_bytes(...):
 *              the KEPT ACTIVATIONS sigmoid(W y_k + b) of the S and I compartments at
 *              every grid point, which the fused H = 64 path has in registers anyway
 *              and gnode_backward_f32 then reads back instead of recomputing (three
 *              of its seven 64x64 products per row and every sigmoid), plus, on the
 *              tiled path, the neighbour sums A*Z_I(y_k) already multiplied by the
 *              sigmoid's derivative.  Opaque layout; ignored when sol is NULL or
 *              gnode_forward_keep_bytes() is 0.  Outputs and the S, I, R slabs of sol
 *              do not depend on whether keep is given.  A trajectory and the keep buffer
 *              of the same call belong together: hand gnode_backward_f32 both, or a
 *              trajectory that was produced WITHOUT keep and NULL.
 *   workspace  device, >= gnode_forward_workspace_bytes(g, rows, H, method)
 *   flags      0, or GNODE_FWD_PER_STEP: never take the persistent one-launch path (below)
 *   sol_info_host  NULL, or host int32 that receives what this call leaves in `sol` / `keep`
 *              (GNODE_SOL_AI: the 4th slabs of sol[1 .. n_steps-1] carry A*Z_I; GNODE_SOL_KEEP: the
 *              keep buffer was filled and those slabs are unwritten; 0: neither): hand it to
 *              gnode_backward_f32, which then refuses a trajectory / keep pair that does not
 *              belong together instead of reading unwritten memory.
 * Mid-size graphs at H = 64 (a few hundred to ~16k rows per launch, no rows longer than the hub
 * threshold, <= 128 steps): the whole integration runs as ONE persistent launch in which every
 * workgroup keeps its rows in registers across all steps and the workgroups of a sample meet at an
 * in-launch barrier once per step.  Its spins are bounded: gnode_forward_status() reports a
 * workgroup that gave up (never observed; it exists so that a hang becomes an error).  Same
 * outputs, bit for bit, as the one-launch-per-step form. */
#define GNODE_FWD_PER_STEP 1
#define GNODE_SOL_AI 1
#define GNODE_SOL_KEEP 2
#define GNODE_SOL_TINY 4   /* produced by the one-workgroup-per-sample forward: no A*Z_I anywhere, keep holds the sigmoids only */
size_t gnode_forward_workspace_bytes(gnode_graph_t g, int64_t rows, int32_t H, int32_t method);
/* Which form gnode_forward_f32 runs for this shape: 0 = one launch per step, 1 = the one-workgroup-per-sample launch (tiny
 * graphs in batches too large for one resident grid), 2 = the persistent launch (H = 64: tiny and mid-size graphs) (then plan_host, if given, receives {16-row tiles per
 * workgroup, workgroups per sample, XCDs per sample, samples side by side per XCD, samples alive at once}), 3 = the persistent
 * launch of the small hidden sizes (H = 8, 16, 32; batches that fit one resident grid); -1 = bad arguments.  n_out: emitted grid points; with_sol: a trajectory is requested (training). */
int gnode_forward_path(gnode_graph_t g, int64_t rows, int32_t H, int32_t method, int32_t n_steps, int32_t n_out,
                       int32_t with_sol, int32_t flags, int32_t* plan_host);
/* Synchronises `stream` and writes 0 to *code_host, or the give-up code of the last gnode_forward_f32 call that ran the
 * persistent path on this workspace (then its outputs are invalid).  Meaningful only after a call for which
 * gnode_forward_path() says 2 or 3 (the other forms never touch the control block).  Not capturable. */
int gnode_forward_status(int64_t rows, int32_t H, int32_t method, const void* workspace, void* stream, int32_t* code_host);
/* The same for the last gnode_backward_f32 call on this workspace: the give-up code of its persistent adjoint sweep, 0 when
 * all went well or the call ran no persistent launch (every call leaves the word defined).  Not capturable. */
int gnode_backward_status(int64_t rows, int32_t H, const void* workspace, void* stream, int32_t* code_host);
/* 1 when gnode_forward_f32 (method 0, no `keep` buffer) on this graph stores A*Z_I(y_k) in the 4th slab of sol[k],
 * 1 <= k <= n_steps-1 (see `sol` below), 0 when the 4th slab repeats beta, gamma at every grid point.  n_out: number
 * of emitted grid points (n_steps+1 when out_rows_host is NULL). */
int gnode_sol_carries_neighbour_sums(gnode_graph_t g, int64_t rows, int32_t H, int32_t n_steps, int32_t n_out, int32_t flags);
/* Size of the optional `keep` buffer of gnode_forward_f32 / gnode_backward_f32 (method 0), or 0 when this H keeps
 * nothing (then pass NULL).  3 * (n_steps + 1) * (rows + 1) * H floats at H = 64 (the tiled and the one-launch form). */
size_t gnode_forward_keep_bytes(gnode_graph_t g, int64_t rows, int32_t H, int32_t n_steps, int32_t n_out);
int gnode_forward_f32(gnode_graph_t g, const float* x, const gnode_params* p, const float* dt_host,
                      int32_t n_steps, int32_t method, const int32_t* out_rows_host, int32_t n_out,
                      float* S, float* I, float* R, float* sol, float* keep, size_t keep_bytes,
                      int64_t rows, int32_t H, void* workspace, size_t workspace_bytes, void* stream,
                      int32_t flags, int32_t* sol_info_host);

/* ---- backward -------------------------------------------------------------
 * The gradient the reference trains with: torchdiffeq's odeint_adjoint under
 * method='euler' (imported at ode_nn_ngraph_sim.py:16, called at :168; semantics in
 * SURVEY Appendix A) followed by autograd through the head and the encoder.
 *   sol          device [n_steps+1, 4*rows, H] saved by gnode_forward_f32 on THIS graph with the
 *                same n_steps / out_rows (its 4th slabs are read as described there)
 *   keep         the buffer the SAME gnode_forward_f32 call filled (then every interval
 *                but the last reads the kept activations; gradients agree with the
 *                recomputing path to fp32 rounding of the summation order), or NULL for a
 *                trajectory that was produced without one
 *   flags        0, or GNODE_FWD_PER_STEP: one launch per interval even where the persistent sweep applies (mid-size
 *                graphs at H = 64 with a keep buffer: intervals n_steps-1 .. 1 run as ONE launch, see the forward)
 *   sol_info     what gnode_forward_f32 reported through sol_info_host for that call (checked against
 *                `keep`: GNODE_ERR_ARG on a mismatch), or -1 = unchecked (the caller vouches for the pairing)
 *   gS, gI, gR   device [n_out, rows] upstream gradients of the outputs
 *   grads        device pointers (same struct as the parameters) that RECEIVE
 *                dL/dparam (overwritten, not accumulated)
 * Euler only (the reference's method).  Deterministic (no float atomics).
 *   workspace  device, >= gnode_backward_workspace_bytes(g, rows, H) */
size_t gnode_backward_workspace_bytes(gnode_graph_t g, int64_t rows, int32_t H);
int gnode_backward_f32(gnode_graph_t g, const float* x, const gnode_params* p, const float* dt_host,
                       int32_t n_steps, const int32_t* out_rows_host, int32_t n_out, const float* sol,
                       const float* keep, size_t keep_bytes,
                       const float* gS, const float* gI, const float* gR, const gnode_params* grads,
                       int64_t rows, int32_t H, void* workspace, size_t workspace_bytes, void* stream,
                       int32_t flags, int32_t sol_info);

/* ---- RHS value and vector-Jacobian product -----------------------------------
 * What torch autograd takes through ODEfunc.forward (ode_nn_ngraph_sim.py:58-96, multi: ode_nn_ngraphs.py:54-83) when
 * torchdiffeq's adjoint calls torch.autograd.grad(func(t, y), (y, *params), v): for a cotangent v of the RHS output
 *   y, v       device [4*rows, H], slabs S | I | R | beta-gamma (v's 4th slab is not read: that output is 0, :96)
 *   f_out      NULL, or device [4*rows, H]: f(y), bit-identical to gnode_rhs_f32 on the same input
 *   gy_out     NULL, or device [4*rows, H]: v^T df/dy (R slab 0: Z_R is dead in the reference, :62-66; beta-gamma slab:
 *              column 0 d/dbeta, column 1 d/dgamma, the other columns 0)
 *   gW_out     NULL, or device [H,H]: v^T df/dW     gb_out: NULL, or device [H]: v^T df/db   (overwritten)
 * Each NULL output skips its work.  4 <= H <= 128, H % 4 == 0.  Deterministic (fixed-order reduction, no float atomics);
 * allocates nothing and synchronises nothing (capturable).
 *   workspace  device, >= gnode_rhs_vjp_workspace_bytes(g, rows, H) */
size_t gnode_rhs_vjp_workspace_bytes(gnode_graph_t g, int64_t rows, int32_t H);
int gnode_rhs_vjp_f32(gnode_graph_t g, const float* y, const float* W, const float* b, const float* v, float* f_out,
                      float* gy_out, float* gW_out, float* gb_out, int64_t rows, int32_t H, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---- RK4 backward ------------------------------------------------------------
 * The gradient of ODEBlock(method='rk4'): torchdiffeq 0.2.2's odeint_adjoint(..., method='rk4') (the 3/8 rule on the fixed
 * grid; the reference's call site is ode_nn_ngraph_sim.py:168, which hard-codes 'euler') followed by autograd through the
 * head and the encoder; the rule is restated in DESIGN.md section 7.  Arguments as gnode_backward_f32 without keep / flags /
 * sol_info: `sol` is the trajectory of a gnode_forward_f32 call with method = 1 on THIS graph, same n_steps / out_rows;
 * only its S, I, R slabs and grid point 0's 4th slab are read.  grads receive dL/dparam (overwritten).  Deterministic.
 * Enqueue-only, one launch sequence per interval.
 *   workspace  device, >= gnode_backward_rk4_workspace_bytes(g, rows, H) */
size_t gnode_backward_rk4_workspace_bytes(gnode_graph_t g, int64_t rows, int32_t H);
int gnode_backward_rk4_f32(gnode_graph_t g, const float* x, const gnode_params* p, const float* dt_host,
                           int32_t n_steps, const int32_t* out_rows_host, int32_t n_out, const float* sol,
                           const float* gS, const float* gI, const float* gR, const gnode_params* grads,
                           int64_t rows, int32_t H, void* workspace, size_t workspace_bytes, void* stream);

/* ---- input gradient: backpropagation to the ODEBlock input x ---------------
 * gnode_backward_f32 / gnode_backward_rk4_f32 with one more output: what odeint_adjoint returns for the initial state
 * (ode_nn_ngraph_sim.py:148-168, multi: ode_nn_ngraphs.py:124-137) taken back through the encoder, i.e. dL/dx.
 *   gx     NULL (then exactly the call without _dx), or device [rows, 3+H] fp32 in the layout of x, OVERWRITTEN:
 *            columns 0, 1, 2  dL/dS0, dL/dI0, dL/dR0 = sum_h a_X(t0)[r,h] [sol0_X[r,h] > 0] linearS1.weight[h]
 *                             (a(t0) includes the head's VJP at grid point 0 when that point is emitted)
 *            column 3, 4      dL/dbeta, dL/dgamma: the beta-gamma slab's adjoint, over intervals i = G-1 .. 1 with the
 *                             adjoint a_i before its update and the Jacobian at y_i, AI = A Z_I(y_i):
 *                               beta  += dt_{i-1} sum_h (a_I - a_S) AI Z_S      gamma += dt_{i-1} sum_h (a_R - a_I) Z_I
 *                             (RK4: the same two sums per stage at the stage state, weighted dt {1, 3, 3, 1} / 8)
 *            columns 5 ..     0 (the slab's other columns, the multi-graph marker among them, feed nothing)
 *   grads  as there, or NULL when gx is given: the parameter reduction is then skipped.  NULL grads and NULL gx: GNODE_ERR_ARG.
 *   keep   (Euler) must be NULL when gx is given (GNODE_ERR_ARG otherwise): the kept activations hold AI Z_S (1 - Z_S), not
 *          AI, so a gx call needs a trajectory produced WITHOUT keep.
 * A gx call runs the recomputing one-launch-per-interval forms (H = 64: the fused interval kernel over one table when sol
 * carries A Z_I, two otherwise; H <= 32: the small-H interval kernel; other H: the five-launch path), never the one-launch
 * sweeps of tiny graphs / small H nor the kept or persistent H = 64 sweeps, whatever `flags` says: slower than the
 * training backward on the shapes that take those.  Parameter gradients are bitwise those of the
 * call without gx on the same path.  Same workspace as without gx; deterministic (the beta / gamma columns are
 * read-modify-written by one lane per row per launch, launches stream-ordered; no atomics); enqueue-only (capturable). */
int gnode_backward_dx_f32(gnode_graph_t g, const float* x, const gnode_params* p, const float* dt_host,
                          int32_t n_steps, const int32_t* out_rows_host, int32_t n_out, const float* sol,
                          const float* keep, size_t keep_bytes,
                          const float* gS, const float* gI, const float* gR, const gnode_params* grads,
                          int64_t rows, int32_t H, void* workspace, size_t workspace_bytes, void* stream,
                          int32_t flags, int32_t sol_info, float* gx);
int gnode_backward_rk4_dx_f32(gnode_graph_t g, const float* x, const gnode_params* p, const float* dt_host,
                              int32_t n_steps, const int32_t* out_rows_host, int32_t n_out, const float* sol,
                              const float* gS, const float* gI, const float* gR, const gnode_params* grads,
                              int64_t rows, int32_t H, void* workspace, size_t workspace_bytes, void* stream, float* gx);

/* ---- exact gradient of the Euler solve (backpropagation through the solver) -----------
 * What torch autograd returns through a plain Euler loop y_i = y_{i-1} + dt_{i-1} f(y_{i-1}) (torchdiffeq's odeint instead
 * of odeint_adjoint at ode_nn_ngraph_sim.py:168): the adjoint sweep of gnode_backward_f32 with every interval's Jacobian
 * and parameter VJP evaluated at its LEFT endpoint y_{i-1}, where the forward took its slope, instead of at y_i.  With
 * a = dL/dsol[G-1], for i = G-1 .. 1:
 *     gtheta += dt_{i-1} (df/dtheta (y_{i-1}))^T a        a += dt_{i-1} (df/dy (y_{i-1}))^T a + dL/dsol[i-1]
 * then the encoder on a.  DESIGN.md section 7.3 has the rule, the launch structure and how far the adjoint is from it.
 *   sol        device [n_steps+1, 4*rows, H]: the trajectory of a gnode_forward_f32 call with method = 0 on THIS graph, same
 *              n_steps / out_rows, produced WITHOUT a keep buffer
 *   sol_info   what that forward reported through sol_info_host (A*Z_I(y_k) is then read back from the 4th slabs that
 *              carry it), or -1 = unchecked (A*Z_I is gathered at every interval).  A keep-produced trajectory
 *              (GNODE_SOL_KEEP): GNODE_ERR_ARG.
 *   grads, gx  as gnode_backward_dx_f32 (gx columns 3, 4 sum the same terms at y_{i-1}); either may be NULL, not both.
 * Other arguments as gnode_backward_f32.  ALWAYS runs the recomputing one-launch-per-interval forms (H = 64: the fused interval
 * kernel; H <= 32: the small-H interval kernel; other H: five launches per interval), never the kept, persistent or
 * one-launch sweeps.  Deterministic (fixed-order reduction, no float atomics); enqueue-only (capturable).
 *   workspace  device, >= gnode_backward_discrete_workspace_bytes(g, rows, H) */
size_t gnode_backward_discrete_workspace_bytes(gnode_graph_t g, int64_t rows, int32_t H);
int gnode_backward_discrete_f32(gnode_graph_t g, const float* x, const gnode_params* p, const float* dt_host,
                                int32_t n_steps, const int32_t* out_rows_host, int32_t n_out,
                                const float* sol, int32_t sol_info,
                                const float* gS, const float* gI, const float* gR,
                                const gnode_params* grads, float* gx,
                                int64_t rows, int32_t H, void* workspace, size_t workspace_bytes, void* stream);

/* The same gradient on the forms of the training backward (ABI 225): the arguments of gnode_backward_dx_f32.
 *   keep, keep_bytes  the kept activations of the forward that produced `sol` (H = 64), or NULL.  With a checked sol_info the
 *              pairing rule of gnode_backward_f32 holds: keep with a trajectory lacking GNODE_SOL_KEEP, or a keep-produced
 *              trajectory without its buffer, is GNODE_ERR_ARG; keep together with gx is GNODE_ERR_ARG; a keep buffer smaller
 *              than gnode_forward_keep_bytes is GNODE_ERR_WORKSPACE.
 *   flags      as gnode_backward_f32 (GNODE_FWD_PER_STEP: no persistent launch)
 * Interval i reads grid point i-1, all of which the forward kept for i = G-1 .. 2: P_S(y_{i-1}), Z_I(y_{i-1}), and
 * Z_S(y_{i-2}) for the next q row; the head's VJP at grid point i-1 reuses the rows staged for gW.  Forms
 * (gnode_backward_discrete_path):
 *   0  recomputing, one launch per interval: what gnode_backward_discrete_f32 runs.  Any gx call, H = 64 without keep, graphs
 *      of the one-workgroup sweep's size (n <= 64: karate) or behind a one-workgroup forward (GNODE_SOL_TINY), 2-point grids, H > 32 other than 64, batches beyond one resident grid at H <= 32
 *   1  H = 64 with keep: intervals G-1 .. 2 one launch each over the kept activations, interval 1 (P_S(y_0) is not kept) on
 *      the two-table recomputing launch, which gathers A Z_I(y_0) from the kept Z_I table
 *   2  H = 64 with keep, mid-size graphs: intervals G-1 .. 2 in ONE persistent launch (up to two per batch), then interval 1
 *   3  H = 8, 16, 32: the whole sweep in one persistent launch
 * Forms 2 and 3 write the give-up word gnode_backward_status reads.  Gradients agree with form 0 to rounding (rows enter
 * the parameter sums in another order).  Deterministic (fixed-slot reduction, no float atomics, bitwise repeatable); allocates
 * nothing, synchronises nothing, reads no environment variable; enqueue-only (capturable).
 *   workspace  device, >= gnode_backward_discrete_workspace_bytes(g, rows, H) */
int gnode_backward_discrete_keep_f32(gnode_graph_t g, const float* x, const gnode_params* p, const float* dt_host,
                                     int32_t n_steps, const int32_t* out_rows_host, int32_t n_out, const float* sol,
                                     const float* keep, size_t keep_bytes,
                                     const float* gS, const float* gI, const float* gR, const gnode_params* grads,
                                     int64_t rows, int32_t H, void* workspace, size_t workspace_bytes, void* stream,
                                     int32_t flags, int32_t sol_info, float* gx);
/* Which form (0 .. 3 above) a gnode_backward_discrete_keep_f32 call with these arguments takes; -1 on a bad argument.
 * with_keep / with_gx: whether the call passes keep / gx.  Host only, touches no device memory. */
int gnode_backward_discrete_path(gnode_graph_t g, int64_t rows, int32_t H, int32_t n_steps, const int32_t* out_rows_host,
                                 int32_t n_out, int32_t with_keep, int32_t flags, int32_t sol_info, int32_t with_gx);

/* ---- Monte-Carlo SIR labels ------------------------------------------------
 * sir_torch(G, seed_set, beta, gamma, sims, T): ode_nn.py:30-88.
 *
 * gnode_sir_mc_philox: production mode.  One workgroup per trajectory walking the
 * out-edges of its current frontier (work per step = the frontier's out-degree, not
 * nnz); coins are counter-based Philox4x32-10: the coin of CSR position / node id p is
 * word (p & 3) of the block keyed (p >> 2, step, sim, kind) -- four consecutive items
 * share one block, which a lane computes once -- so that neither the visiting order nor any sharding of
 * [sim_offset, sim_offset+sims) over GPUs can change a count.  counts: device uint32 [3, T, n] (S, I, R), ACCUMULATED into (caller
 * zeroes it); rows t >= 1 add one per trajectory per node, row 0 of S and I is
 * written with the initial state once (reference quirk: assigned, ode_nn.py:55-56).
 * Up to 32 seeds travel as a kernel argument (nothing is synchronised); with more,
 * seeds_host is copied and `stream` is synchronised before the function returns.
 *
 * gnode_sir_mc_coins: parity mode.  Consumes a recorded coin stream exactly as
 * the reference consumes torch.rand (ode_nn.py:65,70): per step first one coin
 * per (infected src -> susceptible dst) row of the directed edge table in table
 * order, then one per infected node in ascending id.  table_src/table_dst:
 * device int32 [n_table] (ode_nn.py:32-38 order).  coins: device fp64.
 * Sequential over sims (one workgroup), writes counts as above and the number
 * of coins consumed to *coins_used_host after synchronising `stream`. */
size_t gnode_sir_workspace_bytes(gnode_graph_t g, int32_t T);   /* for gnode_sir_mc_philox */
size_t gnode_sir_coins_workspace_bytes(void);                    /* for gnode_sir_mc_coins  */
int gnode_sir_mc_philox(gnode_graph_t g, const int32_t* seeds_host, int32_t n_seeds, double beta, double gamma,
                        int64_t sims, int64_t sim_offset, int32_t T, uint64_t rng_seed, uint32_t* counts,
                        void* workspace, size_t workspace_bytes, void* stream);
/* The same model, same coins, same counts by the edge-parallel statement: every workgroup tests EVERY directed edge
 * against the infected set each step (what the reference's `isin` scan does, ode_nn.py:61), O(nnz) per trajectory-step
 * whatever the frontier.  gnode_sir_mc_philox walks the frontier's rows instead and falls back to this scan only for
 * graphs whose frontier lists do not fit the LDS; exported as the cross-check of that kernel and as its measured
 * baseline. */
int gnode_sir_mc_philox_scan(gnode_graph_t g, const int32_t* seeds_host, int32_t n_seeds, double beta, double gamma,
                             int64_t sims, int64_t sim_offset, int32_t T, uint64_t rng_seed, uint32_t* counts,
                             void* workspace, size_t workspace_bytes, void* stream);
/* gnode_sir_mc_philox through the kernel's PROFILING instantiation (a template flag, not a different algorithm): the same
 * counts, plus what the launch did -- stats_host[0] Philox blocks computed, [1] infection coins drawn, [2] recovery coins
 * drawn, [3] CSR entries read (bench.py prices the kernel against the chip's integer rate with them).  Synchronises `stream`. */
int gnode_sir_mc_philox_counted(gnode_graph_t g, const int32_t* seeds_host, int32_t n_seeds, double beta, double gamma,
                                int64_t sims, int64_t sim_offset, int32_t T, uint64_t rng_seed, uint32_t* counts,
                                void* workspace, size_t workspace_bytes, void* stream, uint64_t* stats_host);
/* Per-node rates (ABI 226): the same model, coins and counts with a rate per node instead of one for the graph.
 *   beta_host   host fp64 [n]   a directed CSR entry (u -> v), u infected and v susceptible in the pre-step state, fires iff
 *                               coin(entry) < thr(beta_host[v]): indexed by the TARGET, the GN-ODE's convention for x[:, 3]
 *                               (row v's dS_v = -beta_v (A Z_I)_v Z_S,v)
 *   gamma_host  host fp64 [n]   the infected node u recovers iff coin(u) < thr(gamma_host[u])
 * thr(p) = floor(p * 2^32) in [0, 2^32], compared in 64 bits: p = 0 never fires, p = 1 always does.  Arrays that hold one
 * constant each give gnode_sir_mc_philox's counts exactly.  Every entry is validated on the host (a NaN or a value
 * outside [0, 1]: GNODE_ERR_ARG, the message names the index); the thresholds are staged through the workspace, whose
 * layout is gnode_sir_mc_philox's followed by them.  Synchronises `stream`.  edge_scan != 0 runs the edge-parallel
 * statement where the frontier walk would apply (what gnode_sir_mc_philox_scan is to gnode_sir_mc_philox). */
size_t gnode_sir_nodes_workspace_bytes(gnode_graph_t g, int32_t T);
int gnode_sir_mc_philox_nodes(gnode_graph_t g, const int32_t* seeds_host, int32_t n_seeds,
                              const double* beta_host, const double* gamma_host,   /* host fp64 [n] each */
                              int64_t sims, int64_t sim_offset, int32_t T, uint64_t rng_seed, uint32_t* counts,
                              void* workspace, size_t workspace_bytes, void* stream, int32_t edge_scan);
/* Per-trajectory output: what the counts have averaged away.  The call is gnode_sir_mc_philox (both rate arrays NULL: the
 * scalars beta / gamma hold) or gnode_sir_mc_philox_nodes (both given; exactly one is GNODE_ERR_ARG) -- same validation, path
 * selection, launch geometry and coins -- through the kernels' TRAJ instances, which also keep
 *   events  device int16 [2, sims, n], OVERWRITTEN   [0, s, v] the step at which node v of the call's s-th trajectory became
 *                                                    infected (0 for a seed), [1, s, v] the step at which it recovered; -1 =
 *                                                    never within T.  s counts inside the call (the trajectory's coins are
 *                                                    those of sim_offset + s).  Recovery is decided on the pre-step state, so
 *                                                    [1, s, v] > [0, s, v] wherever both are set.  T <= 32767 (GNODE_ERR_ARG).
 *   curves  device uint32 [sims, T, 3], OVERWRITTEN  (S_t, I_t, R_t), the population totals of each trajectory.  Row 0 is the
 *                                                    true initial state (n - k, k, 0), k distinct seeds: the assigned-once
 *                                                    row 0 is a property of the accumulated counts, not of a trajectory.
 *   counts  device uint32 [3, T, n], ACCUMULATED     exactly what gnode_sir_mc_philox / _nodes add, or NULL (nothing is added)
 * events or curves may be NULL, not both (GNODE_ERR_ARG).  sims == 0 is valid and touches neither.  Memory: events take
 * 4 * sims * n bytes -- 283 MB for 10 000 trajectories of a 7 066-node graph -- and curves 12 * sims * T, so callers shard a
 * large run with sim_offset.  The -1 background of events is laid by a fill kernel on `stream` in front of the Monte-Carlo
 * kernel (2 * sims * n elements, no more).  Enqueue-only with up to 32 seeds and scalar rates; otherwise `stream` is
 * synchronised as by the entries above.  The workspace is gnode_sir_nodes_workspace_bytes' in either case. */
size_t gnode_sir_traj_workspace_bytes(gnode_graph_t g, int32_t T);
int gnode_sir_mc_philox_traj(gnode_graph_t g, const int32_t* seeds_host, int32_t n_seeds,
                             double beta, double gamma,                          /* used when both arrays are NULL */
                             const double* beta_host, const double* gamma_host,  /* host fp64 [n] each, or both NULL */
                             int64_t sims, int64_t sim_offset, int32_t T, uint64_t rng_seed,
                             int16_t* events,    /* device [2, sims, n], OVERWRITTEN, or NULL */
                             uint32_t* curves,   /* device [sims, T, 3], OVERWRITTEN, or NULL */
                             uint32_t* counts,   /* device [3, T, n], ACCUMULATED as gnode_sir_mc_philox does, or NULL */
                             void* workspace, size_t workspace_bytes, void* stream, int32_t edge_scan);
/* Per-edge transmission probabilities (no version step: a stale library is known by the missing symbol): the same model,
 * coins and counts with one probability per directed CSR entry.
 *   w_host      host fp64 [nnz], in CSR position order.  The entry at position p, in row u with col[p] = v, u infected and v
 *               susceptible in the pre-step state, fires iff coin(p) < thr(w_host[p]): w_host[p] is the probability that u
 *               infects v -- the SOURCE is the row, the TARGET the column, the convention of gnode_dmp_f32's `weights`, so one
 *               array serves both.  The handle's pattern stays symmetric; a directed contact u -> v is a zero on the reverse
 *               entry (v -> u).  May be NULL when nnz = 0.
 *   gamma       the recovery probability of every node, used when gamma_host is NULL
 *   gamma_host  host fp64 [n] or NULL: the infected node u recovers iff coin(u) < thr(gamma_host[u])
 * thr as above, compared in 64 bits: an array that holds one constant gives gnode_sir_mc_philox's counts exactly, w_host[p] =
 * beta[col[p]] gives gnode_sir_mc_philox_nodes' exactly, 0 never fires, 1 always does.  Every weight and rate is validated on
 * the host (a NaN or a value outside [0, 1]: GNODE_ERR_ARG, the message names the CSR position); the thresholds -- uint64
 * [nnz], then uint64 [n] -- are staged through the workspace behind gnode_sir_mc_philox's layout.  Both calls SYNCHRONISE
 * `stream`, because host arrays are staged.  edge_scan as in gnode_sir_mc_philox_nodes.  gnode_sir_mc_philox_traj_edges takes
 * events / curves / counts under the rules of gnode_sir_mc_philox_traj; both calls use gnode_sir_edges_workspace_bytes. */
size_t gnode_sir_edges_workspace_bytes(gnode_graph_t g, int32_t T);
int gnode_sir_mc_philox_edges(gnode_graph_t g, const int32_t* seeds_host, int32_t n_seeds,
                              const double* w_host,                       /* host fp64 [nnz], CSR position order */
                              double gamma, const double* gamma_host,     /* host fp64 [n], or NULL: then the scalar */
                              int64_t sims, int64_t sim_offset, int32_t T, uint64_t rng_seed, uint32_t* counts,
                              void* workspace, size_t workspace_bytes, void* stream, int32_t edge_scan);
int gnode_sir_mc_philox_traj_edges(gnode_graph_t g, const int32_t* seeds_host, int32_t n_seeds,
                                   const double* w_host, double gamma, const double* gamma_host,
                                   int64_t sims, int64_t sim_offset, int32_t T, uint64_t rng_seed,
                                   int16_t* events,    /* device [2, sims, n], OVERWRITTEN, or NULL */
                                   uint32_t* curves,   /* device [sims, T, 3], OVERWRITTEN, or NULL */
                                   uint32_t* counts,   /* device [3, T, n], ACCUMULATED, or NULL */
                                   void* workspace, size_t workspace_bytes, void* stream, int32_t edge_scan);
/* Initial-state distributions (no version step: a stale library is known by the missing symbol): the same model with every
 * trajectory drawing its own start from one probability triple per node, the GN-ODE's own x[:, 0:3], instead of sharing a
 * seed set.  One entry for the three rate forms and every output.
 *   init_host   host fp64 [n][3] = (pS, pI, pR) per node.  Validated here -- a NaN, an entry outside [0, 1] or a row whose sum
 *               is off 1 by more than 1e-6 is GNODE_ERR_ARG, the message names the node -- and never renormalised.  Node v of
 *               trajectory s starts in S iff c < thr(pS), else in R iff c >= 2^32 - thr(pR), else in I, compared in 64 bits,
 *               thr(p) = floor(p * 2^32), c = word (v & 3) of philox(ctr = (v >> 2, step 0, sim_offset + s, kind 2)): four
 *               consecutive nodes share a block, as the recovery coins do, and a one-hot row never depends on c.
 *   rates       w_host non-NULL: per-edge rates as in gnode_sir_mc_philox_edges (beta_host must be NULL; gamma_host or the
 *               scalar gamma).  Else beta_host and gamma_host both non-NULL: per-node rates as in gnode_sir_mc_philox_nodes.
 *               Else both NULL: the scalars beta / gamma.  Any other combination is GNODE_ERR_ARG.
 *   events / curves / counts   as in gnode_sir_mc_philox_traj, each may be NULL but not all three.  A node that starts in I
 *               has t_inf = 0, as a seed has; one that starts in R has t_inf = 0 AND t_rec = 0 (the one case of t_rec ==
 *               t_inf).  curves row 0 is the trajectory's drawn state.  counts row 0 is ACCUMULATED like every other row --
 *               the number of trajectories that start in S / I / R -- so shards of the sims range add up on it too.
 * Steps 1 .. T-1 are the other entries', with the same coins (kinds 0 and 1): a node that starts in R is never infected and
 * never infects, and an init that is one-hot I on a seed set and S elsewhere gives the seed-list call's counts exactly on rows
 * t >= 1 and `sims` times its row 0.  The workspace is gnode_sir_edges_workspace_bytes' followed by the two uint64 [n] start
 * thresholds.  A refused call writes nothing.  SYNCHRONISES `stream`, because host arrays are staged.  edge_scan as above. */
size_t gnode_sir_init_workspace_bytes(gnode_graph_t g, int32_t T);
int gnode_sir_mc_philox_init(gnode_graph_t g, const double* init_host,
                             double beta, const double* beta_host, const double* w_host,
                             double gamma, const double* gamma_host,
                             int64_t sims, int64_t sim_offset, int32_t T, uint64_t rng_seed,
                             int16_t* events,    /* device [2, sims, n], OVERWRITTEN, or NULL */
                             uint32_t* curves,   /* device [sims, T, 3], OVERWRITTEN, or NULL */
                             uint32_t* counts,   /* device [3, T, n], ACCUMULATED (row 0 included), or NULL */
                             void* workspace, size_t workspace_bytes, void* stream, int32_t edge_scan);
/* Rates that change over time (no version step: a stale library is known by the missing symbol): the same model with a
 * piecewise-constant SCHEDULE of P >= 1 phases.  A call over T grid points takes steps t = 1 .. T-1, step t leading from state
 * t-1 to state t; phase_host[t] in [0, P) names the tables that govern step t (entry 0 is never read).  Phase p has per-edge
 * weights w_host[p][nnz] and per-node recovery probabilities gamma_host[p][n], under gnode_sir_mc_philox_edges' convention
 * (source = row, target = column).  In step t, on the pre-step state, entry q (row u infected, col[q] = v susceptible) fires
 * iff coin(q, t, sim, kind 0) < thr(w_host[phase[t]][q]), and the infected u recovers iff coin(u, t, sim, kind 1) <
 * thr(gamma_host[phase[t]][u]): the coins and thresholds of the other entries, so one phase gives gnode_sir_mc_philox_traj_edges'
 * / gnode_sir_mc_philox_init's output exactly, as do several phases that hold equal tables.  The one rate form is the most
 * general; a caller restates scalars and per-node rates as such tables (w[q] = beta[col[q]]).
 *   start       a seed list (seeds_host, n_seeds; init_host NULL): outputs and the row-0 rule of gnode_sir_mc_philox_traj_edges;
 *               or drawn (init_host, host fp64 [n][3]; seeds_host NULL, n_seeds 0): those of gnode_sir_mc_philox_init.  Both
 *               or neither is GNODE_ERR_ARG.
 *   events / curves / counts   each may be NULL, not all three.  T = 1 is legal (no step, phase_host is not read).
 * GNODE_ERR_ARG: P < 1, a phase outside [0, P) at a step 1 .. T-1, a NaN or a rate outside [0, 1] (the message names the phase
 * and the CSR position or node), and what the other entries refuse; GNODE_ERR_WORKSPACE: a workspace shorter than
 * gnode_sir_schedule_workspace_bytes(g, T, P) -- gnode_sir_workspace_bytes' layout, then uint64 [P][nnz] and [P][n] thresholds,
 * the two uint64 [n] start thresholds and the int32 [T] phase table.  A refused call writes nothing.  SYNCHRONISES `stream`. */
size_t gnode_sir_schedule_workspace_bytes(gnode_graph_t g, int32_t T, int32_t P);
int gnode_sir_mc_philox_schedule(gnode_graph_t g,
                                 const int32_t* seeds_host, int32_t n_seeds,   /* the start: a seed list ... */
                                 const double* init_host,                      /* ... or host fp64 [n][3], then seeds NULL / 0 */
                                 const int32_t* phase_host, int32_t P,         /* host [T], entry 0 ignored, the others in [0, P) */
                                 const double* w_host,                         /* host fp64 [P][nnz], CSR position order */
                                 const double* gamma_host,                     /* host fp64 [P][n] */
                                 int64_t sims, int64_t sim_offset, int32_t T, uint64_t rng_seed,
                                 int16_t* events, uint32_t* curves, uint32_t* counts,
                                 void* workspace, size_t workspace_bytes, void* stream, int32_t edge_scan);
/* Outbreak sizes for many candidates in one launch (no version step: a stale library is known by the missing symbol): C x sims
 * trajectories of gnode_sir_mc_philox_schedule's drawn-start form, the Monte-Carlo counterpart of
 * gnode_dmp_outbreak_sizes_schedule_f32.  Trajectory (c, s) draws the start of trajectory sim_offset + s from init_host, as
 * gnode_sir_mc_philox_init does, and then node candidates_host[c] alone is changed -- action 0 (seed): it starts in I; action 1
 * (immunise): it starts in R, t_inf = t_rec = 0, never infected and never infecting, as every R start.  An id outside [0, n)
 * matches no node and gives the start as drawn; -1 is the documented spelling.  Repeated ids are allowed.  Step t = 1 .. T-1 of
 * (c, s) reads the tables of phase_host[shifts_host[c] + t], while its coins stay keyed by the run's own t: (c, shift k) under a
 * phase row equals (c, shift 0) under the row moved by k, integer for integer.  The coin of (position, step, sim, kind) does not
 * know c, so candidates are compared on common random numbers.
 *   phase_host  host int32 [L], L >= T; entries 1 .. L-1 in [0, P) (entry 0 is never read); w_host [P][nnz], gamma_host [P][n]
 *               as in gnode_sir_mc_philox_schedule
 *   shifts_host host int32 [C], each >= 0 with shift + T <= L, or NULL: all 0
 *   sums        device uint64 [C][T][3], ACCUMULATED by integer atomic adds: sums[c][t] += (S_t, I_t, R_t) of every trajectory of
 *               c; row 0 is the start after the override, rows after an early end of the epidemic repeat the final state.
 *               Integer adds commute: the result is exact and does not depend on the order of the jobs, the grid or the path,
 *               and shards of the sims range add up.
 *   ever        device uint32 [C][sims], OVERWRITTEN, or NULL: the number of nodes of trajectory (c, s) that were infected at
 *               any step 0 .. T-1; nodes that start in I count, nodes that start in R (the immunised candidate included) do
 *               not.  Hence sum_s ever[c][s] = sums[c][T-1][1] + sums[c][T-1][2] - sums[c][0][2] of the same call.
 * No histogram, no events and no curves are allocated or written.  GNODE_ERR_ARG: what gnode_sir_mc_philox_schedule refuses,
 * C < 1, an action other than 0 or 1, L < T, a shift that is negative or reaches past L, a phase outside [0, P) anywhere in
 * 1 .. L-1; GNODE_ERR_WORKSPACE: a workspace shorter than gnode_sir_sweep_workspace_bytes(g, T, P, L, C) -- the scheduled call's
 * layout without the histogram and the seed list, with an int32 [L] phase row and the int32 [C] candidates and shifts behind it;
 * the query answers 0 for a null handle, T < 1, P < 1, L < T or C < 1.  A refused call writes nothing.  sims = 0 is valid and
 * touches neither output.  SYNCHRONISES `stream`, because host arrays are staged.  edge_scan as above. */
size_t gnode_sir_sweep_workspace_bytes(gnode_graph_t g, int32_t T, int32_t P, int32_t L, int32_t C);
int gnode_sir_mc_philox_sweep(gnode_graph_t g, const double* init_host,          /* host fp64 [n][3] */
                              const int32_t* candidates_host,                    /* host [C] */
                              const int32_t* shifts_host,                        /* host [C], or NULL: all 0 */
                              int32_t C, int32_t action,
                              const int32_t* phase_host, int32_t P, int32_t L,   /* host [L] */
                              const double* w_host,                              /* host fp64 [P][nnz] */
                              const double* gamma_host,                          /* host fp64 [P][n] */
                              int64_t sims, int64_t sim_offset, int32_t T, uint64_t rng_seed,
                              uint64_t* sums,     /* device [C][T][3], ACCUMULATED */
                              uint32_t* ever,     /* device [C][sims], OVERWRITTEN, or NULL */
                              void* workspace, size_t workspace_bytes, void* stream, int32_t edge_scan);
/* Monte-Carlo source scores (no version step: a stale library is known by the missing symbol): the trajectories of
 * gnode_sir_mc_philox_sweep -- same candidates, override, shifts, coins and job order -- with every step of every trajectory
 * compared with O snapshots of the epidemic, the soft-margin estimator's raw material (Antulov-Fantulin et al., PRL 2015).
 *   obs_host   host int8 [O][n]: -1 not observed, 0 / 1 / 2 = S / I / R (gnode_dmp_source_scores_f32's codes); 1 <= O <= 16
 *              (GN_SIR_SCORE_MAXO of the build), every snapshot observing at least one node
 *   measure    the similarity phi = num / den of a state with snapshot o, over the observed nodes only:
 *              0 (Jaccard)  num = |A & B|, den = |A | B|, A = the nodes with code 1 or 2, B = the observed nodes that have left S
 *              1 (match)    num = the observed nodes whose state equals their code, den = the observed nodes
 *   bins       1 .. 4096: the bin of a state is k = (num * bins) / den in 64-bit integer division, k = bins when den = 0; hence
 *              k = bins exactly when state and snapshot agree completely, and bin k < bins holds phi in [k / bins, (k + 1) / bins)
 *   hist       device uint64 [O][C][T][bins + 1], ACCUMULATED by integer atomic adds: hist[o][c][t][k] += 1 for every trajectory
 *              of candidate c whose step t falls into bin k of snapshot o (row 0 is the start after the override, rows after an
 *              early end of the epidemic repeat the final bin), so sum_k hist[o][c][t][k] grows by sims.  Exact, whatever the
 *              order of the jobs, the grid or the path; shards of the sims range add up.  The floating-point kernel of any width
 *              is applied to these integers by the caller: hist[..][bins] / sims is the exact-match frequency.
 * No sums, no ever, no events.  GNODE_ERR_ARG, before any launch and with `hist` untouched: what gnode_sir_mc_philox_sweep
 * refuses, O outside [1, 16], bins outside [1, 4096], a measure other than 0 or 1, a code outside [-1, 2], a snapshot that
 * observes no node, O * C * T * (bins + 1) >= 2^31; GNODE_ERR_WORKSPACE: a workspace shorter than
 * gnode_sir_sweep_scores_workspace_bytes(g, T, P, L, C, O) -- the sweep's layout, then the snapshots staged node-major and two
 * int32 [O] tables; the query answers 0 where the sweep's does and for O outside [1, 16].  sims = 0 is valid and touches
 * nothing.  SYNCHRONISES `stream`.  edge_scan as above. */
size_t gnode_sir_sweep_scores_workspace_bytes(gnode_graph_t g, int32_t T, int32_t P, int32_t L, int32_t C, int32_t O);
int gnode_sir_mc_philox_sweep_scores(gnode_graph_t g, const double* init_host,   /* host fp64 [n][3] */
                                     const int32_t* candidates_host,             /* host [C] */
                                     const int32_t* shifts_host,                 /* host [C], or NULL: all 0 */
                                     int32_t C, int32_t action,
                                     const int32_t* phase_host, int32_t P, int32_t L,   /* host [L] */
                                     const double* w_host,                       /* host fp64 [P][nnz] */
                                     const double* gamma_host,                   /* host fp64 [P][n] */
                                     const int8_t* obs_host, int32_t O,          /* host int8 [O][n] */
                                     int32_t measure, int32_t bins,
                                     int64_t sims, int64_t sim_offset, int32_t T, uint64_t rng_seed,
                                     uint64_t* hist,     /* device [O][C][T][bins + 1], ACCUMULATED */
                                     void* workspace, size_t workspace_bytes, void* stream, int32_t edge_scan);
/* Monte-Carlo source scores from timed evidence (no version step: a stale library is known by the missing symbol): the
 * trajectories of gnode_sir_mc_philox_sweep -- same candidates, override, shifts, coins and job order -- each compared, for every
 * possible age t = 0 .. T-1 of the outbreak, with ALL records of an evidence set jointly, and counted by the number of records it
 * agrees with.  Record i belongs to set rec_set[i] in [0, O) and says that node rec_node[i] was seen rec_offset[i] <= 0 steps
 * from "now" in kind rec_kind[i] (gnode.dmp.timed_observations' records):
 *   0 / 1 / 2  it was S / I / R then;   3  it became infected at that step;   4  it recovered at that step.
 * With t_inf[v], t_rec[v] the event steps of a trajectory as gnode_sir_mc_philox_traj reports them (-1 never; an I start has
 * t_inf = 0, an R start t_inf = t_rec = 0) and "now" = t, the record is read at model step m = t + offset and is MATCHED when
 *   m < 0   (before the outbreak: everybody susceptible)  kind == 0
 *   m >= 0  kind 0: not 0 <= t_inf[v] <= m;   kind 1: 0 <= t_inf[v] <= m and not 0 <= t_rec[v] <= m;   kind 2: 0 <= t_rec[v] <= m;
 *           kind 3: t_inf[v] == m;   kind 4: t_rec[v] == m.
 *   rec_set, rec_node, rec_offset, rec_kind   host int32 [R] each, R >= 1; 1 <= O <= 16 (GN_SIR_SCORE_MAXO of the build) sets,
 *              every one holding a record, and O * T <= 2048 (GN_SIR_TIMED_CELLS: the kernels' difference array in LDS).  A node
 *              may have several records, in one set or in several.
 *   bins       1 .. 4096: the bin of (trajectory, t) in set o is k = (agree * bins) / records in integer division, agree the
 *              matched records of the set and records >= 1 its size: k = bins exactly when EVERY record is matched
 *   hist       device uint64 [O][C][T][bins + 1], ACCUMULATED by integer atomic adds: hist[o][c][t][k] += 1 for every trajectory
 *              of candidate c whose age t falls into bin k of set o, so sum_k hist[o][c][t][k] grows by sims.  Exact, whatever
 *              the order of the jobs, the grid or the path; shards of the sims range add up.  hist[..][bins] / sims is an
 *              unbiased estimate of the joint likelihood P(all records | source c, age t).
 * No sums, no ever, no events.  GNODE_ERR_ARG, before any launch and with `hist` untouched: what gnode_sir_mc_philox_sweep
 * refuses, O outside [1, 16], O * T > 2048, bins outside [1, 4096], O * C * T * (bins + 1) >= 2^31, R < 1, a set outside [0, O),
 * a node outside [0, n), a kind outside [0, 4], an offset > 0, a set without a record; GNODE_ERR_WORKSPACE: a workspace shorter
 * than gnode_sir_sweep_timed_workspace_bytes(g, T, P, L, C, O, R) -- the sweep's layout, then an int32 [n + 1] index of the
 * records by node, one word per record and two int32 [O] tables; the query answers 0 where the sweep's does, for O outside
 * [1, 16] and for R < 1.  sims = 0 is valid and touches nothing.  SYNCHRONISES `stream`.  edge_scan as above. */
size_t gnode_sir_sweep_timed_workspace_bytes(gnode_graph_t g, int32_t T, int32_t P, int32_t L, int32_t C, int32_t O, int32_t R);
int gnode_sir_mc_philox_sweep_timed(gnode_graph_t g, const double* init_host,    /* host fp64 [n][3] */
                                    const int32_t* candidates_host,              /* host [C] */
                                    const int32_t* shifts_host,                  /* host [C], or NULL: all 0 */
                                    int32_t C, int32_t action,
                                    const int32_t* phase_host, int32_t P, int32_t L,   /* host [L] */
                                    const double* w_host,                        /* host fp64 [P][nnz] */
                                    const double* gamma_host,                    /* host fp64 [P][n] */
                                    const int32_t* rec_set, const int32_t* rec_node,          /* host [R] each */
                                    const int32_t* rec_offset, const int32_t* rec_kind, int32_t R, int32_t O,
                                    int32_t bins,
                                    int64_t sims, int64_t sim_offset, int32_t T, uint64_t rng_seed,
                                    uint64_t* hist,     /* device [O][C][T][bins + 1], ACCUMULATED */
                                    void* workspace, size_t workspace_bytes, void* stream, int32_t edge_scan);
/* Monte-Carlo nowcast and forecast from timed evidence (no version step: a stale library is known by the missing symbol): the
 * trajectories of gnode_sir_mc_philox_sweep -- same candidates, override, shifts, coins and job order -- each held against the
 * records of gnode_sir_mc_philox_sweep_timed at ONE age `now` of the outbreak, by rejection sampling.  Trajectory (c, s) is
 * ACCEPTED for set o when every record of the set is matched at age `now`, by the definition above: agree[o][now] == records[o].
 *   now        in [0, T): the age of the outbreak at which the records' offsets are anchored
 *   horizons_host   host int32 [H], 1 <= H <= 32 (GN_SIR_POST_MAXH of the build): whole numbers >= 0, ascending, with
 *              now + horizons[H - 1] <= T - 1
 *   accepted   device uint64 [O][C], ACCUMULATED: accepted[o][c] += the accepted trajectories of candidate c for set o.  It is
 *              what gnode_sir_mc_philox_sweep_timed adds to hist[o][c][now][bins] for the same seed.
 *   counts     device uint64 [O][H][2][n], ACCUMULATED: over the accepted trajectories of ALL candidates, counts[o][j][0][v] += those
 *              in which node v is I at model step now + horizons[j], counts[o][j][1][v] += those in which it is R; S is the
 *              accepted total minus the two.  A trajectory that ended early keeps its final state at every later step.
 * Both by integer atomic adds: exact, whatever the order of the jobs, the grid or the path; shards of the sims range add up.
 * With a set that is always matched (one kind-0 record further back than T) accepted grows by sims everywhere and the sum of
 * counts[o][j][k] over the nodes is what gnode_sir_mc_philox_sweep adds to sums[c][now + horizons[j]][1 + k], summed over c.  A
 * trajectory that no set accepts ends at step `now`; none runs past step now + horizons[H - 1].  1 <= O <= 16; no O * T limit.
 * No sums, no ever, no histogram.  GNODE_ERR_ARG, before any launch and with both outputs untouched: what
 * gnode_sir_mc_philox_sweep refuses, O outside [1, 16], now outside [0, T), H outside [1, 32], a horizon < 0, not ascending or
 * with now + horizon > T - 1, O * H * 2 * n >= 2^31, and what gnode_sir_mc_philox_sweep_timed refuses of the records;
 * GNODE_ERR_WORKSPACE: a workspace shorter than gnode_sir_sweep_posterior_workspace_bytes(g, T, P, L, C, O, R, H) -- the timed
 * call's tables behind the sweep's layout, then the horizons; the query answers 0 where the timed one does and for H outside
 * [1, 32].  sims = 0 is valid and touches nothing.  SYNCHRONISES `stream`.  edge_scan as above. */
size_t gnode_sir_sweep_posterior_workspace_bytes(gnode_graph_t g, int32_t T, int32_t P, int32_t L, int32_t C, int32_t O, int32_t R, int32_t H);
int gnode_sir_mc_philox_sweep_posterior(gnode_graph_t g, const double* init_host,    /* host fp64 [n][3] */
                                        const int32_t* candidates_host,              /* host [C] */
                                        const int32_t* shifts_host,                  /* host [C], or NULL: all 0 */
                                        int32_t C, int32_t action,
                                        const int32_t* phase_host, int32_t P, int32_t L,   /* host [L] */
                                        const double* w_host,                        /* host fp64 [P][nnz] */
                                        const double* gamma_host,                    /* host fp64 [P][n] */
                                        const int32_t* rec_set, const int32_t* rec_node,          /* host [R] each */
                                        const int32_t* rec_offset, const int32_t* rec_kind, int32_t R, int32_t O,
                                        int32_t now, const int32_t* horizons_host, int32_t H,     /* host [H] */
                                        int64_t sims, int64_t sim_offset, int32_t T, uint64_t rng_seed,
                                        uint64_t* counts,     /* device [O][H][2][n], ACCUMULATED */
                                        uint64_t* accepted,   /* device [O][C], ACCUMULATED */
                                        void* workspace, size_t workspace_bytes, void* stream, int32_t edge_scan);
/* The same nowcast from evidence that may be wrong (no version step: a stale library is known by the missing symbol): the
 * trajectories, records, `now` and horizons of gnode_sir_mc_philox_sweep_posterior, each trajectory kept by the number of records it
 * MISSES instead of being dropped at the first.  For trajectory (c, s) and set o, d = records[o] - agree[o][now]; it is ACCEPTED
 * for set o in STRATUM d when d <= mismatches.
 *   mismatches  M in [0, 7] (GN_SIR_POST_MAXD - 1 of the build); D = M + 1 strata
 *   accepted   device uint64 [O][C][D], ACCUMULATED: accepted[o][c][d] += the trajectories of candidate c that miss exactly d
 *              records of set o.  It is what gnode_sir_mc_philox_sweep_timed adds to hist[o][c][now][records[o] - d] with bins =
 *              records[o] for the same seed.
 *   counts     device uint64 [O][D][H][2][n], ACCUMULATED: over the trajectories of ALL candidates accepted for set o in stratum d,
 *              counts[o][d][j][0][v] += those in which node v is I at model step now + horizons[j], counts[o][d][j][1][v] += those
 *              in which it is R.  A trajectory that ended early keeps its final state at every later step.
 * Both by integer atomic adds: exact, whatever the order of the jobs, the grid or the path; shards of the sims range add up.
 * Stratum 0 is gnode_sir_mc_philox_sweep_posterior's output; the output for a smaller M is the first strata of that for a larger
 * one; a set with records[o] <= M accepts every trajectory.  Weighted by (e / (1 - e))^d the strata are the posterior when each
 * record independently contradicts the truth with probability e, exactly where records[o] <= M.  A trajectory that no set
 * accepts ends at step `now`; none runs past step now + horizons[H - 1].  GNODE_ERR_ARG, before any launch and with both outputs
 * untouched: what gnode_sir_mc_philox_sweep_posterior refuses, mismatches outside [0, 7] and O * D * H * 2 * n >= 2^31;
 * GNODE_ERR_WORKSPACE: a workspace shorter than gnode_sir_sweep_posterior_workspace_bytes(g, T, P, L, C, O, R, H) -- the strata
 * size only the two outputs.  sims = 0 is valid and touches nothing.  SYNCHRONISES `stream`.  edge_scan as above. */
int gnode_sir_mc_philox_sweep_posterior_strata(gnode_graph_t g, const double* init_host,    /* host fp64 [n][3] */
                                               const int32_t* candidates_host,              /* host [C] */
                                               const int32_t* shifts_host,                  /* host [C], or NULL: all 0 */
                                               int32_t C, int32_t action,
                                               const int32_t* phase_host, int32_t P, int32_t L,   /* host [L] */
                                               const double* w_host,                        /* host fp64 [P][nnz] */
                                               const double* gamma_host,                    /* host fp64 [P][n] */
                                               const int32_t* rec_set, const int32_t* rec_node,          /* host [R] each */
                                               const int32_t* rec_offset, const int32_t* rec_kind, int32_t R, int32_t O,
                                               int32_t now, const int32_t* horizons_host, int32_t H,     /* host [H] */
                                               int32_t mismatches,
                                               int64_t sims, int64_t sim_offset, int32_t T, uint64_t rng_seed,
                                               uint64_t* counts,     /* device [O][D][H][2][n], ACCUMULATED */
                                               uint64_t* accepted,   /* device [O][C][D], ACCUMULATED */
                                               void* workspace, size_t workspace_bytes, void* stream, int32_t edge_scan);
int gnode_sir_mc_coins(const int32_t* table_src, const int32_t* table_dst, int64_t n_table, int32_t n,
                       const int32_t* seeds_host, int32_t n_seeds, double beta, double gamma, int64_t sims,
                       int32_t T, const double* coins, int64_t n_coins, uint32_t* counts,
                       int64_t* coins_used_host, void* workspace, size_t workspace_bytes, void* stream);

/* ---- DMP baseline (reference dmp.py:74-170, `DMP_SIR.run`) ----
 * Dynamic message passing marginals of the SIR process on an UNDIRECTED graph
 * (symmetric sparsity pattern; GNODE_ERR_ARG otherwise).  Directed edges are the
 * CSR positions of the handle in row-major order (what `sp.coo_matrix(weight_adj)`
 * yields, dmp.py:67-72).
 *   weights   device fp32 [nnz]   transmission probability of each directed edge
 *                                 (the reference passes A*beta, dmp.py:349); may be NULL when nnz = 0
 *   gamma     device fp32 [n]     recovery probability of each node (dmp.py:349)
 *   out       device fp32 [maxTime, n, 3] = (Ps, Pi, Pr), row 0 = initial state
 *                                 (`DMP_SIR.output()`, dmp.py:159-162)
 * The seed list is the state (1 - seed, seed, 0) per node: it is written to out row 0, and the call is
 * gnode_dmp_batch_f32's general form with B = 1 reading its start from there.
 * Synchronises `stream` (host arrays are staged through the workspace).
 * Not on the `model='ode_nn'` path: a comparison column of the paper. */
size_t gnode_dmp_workspace_bytes(gnode_graph_t g);
int gnode_dmp_f32(gnode_graph_t g, const float* weights, const float* gamma, const int32_t* seeds_host,
                  int32_t n_seeds, int32_t maxTime, float* out, void* workspace, size_t workspace_bytes,
                  void* stream);
/* gnode_dmp_f32 from an initial-state distribution instead of a seed list: init is device fp32 [n][3] = (pS, pI, pR) per
 * node (not validated here: it lives on the device).  Ps_0 = pS, Pi_0 = pI, Pr_0 = pR, the message of edge (i -> j) starts from
 * Phi_0 = Pi_0[i] (the reference's 1 - Ps_0[i] is the same number when pR = 0), Pr_1 = Pr_0 + gamma Pi_0, everything after
 * that as gnode_dmp_f32, the 1e-10 offset included: a one-hot seed state returns gnode_dmp_f32's output bit for bit.  It is
 * gnode_dmp_batch_f32's general form with B = 1, at every graph size. */
size_t gnode_dmp_init_workspace_bytes(gnode_graph_t g);
int gnode_dmp_init_f32(gnode_graph_t g, const float* weights, const float* gamma,
                       const float* init /* device fp32 [n][3] */, int32_t maxTime, float* out,
                       void* workspace, size_t workspace_bytes, void* stream);
/* The recurrence for B samples on one graph in one call.  Sample b starts from init[b], with the weights at
 * weights + b * w_stride and the recovery probabilities at gamma + b * gamma_stride: a stride of 0 shares one table among
 * the samples, the other legal value is the table's length (nnz, n).  The library states the recurrence once, for every entry
 * and both forms below, in one per-element order (P_k multiplies over row k in ascending position from 1.0f), and no sample
 * reads another's numbers: out[b] is bit for bit what gnode_dmp_init_f32 returns for sample b's weights, gamma and state.  In
 * the general form that holds by construction -- the solo entries ARE that form with B = 1 -- and in the one-workgroup form
 * because it calls the same arithmetic on values held in LDS.
 *   weights   device fp32 [nnz] (w_stride 0) or [B][nnz] (w_stride nnz); may be NULL when nnz = 0
 *   gamma     device fp32 [n] (gamma_stride 0) or [B][n] (gamma_stride n)
 *   init      device fp32 [B][n][3] = (pS, pI, pR), not validated here
 *   out       device fp32 [B][maxTime][n][3], out[b][0] = init[b]
 * The source / reverse-edge tables are the handle's.  Two forms, chosen from the graph alone: when
 * gnode_dmp_batch_lds_bytes(g) -- 5 edge arrays (theta twice, phi, Ps_e, rev) and 3 node arrays (P, Pi, Pr) of 4 bytes,
 * each rounded up to 16 -- fits the 160 KiB of LDS of a gfx950 workgroup, one workgroup integrates one sample over the whole
 * horizon from LDS, in ONE launch for the batch; otherwise the node and edge passes run over B * n rows and B * nnz edge slots
 * of the workspace, two launches per time step whatever B is.  gnode_dmp_batch_lds_bytes and
 * gnode_dmp_batch_workspace_bytes return 0 without a handle (the latter also for B < 1).
 * GNODE_ERR_ARG: a null pointer, B < 1, maxTime < 2, a stride that is neither 0 nor the table's length, an asymmetric
 * pattern; GNODE_ERR_WORKSPACE: a short workspace; nothing is written to `out` in either case.  Synchronises `stream`. */
size_t gnode_dmp_batch_workspace_bytes(gnode_graph_t g, int32_t B);
size_t gnode_dmp_batch_lds_bytes(gnode_graph_t g);
int gnode_dmp_batch_f32(gnode_graph_t g, const float* weights, int64_t w_stride, const float* gamma,
                        int64_t gamma_stride, const float* init /* device fp32 [B][n][3] */, int32_t B,
                        int32_t maxTime, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* Rates that change over time (no version step: a stale library is known by the missing symbol): gnode_dmp_batch_f32 with a
 * piecewise-constant schedule of P >= 1 phases.  Step t = 1 .. maxTime-1 leads from state t-1 to state t under the tables of
 * phase_host[t] in [0, P) (entry 0 is never read):
 *   theta_1     = (1 - w^{phase[1]} phi_0) + 1e-10
 *   node pass t   Pr_t = Pr_{t-1} + gamma^{phase[t]} Pi_{t-1}; Ps_t and Pi_t as in gnode_dmp_batch_f32
 *   edge pass t   (only when t + 1 < maxTime)
 *                 phi_t = (1 - w^{phase[t]})(1 - gamma^{phase[t]}_src) phi_{t-1} - (Ps_e(t) - Ps_e(t-1))
 *                 theta_{t+1} = theta_t - w^{phase[t+1]} phi_t
 * phi_t -- infected, and neither transmitted nor recovered during step t -- reads step t's tables; theta_{t+1} - theta_t is the
 * transmission DURING step t + 1 and reads that step's weight.  Operand order and rounding are gnode_dmp_batch_f32's, so one
 * phase, or several that hold equal tables, return its bits; so does sample b of a batch with respect to its B = 1 call.
 *   weights   device fp32 [P][nnz] (w_stride 0) or [B][P][nnz] (w_stride P * nnz); may be NULL when nnz = 0
 *   gamma     device fp32 [P][n] (gamma_stride 0) or [B][P][n] (gamma_stride P * n)
 *   init, out as in gnode_dmp_batch_f32.  The two tables are read back once and validated on the host: a NaN or an entry
 *             outside [0, 1] is GNODE_ERR_ARG, the message names the sample, the phase and the position
 * The two forms are gnode_dmp_batch_f32's, chosen by gnode_dmp_batch_lds_bytes (the tables are never held in LDS): the
 * one-workgroup form reads a device copy of the phase table at every step, the general form's launches get their step's table
 * offsets from the host loop.  The workspace holds that copy, then the general form's arrays.
 * GNODE_ERR_ARG: a null pointer, B < 1, maxTime < 2, P < 1, a phase outside [0, P) at a step 1 .. maxTime-1, a stride that is
 * neither 0 nor the table's length, a NaN or out-of-range rate, an asymmetric pattern; GNODE_ERR_WORKSPACE: a short workspace; nothing is written to `out`
 * in either case.  Synchronises `stream`. */
size_t gnode_dmp_batch_schedule_workspace_bytes(gnode_graph_t g, int32_t B, int32_t maxTime);
int gnode_dmp_batch_schedule_f32(gnode_graph_t g,
                                 const float* weights, int64_t w_stride,       /* device [P][nnz] (stride 0) or [B][P][nnz] (P * nnz) */
                                 const float* gamma, int64_t gamma_stride,     /* device [P][n] (stride 0) or [B][P][n] (P * n) */
                                 const int32_t* phase_host, int32_t P,         /* host [maxTime], entry 0 ignored */
                                 const float* init, int32_t B, int32_t maxTime, float* out,
                                 void* workspace, size_t workspace_bytes, void* stream);
/* The reverse sweep of gnode_dmp_batch_f32's recurrence (constant rates): the gradient of sum(grad_out * out) with respect
 * to the weights, the recovery probabilities and the start, for B samples on one graph, fp32.  weights, gamma, init, the strides, B and maxTime are the
 * forward call's; `out` is what it returned (the sweep reads Pi_{t-1} from it) and grad_out has its shape.
 *   grad_w      device fp32 [B][nnz], in CSR position order     grad_gamma  device fp32 [B][n]     grad_init  device fp32 [B][n][3]
 * One row per sample even where the forward's table is shared (stride 0): the caller sums the rows of a shared table.  A
 * NULL gradient pointer means "not wanted"; grad_w may also be NULL when nnz = 0.  The entry runs the forward again into the
 * workspace with the forward's own arithmetic, keeping theta_t and phi_t of every step (2 * nnz * 4 bytes per step and sample);
 * P_t is recomputed from theta_t.  Then, from t = maxTime - 1 down to 1, an edge pass (absent at maxTime - 1) and a node pass
 * carry the adjoints of theta, phi, Ps_e per edge and of Pi, Pr per node; every sum runs over the rows of one node in
 * ascending position and every scattered value goes to the reverse edge's slot, written once per step, so there are no
 * atomics and the result is deterministic.  Two forms, chosen from the graph alone: when
 * gnode_dmp_batch_backward_lds_bytes(g) -- 7 edge arrays (theta_bar twice, phi_bar, q_bar, two hand-overs, rev) and 2 node
 * arrays (pi_bar, pr_bar) of 4 bytes, each rounded up to 16 -- fits the 160 KiB of LDS of a gfx950 workgroup, one workgroup
 * sweeps one sample with its adjoint state in LDS, in ONE launch for the batch; otherwise the passes run over B * n rows and
 * B * nnz edge slots of the workspace.  Both call the same arithmetic in the same per-element order: a sample's gradient does
 * not depend on the form or on B.  gnode_dmp_backward_f32 is one sample without strides, in the general form at every graph
 * size (as the forward's solo entries are), so it returns row b of the batch entry bit for bit.
 * Where the forward is not finite (theta = 0: a weight of 1 next to a seed) the gradient is unspecified.
 * The size queries return 0 without a handle, for B < 1 and for maxTime < 2.
 * GNODE_ERR_ARG: a null out, grad_out, init, gamma or workspace, weights null with nnz > 0, B < 1, maxTime < 2, a stride that
 * is neither 0 nor the table's length, all three gradient pointers null, an asymmetric pattern; GNODE_ERR_WORKSPACE: a short
 * workspace; nothing is written to the gradients in either case.  Synchronises `stream`. */
size_t gnode_dmp_batch_backward_lds_bytes(gnode_graph_t g);
size_t gnode_dmp_batch_backward_workspace_bytes(gnode_graph_t g, int32_t B, int32_t maxTime);
int gnode_dmp_batch_backward_f32(gnode_graph_t g, const float* weights, int64_t w_stride, const float* gamma,
                                 int64_t gamma_stride, const float* init /* device fp32 [B][n][3] */, int32_t B,
                                 int32_t maxTime, const float* out /* the forward's [B][maxTime][n][3] */,
                                 const float* grad_out /* the same shape */, float* grad_w /* [B][nnz] or NULL */,
                                 float* grad_gamma /* [B][n] or NULL */, float* grad_init /* [B][n][3] or NULL */,
                                 void* workspace, size_t workspace_bytes, void* stream);
size_t gnode_dmp_backward_workspace_bytes(gnode_graph_t g, int32_t maxTime);
int gnode_dmp_backward_f32(gnode_graph_t g, const float* weights, const float* gamma, const float* init /* device fp32 [n][3] */,
                           int32_t maxTime, const float* out /* the forward's [maxTime][n][3] */,
                           const float* grad_out /* the same shape */, float* grad_w /* [nnz] or NULL */,
                           float* grad_gamma /* [n] or NULL */, float* grad_init /* [n][3] or NULL */,
                           void* workspace, size_t workspace_bytes, void* stream);
/* The reverse sweep under a rate schedule (no version step: a stale library is known by the missing symbol): the gradient of
 * sum(grad_out * out) for gnode_dmp_batch_schedule_f32's recurrence, with respect to every phase's tables and the start.
 * weights, the strides, gamma, phase_host, P, init, B and maxTime are the scheduled forward's arguments, checked as there (the
 * tables are read back once: a NaN or an entry outside [0, 1] is named by sample, phase and position); `out` is what it
 * returned and grad_out has its shape.
 *   grad_w      device fp32 [B][P][nnz]     grad_gamma  device fp32 [B][P][n]     grad_init  device fp32 [B][n][3]
 * One block per sample even where the forward's table is shared; NULL means "not wanted", and grad_w may be NULL when nnz = 0.
 * The entry zeroes the gradients it is given, so a phase that no step names comes back as exact zeros.  The sweep is
 * gnode_dmp_batch_backward_f32's with each step's adjoint going to its phase, p_t = phase_host[t]:
 *   edge pass t (t + 1 < maxTime)   pb = phi_bar - w^{p_{t+1}} theta_bar;   w_bar^{p_{t+1}} -= phi_t theta_bar  (theta_{t+1}'s
 *                                   weight is the NEXT step's);   w_bar^{p_t} -= ((1 - gamma^{p_t}_u) phi_{t-1}) pb;   gamma^{p_t}_u
 *                                   gets -((1 - w^{p_t}) phi_{t-1}) pb;   phi_bar <- ((1 - w^{p_t})(1 - gamma^{p_t}_u)) pb
 *   node pass t                     gamma_bar^{p_t}_k += Pi_{t-1}[k] aR and its row's shares;   pi_bar <- gamma^{p_t}_k aR
 *   after t = 1                     w_bar^{p_1} -= Pi_0[src] theta_bar;   pi0_bar sums phi_bar - w^{p_1} theta_bar over the row
 * In one pass the thread of edge e writes grad_w[p_t][e] and grad_w[p_{t+1}][e] only, the thread of node k grad_gamma[p_t][k]
 * only; where the two phases are equal the two updates of the one slot happen in the constant sweep's order.  No atomics, a
 * deterministic result; with P = 1 the three gradients are gnode_dmp_batch_backward_f32's bit for bit.  The tape is rebuilt
 * with the scheduled forward's own arithmetic (2 * nnz * 4 bytes per step and sample).  The two forms are the constant
 * backward's, chosen by gnode_dmp_batch_backward_lds_bytes(g) <= 160 KiB (the tables are never held in LDS): one workgroup per
 * sample, which reads a device copy of the phase table at every step, or launches per pass over B * n rows and B * nnz edge
 * slots whose table offsets come from the host loop.  The workspace holds that copy, the tapes, then the general form's arrays;
 * the size query returns 0 without a handle, for B < 1 and for maxTime < 2.
 * GNODE_ERR_ARG: a null pointer, weights null with nnz > 0, B < 1, maxTime < 2, P < 1, a phase outside [0, P) at a step
 * 1 .. maxTime-1, a stride that is neither 0 nor the table's length, all three gradient pointers null, a NaN or out-of-range
 * rate, an asymmetric pattern; GNODE_ERR_WORKSPACE: a short workspace; nothing is written to the gradients in either case.
 * Synchronises `stream`. */
size_t gnode_dmp_batch_schedule_backward_workspace_bytes(gnode_graph_t g, int32_t B, int32_t maxTime);
int gnode_dmp_batch_schedule_backward_f32(gnode_graph_t g,
                                          const float* weights, int64_t w_stride,       /* device [P][nnz] (stride 0) or [B][P][nnz] (P * nnz) */
                                          const float* gamma, int64_t gamma_stride,     /* device [P][n] (stride 0) or [B][P][n] (P * n) */
                                          const int32_t* phase_host, int32_t P,         /* host [maxTime], entry 0 ignored */
                                          const float* init, int32_t B, int32_t maxTime,
                                          const float* out /* the scheduled forward's [B][maxTime][n][3] */,
                                          const float* grad_out /* the same shape */, float* grad_w /* [B][P][nnz] or NULL */,
                                          float* grad_gamma /* [B][P][n] or NULL */, float* grad_init /* [B][n][3] or NULL */,
                                          void* workspace, size_t workspace_bytes, void* stream);
/* Source inference from one snapshot (Lokhov, Mezard, Ohta, Zdeborova 2014): the recurrence from each of C candidate sources,
 * scored against the observed states, without a marginal ever reaching global memory.  Candidate c's sample is
 * gnode_dmp_batch_f32's from the one-hot seed state (1 - [k == candidates[c]], [k == candidates[c]], 0) with the shared
 * weights and gamma -- the same fp32 marginals, bit for bit -- and the kernels make that state from the id: no [C][n][3]
 * start exists.  With p = Ps / Pi / Pr of node k at step t for obs[k] = 0 / 1 / 2,
 *   scores[c][t] = sum over the observed k of log((double)min(max(p, floor), 1.0f)),     t = 0 .. maxTime - 1, row 0 = the start;
 * any other obs[k] means "not observed" and contributes nothing, and a candidate id outside [0, n) matches no node (an
 * all-susceptible start), so the device arrays are not validated and cannot cause an access out of bounds.  The clamp is fp32:
 * Pi = 1 - Ps - Pr can round below 0, Ps can exceed 1 by the 1e-10 offset, and a node further than t from the candidate has
 * probability exactly 0.  The sum is fp64, in a fixed order, without atomics: a thread adds its own nodes in ascending k, a
 * wave of 64 adds its lanes in a fixed tree, the waves' sums are added in ascending wave order.
 *   weights     device fp32 [nnz], may be NULL when nnz = 0        gamma   device fp32 [n]
 *   candidates  device int32 [C]                                   obs     device int32 [n]
 *   floor       in (0, 1]                                          scores  device fp64 [C][maxTime]
 * Two forms, chosen from the graph alone: when gnode_dmp_source_lds_bytes(g) -- gnode_dmp_batch_lds_bytes(g) plus 256 bytes
 * of fp64 reduction scratch -- fits the 160 KiB of LDS of a gfx950 workgroup, one workgroup integrates and scores one
 * candidate from LDS, in ONE launch for the call, and the workspace is one unused unit of 256 bytes; otherwise the node and
 * edge passes run over C * n rows and C * nnz edge slots of the workspace, two launches per time step, each block of 256 nodes
 * leaves one partial at [c][t][block], and a last kernel adds them in ascending block order.  A candidate's row does not
 * depend on C or on its position in the call; within a form the bits are reproducible from call to call (the forms differ in
 * the order of the sum, not in the marginals).  The size queries return 0 without a handle, for C < 1 and for maxTime < 2.
 * GNODE_ERR_ARG: a null pointer (weights may be null when nnz = 0), C < 1, maxTime < 2, floor not in (0, 1], in the general
 * form C * max(blocks of 256 over the nodes, over the edges) >= 2^31, an asymmetric pattern; GNODE_ERR_WORKSPACE: a short
 * workspace; nothing is written to `scores` in either case.  Synchronises `stream`. */
size_t gnode_dmp_source_lds_bytes(gnode_graph_t g);
size_t gnode_dmp_source_workspace_bytes(gnode_graph_t g, int32_t C, int32_t maxTime);
int gnode_dmp_source_scores_f32(gnode_graph_t g, const float* weights, const float* gamma,
                                const int32_t* candidates /* device [C] */, int32_t C, const int32_t* obs /* device [n] */,
                                float floor, int32_t maxTime, double* scores /* device fp64 [C][maxTime] */,
                                void* workspace, size_t workspace_bytes, void* stream);
/* gnode_dmp_source_scores_f32 for O snapshots in one pass of the recurrence: a candidate's marginals do not depend on the
 * observation, so per node and step the three possible terms (p = Ps, Pi, Pr) are computed once and each observation selects
 * one of them, or nothing.
 *   obs     device int8 [O][n]: 0 / 1 / 2 observed, anything else not observed
 *   scores  device fp64: scores[o * score_stride + c * maxTime + t], score_stride >= C * maxTime (so a chunk of candidates can
 *           write its slice of a [O][C_total][maxTime] table), and that entry is BIT FOR BIT what gnode_dmp_source_scores_f32
 *           writes at [c][t] for obs[o] alone: the same form (chosen by gnode_dmp_source_lds_bytes as there), the same launch
 *           shape, the same terms and the same order of every sum.  The other arguments are that entry's.
 * One-workgroup form: a workgroup serves one candidate and a tile of gnode_dmp_source_batch_tile(g) observations, whose sums it
 * keeps in registers, so a candidate's recurrence runs ceil(O / tile) times; the tile is at most 16 and narrows, down to 1, on a
 * graph that leaves less LDS than its wave sums need (256 bytes per observation) -- the form never changes with O.  The
 * workspace is one unused unit of 256 bytes.  General form: the node pass loops over all O observations after its three
 * logarithms, in groups of gnode_dmp_source_batch_tile(g) that share a barrier, so the recurrence runs once per candidate; the
 * workspace holds gnode_dmp_source_scores_f32's arrays and the partials [C][maxTime][O][blocks of 256 nodes] in fp64.
 * gnode_dmp_source_batch_tile returns 0 without a handle; gnode_dmp_source_batch_workspace_bytes returns 0 without a handle,
 * for C < 1, for O < 1 and for maxTime < 2.
 * GNODE_ERR_ARG: a null pointer (weights may be null when nnz = 0), maxTime < 2, C < 1, O < 1, floor not in (0, 1],
 * score_stride < C * maxTime, C * (tiles of observations | blocks of 256 over the nodes or the edges) >= 2^31, an asymmetric
 * pattern; GNODE_ERR_WORKSPACE: a short workspace; nothing is written to `scores` in either case.  Synchronises `stream`. */
int gnode_dmp_source_batch_tile(gnode_graph_t g);
size_t gnode_dmp_source_batch_workspace_bytes(gnode_graph_t g, int32_t C, int32_t O, int32_t maxTime);
int gnode_dmp_source_batch_scores_f32(gnode_graph_t g, const float* weights, const float* gamma,
                                      const int32_t* candidates /* device [C] */, int32_t C, const int8_t* obs /* device [O][n] */,
                                      int32_t O, float floor, int32_t maxTime, double* scores /* device fp64, see above */,
                                      int64_t score_stride, void* workspace, size_t workspace_bytes, void* stream);
/* gnode_dmp_source_batch_scores_f32 for time-stamped evidence: a row code may also say that a node CHANGED state at the model
 * step, which DMP gives as a difference of two consecutive marginals that the node pass holds in registers.
 *   rows    device int8 [R][n], code of node k at model step t -> p:
 *             0 / 1 / 2  susceptible / infected / recovered at t   Ps(t), Pi(t), Pr(t)
 *             3          became infected at step t                 Ps(t-1) - Ps(t),   Ps(-1) = 1.0f for every node
 *             4          recovered at step t                       Pr(t) - Pr(t-1),   Pr(-1) = 0.0f
 *             anything else: not observed, contributes 0.0
 *           and the term is log((double)min(max(p, floor), 1.0f)) for every code; the differences are fp32, of the bits
 *           gnode_dmp_batch_f32 writes at [t-1][k] and [t][k].  At t = 0 a code 3 gives log 1 = 0 at the candidate itself and
 *           log(floor) elsewhere, a code 4 gives log(floor) everywhere.
 *   scores  device fp64: scores[r * score_stride + c * maxTime + t], score_stride >= C * maxTime.  A row whose codes are all
 *           outside 3 / 4 is BIT FOR BIT gnode_dmp_source_batch_scores_f32's row: the same form, launch shape, terms and order
 *           of every sum; a row does not depend on R, C, its position or the other rows.
 * The other arguments, the two forms, the tile (gnode_dmp_source_events_tile, at most 16), the workspace (its size for R rows),
 * the error codes and the queries' zeros (no handle; C, R < 1; maxTime < 2) are gnode_dmp_source_batch_scores_f32's with R for
 * O.  Nothing is written to `scores` when the call is refused.  Synchronises `stream`. */
int gnode_dmp_source_events_tile(gnode_graph_t g);
size_t gnode_dmp_source_events_workspace_bytes(gnode_graph_t g, int32_t C, int32_t R, int32_t maxTime);
int gnode_dmp_source_events_scores_f32(gnode_graph_t g, const float* weights, const float* gamma,
                                       const int32_t* candidates /* device [C] */, int32_t C, const int8_t* rows /* device [R][n] */,
                                       int32_t R, float floor, int32_t maxTime, double* scores /* device fp64, see above */,
                                       int64_t score_stride, void* workspace, size_t workspace_bytes, void* stream);
/* Whom to immunise and where to seed (Lokhov, Saad 2017): the recurrence from each of C candidate interventions on one
 * outbreak, kept only as the expected size of each compartment over time.  Candidate c's sample is gnode_dmp_batch_f32's from
 * the shared base start init[n][3] = (pS, pI, pR) with the triple of node candidates[c] replaced -- action 0 (seed): (0, 1, 0),
 * action 1 (immunise): (0, 0, 1) -- with the shared weights and gamma: the same fp32 marginals, bit for bit (Pr_0 from the
 * triple, phi_0 = Pi_0, as gnode_dmp_init_f32 starts).  The kernels make that start from the id wherever one is read: no
 * [C][n][3] start exists, and an id outside [0, n) (-1 is the documented spelling) matches no node and gives the base start
 * itself, the "do nothing" row; so the candidates are not validated and cannot cause an access out of bounds.  No marginal
 * reaches global memory: with P^k_j(t) = Ps / Pi / Pr of node k at step t for j = 0 / 1 / 2,
 *   sizes[c][t][j] = sum over k of (double)value[k] * (double)P^k_j(t),     t = 0 .. maxTime - 1, row 0 = the start;
 * value == NULL means 1 for every node.  The product of two floats is exact in a double; the sum is fp64, in a fixed order,
 * without atomics: a thread adds its own nodes in ascending k, a wave of 64 adds its lanes in a fixed tree (32 16 8 4 2 1), the
 * waves' sums are added in ascending wave order.
 *   weights     device fp32 [nnz], may be NULL when nnz = 0        gamma   device fp32 [n]
 *   init        device fp32 [n][3]                                 candidates  device int32 [C]
 *   value       device fp32 [n] or NULL                            sizes   device fp64 [C][maxTime][3]
 * Two forms, chosen from the graph alone: when gnode_dmp_outbreak_lds_bytes(g) -- gnode_dmp_batch_lds_bytes(g) plus 768 bytes
 * of fp64 reduction scratch (16 waves' three sums, two steps' worth) -- fits the 160 KiB of LDS of a gfx950 workgroup, one
 * workgroup integrates and sums one candidate from LDS, in ONE launch for the call, and the workspace is one unused unit of 256
 * bytes; otherwise the node and edge passes run over C * n rows and C * nnz edge slots of the workspace, two launches per time
 * step, each block of 256 nodes leaves one partial at [c][t][j][block], and a last kernel adds them in ascending block order.
 * A candidate's rows do not depend on C or on its position in the call; within a form the bits are reproducible from call to
 * call (the forms differ in the order of the sum, not in the marginals).  The size queries return 0 without a handle, for
 * C < 1 and for maxTime < 2.
 * GNODE_ERR_ARG: a null pointer (weights may be null when nnz = 0, value always), maxTime < 2, C < 1, an action other than 0
 * or 1, in the general form C * max(blocks of 256 over the nodes, over the edges) >= 2^31, an asymmetric pattern;
 * GNODE_ERR_WORKSPACE: a short workspace; nothing is written to `sizes` in either case.  Does NOT wait on the host: the call
 * enqueues its kernels on `stream` and returns, allocates nothing and keeps nothing in the handle. */
size_t gnode_dmp_outbreak_lds_bytes(gnode_graph_t g);
size_t gnode_dmp_outbreak_workspace_bytes(gnode_graph_t g, int32_t C, int32_t maxTime);
int gnode_dmp_outbreak_sizes_f32(gnode_graph_t g, const float* weights, const float* gamma, const float* init /* device [n][3] */,
                                 const int32_t* candidates /* device [C] */, int32_t C, int32_t action,
                                 const float* value /* device [n] or NULL */, int32_t maxTime,
                                 double* sizes /* device fp64 [C][maxTime][3] */, void* workspace, size_t workspace_bytes,
                                 void* stream);
/* Source scores and outbreak sizes under rates that change over time (no version step: a stale library is known by the missing
 * symbol): gnode_dmp_source_events_scores_f32 and gnode_dmp_outbreak_sizes_f32 with the schedule of gnode_dmp_batch_schedule_f32
 * -- P >= 1 tables of each kind shared by the samples -- a phase row stated in CALENDAR steps, and per sample a candidate id
 * and a SHIFT: step t = 1 .. maxTime-1 of sample j reads the tables of p_t = phase_host[shifts_host[j] + t],
 *   theta_1 from w^{p_1};   node pass t: gamma^{p_t};   edge pass t (only when t + 1 < maxTime): w^{p_t}, gamma^{p_t}, and w^{p_{t+1}}
 *   for theta_{t+1}
 * exactly as gnode_dmp_batch_schedule_f32 reads them under the row phase_host[shift .. shift + maxTime): sample j's fp32
 * marginals are that call's bit for bit, and the sums are the constant entries' (same form, same launch shape, same order).  A
 * source hypothesis "c started tau steps before the snapshot of calendar step D" is the sample (c, D - tau) read at t = tau;
 * shift 0 for everybody is a schedule that counts from the outbreak's start; candidate -1 of the outbreak entry with shifts
 * 0 .. K-1 prices each step of delay.  A sample's rows do not depend on C, on its position or on the other samples; (c, shift s)
 * under a row equals (c, shift 0) under the row moved by s.  With one phase, or several that hold equal tables, every sample is
 * the constant entry's row bit for bit.
 *   weights      device fp32 [P][nnz], may be NULL when nnz = 0     gamma        device fp32 [P][n]
 *   phase_host   host int32 [L], L >= maxTime, entries 1 .. L-1 in [0, P); entry 0 is never read and travels as 0
 *   candidates   device int32 [C] (a sample's candidate)             shifts_host  host int32 [C], each >= 0 with
 *                                                                                shift + maxTime <= L, or NULL: all 0
 *   rows, R, floor, scores, score_stride: gnode_dmp_source_events_scores_f32's (C counts samples);   init, action, value,
 *   sizes: gnode_dmp_outbreak_sizes_f32's
 * The two tables are read back once and validated on the host after every other check has passed: a NaN or an entry outside
 * [0, 1] is GNODE_ERR_ARG, and the message names the phase and the position.  The tables stay in memory, never in LDS, so the
 * form and the tile are the constant entries' (gnode_dmp_source_events_tile, gnode_dmp_outbreak_lds_bytes).  Both forms read a
 * device copy of the phase row and of the shifts: the workspace holds the phase copy [L] and the shifts [C], each rounded up to
 * 256 bytes, then the constant entry's regions; the queries return 0 where the constant entries' do and for L < maxTime.
 * GNODE_ERR_ARG: whatever the constant entry refuses, a null phase_host, P < 1, L < maxTime, a phase outside [0, P) at an entry
 * 1 .. L-1, a shift < 0 or with shift + maxTime > L, a NaN or out-of-range rate; GNODE_ERR_WORKSPACE: a short workspace; nothing
 * is written to `scores` / `sizes` in either case.  Both entries synchronise `stream` once after staging the host arrays (and
 * while they validate the tables), so phase_host and shifts_host are done with on return; the kernels are enqueued after that
 * and not waited for. */
size_t gnode_dmp_source_events_schedule_workspace_bytes(gnode_graph_t g, int32_t C, int32_t R, int32_t maxTime, int32_t L);
int gnode_dmp_source_events_scores_schedule_f32(gnode_graph_t g, const float* weights /* device [P][nnz] */,
                                                const float* gamma /* device [P][n] */, const int32_t* phase_host /* int32 [L] */,
                                                int32_t P, int32_t L, const int32_t* candidates /* device [C] */,
                                                const int32_t* shifts_host /* int32 [C] or NULL = all 0 */, int32_t C,
                                                const int8_t* rows /* device [R][n] */, int32_t R, float floor, int32_t maxTime,
                                                double* scores /* device fp64, see above */, int64_t score_stride, void* workspace,
                                                size_t workspace_bytes, void* stream);
size_t gnode_dmp_outbreak_schedule_workspace_bytes(gnode_graph_t g, int32_t C, int32_t maxTime, int32_t L);
int gnode_dmp_outbreak_sizes_schedule_f32(gnode_graph_t g, const float* weights /* device [P][nnz] */,
                                          const float* gamma /* device [P][n] */, const int32_t* phase_host /* int32 [L] */, int32_t P,
                                          int32_t L, const float* init /* device [n][3] */, const int32_t* candidates /* device [C] */,
                                          const int32_t* shifts_host /* int32 [C] or NULL = all 0 */, int32_t C, int32_t action,
                                          const float* value /* device [n] or NULL */, int32_t maxTime,
                                          double* sizes /* device fp64 [C][maxTime][3] */, void* workspace, size_t workspace_bytes,
                                          void* stream);

/* ---- mean-field baseline (reference ode_nn.py:214-233) ----
 * `runge_kutta_order4(sir, A, ...)`: dS = -beta (A I) S, dI = beta (A I) S - gamma I,
 * dR = gamma I from S = 1 - seeds, I = seeds, R = 0, float64, sampled at the given
 * times (the reference samples scipy LSODA's solution at int(i/deltaT)*deltaT,
 * ode_nn.py:229-232,235-246).  A = the handle's unweighted adjacency (entries 1,
 * a self-loop counts once).  Adaptive Dormand-Prince 5(4) with steps clipped to the
 * output times; rtol/atol are per component.  t_out_host: host fp64 [n_out],
 * ascending, t_out[0] = 0.  gamma: device fp64 [n].  outI/outS/outR: device fp64
 * [n_out, n] (the reference returns I, S, R in that order).  *steps_host (may be
 * NULL) receives the number of attempted steps.  Synchronises `stream`.
 * Not on the `model='ode_nn'` path: a comparison column of the paper. */
size_t gnode_meanfield_workspace_bytes(gnode_graph_t g);
int gnode_meanfield_f64(gnode_graph_t g, const int32_t* seeds_host, int32_t n_seeds, double beta, const double* gamma,
                        const double* t_out_host, int32_t n_out, double rtol, double atol, double* outI, double* outS,
                        double* outR, int64_t* steps_host, void* workspace, size_t workspace_bytes, void* stream);
/* gnode_meanfield_f64 from y(0) = init, device fp64 [n][3] = (pS, pI, pR) per node, in place of the seed list; the rest,
 * gnode_meanfield_workspace_bytes included, is the same. */
int gnode_meanfield_init_f64(gnode_graph_t g, const double* init, double beta, const double* gamma,
                             const double* t_out_host, int32_t n_out, double rtol, double atol, double* outI, double* outS,
                             double* outR, int64_t* steps_host, void* workspace, size_t workspace_bytes, void* stream);
/* The mean-field with per-node and per-contact rates, for B samples on one graph in one integration.  For sample b, node v:
 *     dS_v = -beta[b][v] S_v sum_{p in row v} w_in[p] I[b][col[p]],  dI_v = -dS_v - gamma[b][v] I_v,  dR_v = gamma[b][v] I_v
 * where w_in[p] = w[rev(p)] is the weight of the contact col[p] -> v.  `w` comes in the convention of
 * gnode_sir_mc_philox_edges and gnode_dmp_f32 (w[p], in row u with col[p] = v, is the rate at which u infects v); the entry
 * gathers w_in into the workspace through the handle's reverse-edge table.  With `w` given the sparsity pattern must be symmetric (GNODE_ERR_ARG
 * otherwise); a directed contact is a zero on the reverse entry; a self-loop is its own reverse and counts once.
 *   init    device fp64 [B][n][3] = (pS, pI, pR) per sample and node
 *   beta    device fp64 [B][n], indexed by the TARGET node (x[:, 3]'s convention), or NULL = 1
 *   w       device fp64 [nnz], CSR position order, source = row, target = column, or NULL = 1 (no table is built)
 *   gamma   device fp64 [B][n]
 *   outI/outS/outR  device fp64 [n_out][B * n], row r = b * n + node
 * The same Dormand-Prince 5(4) as gnode_meanfield_f64 over the 3 * B * n state with ONE shared step size: the error norm is
 * the maximum over every sample, so a sample's numbers inside a batch differ from its solo run at the level of the
 * tolerances, not bit for bit; *steps_host counts the shared steps.  B = 1, w NULL or all ones and one constant beta return
 * gnode_meanfield_init_f64's outputs and step count bit for bit.  Host arguments are validated as there, plus B >= 1 and
 * 3 * B * n < 2^31; device arrays are not.  Synchronises `stream`.  A short workspace is GNODE_ERR_WORKSPACE with nothing
 * written. */
size_t gnode_meanfield_rates_workspace_bytes(gnode_graph_t g, int32_t B);
int gnode_meanfield_rates_f64(gnode_graph_t g, int32_t B, const double* init, const double* beta, const double* w,
                              const double* gamma, const double* t_out_host, int32_t n_out, double rtol, double atol,
                              double* outI, double* outS, double* outR, int64_t* steps_host, void* workspace,
                              size_t workspace_bytes, void* stream);
/* gnode_meanfield_rates_f64, and the record of its accepted steps: the same integration through the same code, so the outputs
 * and *steps_host are that entry's bit for bit, and gnode_meanfield_rates_workspace_bytes is its workspace too.
 *   h_host      host fp64 [h_cap]: the accepted step sizes in order; those past h_cap are dropped (h_host may be NULL with
 *               h_cap = 0: a first call that only counts)
 *   n_h_host    host: the number of accepted steps, whatever h_cap is
 *   n_acc_host  host int32 [n_out]: n_acc[to] accepted steps carried t_out[to - 1] to t_out[to]; n_acc[0] = 0, and an interval
 *               between equal output times has none
 * GNODE_ERR_ARG for a null n_h_host or n_acc_host, h_cap < 0, or h_host null with h_cap > 0; otherwise as that entry. */
int gnode_meanfield_rates_steps_f64(gnode_graph_t g, int32_t B, const double* init, const double* beta, const double* w,
                                    const double* gamma, const double* t_out_host, int32_t n_out, double rtol, double atol,
                                    double* outI, double* outS, double* outR, int64_t* steps_host, void* workspace,
                                    size_t workspace_bytes, void* stream, double* h_host, int64_t h_cap, int64_t* n_h_host,
                                    int32_t* n_acc_host);
/* The reverse sweep of that solve: the gradient of  sum(gI * outI) + sum(gS * outS) + sum(gR * outR)  with respect to the
 * start, beta, the contact weights and gamma, for B samples on one graph, fp64.  It is the exact derivative of the numbers
 * the forward returned WITH THE ACCEPTED STEP SIZES HELD FIXED (what backpropagating through an explicit Dormand-Prince loop
 * gives), not a second adaptive solve of the continuous adjoint: an accepted step is the 6-stage map
 *     Y_1 = y,  Y_s = y + h sum_{j<s} a_sj k_j,  k_s = f(Y_s),  y' = Y_7
 * (stage 7 feeds only the error estimate) and the sweep applies its transpose step by step, from the last output time down,
 * adding gI / gS / gR row `to` to the adjoint of y when it passes t_out[to] (rows at equal times both add).
 *   g, B, init, beta, w, gamma, t_out_host, n_out   the forward call's (beta and w may be NULL as there)
 *   h_host, n_h, n_acc_host   gnode_meanfield_rates_steps_f64's record, complete (n_h = its *n_h_host <= its h_cap)
 *   outI/outS/outR            what the forward returned, device fp64 [n_out][B * n]
 *   gI/gS/gR                  device fp64, the outputs' layout
 *   grad_init   device fp64 [B][n][3]      grad_beta, grad_gamma   device fp64 [B][n]
 *   grad_w      device fp64 [B][nnz], CSR position order: one row per sample, which the caller sums (w is shared)
 * A NULL gradient pointer means "not wanted"; the others' bits do not depend on it.  With beta or w NULL the gradient asked
 * for is the one at beta = 1, w = 1.  Per interval the entry integrates again from the forward's own output row with the
 * recorded steps and the forward's arithmetic, keeping y at every step (3 * B * n * 8 bytes each), then walks the steps
 * backwards: 5 launches recompute Y_2..Y_6 and 7 launches carry the adjoint through the six stages -- each completes one
 * stage's neighbour gather and does the next stage's row-local part, so there is one grid-wide dependency per stage.  No
 * atomics; every accumulator has one writer per launch and every row sum runs in ascending CSR position: two calls return
 * the same bits.  Enqueue-only: the host arrays are read before the call returns and `stream` is not synchronised.
 * gnode_meanfield_rates_backward_workspace_bytes(g, B, m) is the workspace for a record whose largest n_acc is m; it returns
 * 0 without a handle, for B < 1 and for m < 0.
 * GNODE_ERR_ARG, before any launch and with no gradient written: a null required pointer, all four gradient pointers null,
 * B < 1 or 3 * B * n >= 2^31, output times that do not start at 0 or ascend, an asymmetric pattern (also with w NULL: the
 * transpose gather needs every contact's reverse entry), a step list that the forward cannot have walked -- a step that is not
 * finite and > 0, counts that do not add up to n_h, an interval whose last step is not t_end - t bit for bit, an interval
 * of positive length without a step; the message names the interval.  GNODE_ERR_WORKSPACE: a short workspace.
 * n_out = 1 is valid: grad_init is row 0 of gS / gI / gR and the other gradients are 0. */
size_t gnode_meanfield_rates_backward_workspace_bytes(gnode_graph_t g, int32_t B, int32_t max_interval_steps);
int gnode_meanfield_rates_backward_f64(gnode_graph_t g, int32_t B, const double* init, const double* beta, const double* w,
                                       const double* gamma, const double* t_out_host, int32_t n_out, const double* h_host,
                                       int64_t n_h, const int32_t* n_acc_host, const double* outI, const double* outS,
                                       const double* outR, const double* gI, const double* gS, const double* gR,
                                       double* grad_init, double* grad_beta, double* grad_w, double* grad_gamma,
                                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- loss ------------------------------------------------------------------
 * The training loss of ode_nn_ngraph_sim.py:230-234 (multi-graph: ode_nn_ngraphs.py:199-203) and its gradient in one
 * pass: pred = cat(S, I, R)[rows, T, 3] against the labels y, t = 0 excluded,
 *     *loss_sum = sum_{row, t >= t0, c} |pred_c[t, row] - y[row, t, c]|        (float64; L1Loss's mean = sum / count)
 *     sgn[c, t, row] = sign(pred_c[t, row] - y[row, t, c]), 0 for t < t0       (= d loss_sum / d pred; may be NULL)
 *   S, I, R   device [T, rows] fp32 (gnode_forward_f32's outputs)
 *   y         device [rows, T, 3], fp32 or fp64 (y_is_f64); the difference is taken in y's type
 *   loss_sum  device double;  sgn: device [3, T, rows] fp32 or NULL
 *   workspace device, >= gnode_l1_loss_workspace_bytes()
 * Deterministic (fixed-order reduction), asynchronous on `stream`. */
size_t gnode_l1_loss_workspace_bytes(void);
int gnode_l1_loss_f32(const float* S, const float* I, const float* R, const void* y, int32_t y_is_f64, int64_t rows,
                      int32_t T, int32_t t0, double* loss_sum, float* sgn, void* workspace, size_t workspace_bytes,
                      void* stream);
/* The same with the signs already multiplied by `sign_scale` (e.g. 1 / element count: L1Loss's mean): sgn is then the loss
 * gradient with respect to the outputs as it stands, and no scaling launch follows. */
int gnode_l1_loss_scaled_f32(const float* S, const float* I, const float* R, const void* y, int32_t y_is_f64, int64_t rows,
                             int32_t T, int32_t t0, double* loss_sum, float* sgn, float sign_scale, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ---- instrumentation -------------------------------------------------------
 * While enabled, every launch of the two step kernels (0: gather + SIR update +
 * read-out, 1: node MLP) is bracketed by HIP events on the launch stream;
 * gnode_profile_read waits for them and returns summed milliseconds and launch
 * counts.  Used by bench.py's roofline leg; off by default (no overhead).
 * Process-wide and not thread-safe: switch it on around a single-threaded region. */
int gnode_profile_enable(int on);
int gnode_profile_read(double* gather_ms, int64_t* gather_launches, double* mlp_ms, int64_t* mlp_launches);
/* kind: 0 = Euler-step kernel, 1 = node-MLP kernel, 2 = backward interval kernel (H = 64), 3 = Monte-Carlo kernel;
 * one launch in 7 is sampled (the first of every 7 of its kind since gnode_profile_enable(1)). */
int gnode_profile_read_kind(int32_t kind, double* ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* GNODE_H */
