/*
 * raocp_hip.h — C-ABI of libraocp_hip.so, the MI355X (gfx950) implementation of
 * raocp's Chambolle–Pock inner loop.
 *
 * The reference (smokinmirror/raocp-toolbox) is pure Python and has no FFI; its
 * "operator API" is a set of Python methods. Each entry point below replaces one
 * of them and is what the drop-in Python layer (raocp-toolbox_amd/raocp/core,
 * via ctypes) binds. Citations are /root/reference paths.
 *
 * Conventions
 *  - All functions return 0 on success or a negative RAOCP_ERR_* code;
 *    raocp_last_error() returns the message of the last failure on this thread.
 *  - Vectors crossing the boundary are FLAT fp64 arrays in the reference's block
 *    order (np.vstack of the block lists built in cache.py:126-170), placeholders
 *    included: primal length raocp_sizes(..)[0], dual length [1].
 *  - Pointers are host pointers unless RAOCP_DEVICE_PTR is passed in `flags`,
 *    in which case they are device (HBM) pointers on the context's device.
 *  - A context is bound to one device and one HIP stream; it is not thread-safe
 *    (neither is the reference: shared cone instances, cache.py:180-182).
 *  - Matrix tables are row-major, one matrix after another; per-node int32
 *    index arrays select a table entry (the packer dedupes shared matrices).
 */
#ifndef RAOCP_HIP_H
#define RAOCP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RAOCP_OK 0
#define RAOCP_ERR_ARG -1          /* bad argument / shape (cache.py:84-122 shape errors) */
#define RAOCP_ERR_HIP -2          /* HIP runtime failure (no device, OOM, launch) */
#define RAOCP_ERR_TREE -3         /* tree violates a layout invariant (see raocp_tree_desc) */
#define RAOCP_ERR_NAN_IN_BOX -4   /* NaN reached a box projection (rectangle.py:50-59) */
#define RAOCP_ERR_STATE -5        /* call out of order (e.g. prox_f before an initial state) */

#define RAOCP_DEVICE_PTR 1

typedef struct raocp_ctx raocp_ctx;

/* Scenario tree (scenario_tree.py:21-154). Invariants checked at create:
 * nodes numbered so stage[] is non-decreasing, nonleaf nodes are 0..m-1, and the
 * children of node i are the contiguous ids ch_start[i] .. ch_start[i]+nch[i]-1
 * (true for every tree MarkovChainScenarioTreeFactory builds, scenario_tree.py:273-315). */
typedef struct {
    int32_t n;              /* num_nodes */
    int32_t m;              /* num_nonleaf_nodes */
    int32_t nx, nu;         /* state / control sizes */
    const int32_t* anc;     /* [n] ancestor, anc[0] = -1 */
    const int32_t* stage;   /* [n] stage of each node */
    const int32_t* ch_start;/* [m] first child */
    const int32_t* nch;     /* [m] number of children (>= 1) */
} raocp_tree_desc;

/* Problem data (raocp_spec.py, costs.py, risks.py, rectangle.py) and the offline
 * products of the dynamics projection (cache.py:207-233), computed by the host
 * packer (raocp/core/_pack.py). Index arrays are per node; -1 = not applicable. */
typedef struct {
    /* L / L^T weights (operators.py:19-94): sqrtm of Q, R (node j >= 1) and Pf (leaves) */
    int32_t n_sq, n_sr, n_sp;
    const double* sqrt_q;   /* [n_sq][nx][nx] */
    const double* sqrt_r;   /* [n_sr][nu][nu] */
    const double* sqrt_pf;  /* [n_sp][nx][nx] */
    const int32_t* i_sq;    /* [n] */
    const int32_t* i_sr;    /* [n] */
    const int32_t* i_sp;    /* [n] */
    /* AVaR (risks.py:28-35): b_i = [p; 0; 1]; p_k stored at child ch_start[i]+k */
    const double* alpha_r;  /* [m] risk parameter alpha of node i */
    const double* cond;     /* [n] conditional probability of node j given its parent */
    /* boxes (rectangle.py): nonleaf rows nx+nu, leaf rows nx */
    int32_t n_box_nl, n_box_l;
    const double* box_nl_lo; const double* box_nl_hi;   /* [n_box_nl][nx+nu] */
    const double* box_l_lo;  const double* box_l_hi;    /* [n_box_l][nx] */
    const int32_t* i_box_nl;/* [m] -1 = No constraint */
    const int32_t* i_box_l; /* [n] (leaves used) -1 = No constraint */
    /* dynamics projection: per-mode A, B (state / control dynamics of node j) and,
     * per subtree class (classes numbered by stage), the offline products
     * K, Rinv = (I + sum_j B_j'P_j B_j)^-1 and M = K' + sum_j Abar_j' P_j B_j */
    int32_t n_a, n_b, n_k;
    const double* A;        /* [n_a][nx][nx] */
    const double* B;        /* [n_b][nx][nu] */
    const double* K;        /* [n_k][nu][nx] */
    const double* Rinv;     /* [n_k][nu][nu] */
    const double* M;        /* [n_k][nx][nu] */
    const int32_t* i_a;     /* [n] */
    const int32_t* i_b;     /* [n] */
    const int32_t* i_k;     /* [m] class of nonleaf node i */
    /* arithmetic of the context: RAOCP_F64 (the reference's) or RAOCP_F32 (BASELINE
     * configs[4]: iterate, tables and products in fp32; vectors still cross the host
     * boundary as fp64 arrays, device pointers (RAOCP_DEVICE_PTR) are then float*) */
    int32_t dtype;
} raocp_problem_desc;

#define RAOCP_F64 0
#define RAOCP_F32 1

/* Create a context on HIP device `device`: validates the tree, uploads all tables
 * to HBM, allocates the iterate and work buffers. Replaces Cache.__init__
 * (cache.py:13-52) + Operator.__init__ (operators.py:10-17). */
int raocp_ctx_create(const raocp_tree_desc* tree, const raocp_problem_desc* prob, int device,
                     raocp_ctx** out);
void raocp_ctx_destroy(raocp_ctx* ctx);
const char* raocp_last_error(void);
/* hipDeviceSynchronize on `device` through this library's HIP runtime (bench.py
 * brackets its timed region with it; see bench.py for why not torch.cuda). */
int raocp_device_synchronize(int device);

/* Flat primal / dual lengths (placeholders included), cache.py:126-170. */
int raocp_sizes(raocp_ctx* ctx, int64_t* primal_size, int64_t* dual_size);

/* eta <- L z (Operator.ell, operators.py:19-53 / linop_ell 96-107). Only slots L
 * writes are stored; every other slot of `eta` keeps its input value, exactly like
 * the reference's output template. */
int raocp_ell(raocp_ctx* ctx, const double* z, double* eta, int flags);
/* z <- L^T eta (Operator.ell_transpose, operators.py:55-94 / linop_ell_transpose
 * 109-120). tau_0 keeps its input value. */
int raocp_ell_t(raocp_ctx* ctx, const double* eta, double* z, int flags);

/* The context's current iterate (Cache.__primal / __dual, cache.py:84-122). */
int raocp_set_primal(raocp_ctx* ctx, const double* z, int flags);
int raocp_get_primal(raocp_ctx* ctx, double* z, int flags);
int raocp_set_dual(raocp_ctx* ctx, const double* eta, int flags);
int raocp_get_dual(raocp_ctx* ctx, double* eta, int flags);
/* Cache.cache_initial_state (cache.py:79-82): x0 has nx entries. */
int raocp_set_initial_state(raocp_ctx* ctx, const double* x0);
/* Zero the current primal and dual on the device: the iterate of a fresh Cache
 * (cache.py:126-170 zero templates), without a host upload (cold-started chock). */
int raocp_reset_iterate(raocp_ctx* ctx);
/* Name of the kernel the context's default selection launches for `op` (raocp_op_bench
 * numbering: 0 L, 1 L^T, 2 dual CP kernel, 6 primal CP kernel, 9 dynamics projection,
 * 10 fused CP iteration, 11 the CP loop's one launch of dynamics projection + CP iteration
 * (k_drc; "" when the loop runs 9 and 10 as separate launches)), as rocprofv3 reports it;
 * op 12: the forms of the k_cp5 launches ("leaf_pf=. fams=. fam_pf=.", "" when k_cp5 does not
 * run); op 13: the batched CP kernel of raocp_cp_batch_run ("" when the batch runs as
 * sequential solves); op 14: the step kernel of raocp_cp_batch_mpc ("" when that loop runs on
 * the host); ops 13 and 14 name a kernel on contexts of either precision: "k_cpb<true>" /
 * "k_cpb<false>" and "k_mpc_step" on an fp64 context (the names the fp64 forms have always
 * reported), "k_cpb<float, true>" / "k_cpb<float, false>" and "k_mpc_step<float>" on an fp32
 * one that runs with RAOCP_CPB_F32=1 (the bool: the shared tables are staged in LDS; without
 * that switch an fp32 context reports "" for both, as it always has); op 15: the composed maps active in the regular-tree sweep (k_dr / k_drc), as
 * space-separated "name@tier" terms: "mid_back_root@k" = tier k (between the top and the
 * deepest) publishes its root's q row from one composed product before its backward levels;
 * "" when none is (RAOCP_DR_XFER=0, a plan with no such tier or with a tier of more than 4
 * levels, another sweep); op 16: the composed forward maps active in that sweep, in the same
 * form: "mid_fwd@k" / "deep_fwd@k" = tier k (between the top and the deepest / the deepest)
 * runs its forward levels from a zero root x row while it waits for that row and adds the
 * composed map's product with the row once it has landed; "" when none is (RAOCP_DR_XFER=0,
 * RAOCP_DR_FWD=0, a one-tier plan or one with a tier of more than 4 levels, another sweep);
 * op 17: the kernels of raocp_evaluate, "k_eval_nodes<double> + k_eval_sweep<double> xS" with S
 * the number of sweep launches ("<float>" on an fp32 context); op 18: the kernel of
 * raocp_cp_batch_evaluate, "k_eval_batch<double>" / "k_eval_batch<float>", or "" when the batch
 * evaluation runs the kernels of op 17 over each stored primal (after a batch: by how that batch
 * ran; before any: by how one would run now, as op 13 reports it); op 19: the kernel of
 * raocp_cp_batch_run_aa, "k_cpa<true>" / "k_cpa<false>" (the shared tables staged in LDS or
 * not), or "" on a context that call refuses (fp32, sharded, or one k_cpb does not cover);
 * op 20: the step kernel of raocp_cp_batch_mpc_aa, "k_mpc_step_aa", or "" on a context that call
 * refuses (the contexts of op 19);
 * written NUL-terminated to buf. */
int raocp_kernel_info(raocp_ctx* ctx, int op, char* buf, int cap);

/* prox of f on the current primal (Cache.proximal_of_f, cache.py:248-257) and its steps */
int raocp_prox_f(raocp_ctx* ctx, double alpha);
int raocp_relax_s0(raocp_ctx* ctx, double alpha);        /* cache.py:253-257 */
int raocp_project_on_dynamics(raocp_ctx* ctx);           /* cache.py:259-288 */
int raocp_project_on_kernel(raocp_ctx* ctx);             /* cache.py:290-317 */
/* prox of alpha g* on the current dual (Cache.proximal_of_g_conjugate, cache.py:321-393) */
int raocp_prox_gconj(raocp_ctx* ctx, double alpha);

/* Sub-steps of prox_g* on the current dual, for the Cache API (cache.py:329-393):
 * modify_dual (eta /= alpha over every slot), add_halves (-1/2 on eta5, eta12 and
 * +1/2 on eta6, eta13, all blocks incl. placeholders), the cone/box projections
 * (which: 1 = project_on_constraints_nonleaf, 2 = _leaf, 3 = both) and
 * modify_projection (eta <- alpha (modified - eta), `modified` a host flat dual). */
int raocp_dual_scale(raocp_ctx* ctx, double alpha);
int raocp_dual_add_halves(raocp_ctx* ctx);
int raocp_dual_project(raocp_ctx* ctx, int which);
int raocp_dual_moreau(raocp_ctx* ctx, double alpha, const double* modified);

/* lambda_max(L'L) by device Lanczos (replaces ARPACK eigs, solver.py:104-118).
 * alpha = 0.999 / lambda_max. */
int raocp_step_size(raocp_ctx* ctx, double* lambda_max, int max_it, double rtol);

/* The whole Chambolle–Pock loop (Solver.chock, solver.py:97-171) on the device.
 * Starts from the context's current primal / dual (raocp_set_primal / raocp_set_dual;
 * both zero after raocp_ctx_create) with x0 written into node 0's state, as the
 * reference's chock continues from the cache's old primal / dual (solver.py:27-61,
 * cache.py:79-82, 186-196); runs until
 * k >= max_iters or max(error) <= tol, like the reference. Outputs:
 *   status    0 converged (k < max_iters) / 1 not converged (solver.py:166-169)
 *   iters     number of iterations run (rows of the error caches)
 *   err_hist, delta_hist: [max_iters+1][3] host arrays (row k = iteration k)
 * The final iterate is left as the context's current primal/dual. */
int raocp_cp_run(raocp_ctx* ctx, const double* x0, int max_iters, double tol, double alpha,
                 int* status, int* iters, double* err_hist, double* delta_hist);

/* Batched Chambolle–Pock solves: B instances of the context's problem that share the tree,
 * the tables and alpha and differ in x0 (and, when z0 / eta0 are given, in the starting
 * iterate; both NULL: every instance starts from zero). Each instance runs Solver.chock's loop
 * (solver.py:97-171) with its own stopping test. One launch runs one workgroup per instance
 * (k_cpb, raocp_cpb.hip; chunks of RAOCP_BATCH_CHUNK iterations, default 256, until every
 * instance is done) in the context's precision. An fp64 context takes the kernel by default;
 * an fp32 context takes its float form when the environment has RAOCP_CPB_F32=1 (read at call
 * time; unset, an fp32 context behaves as it always has and runs the sequential solves). On
 * an fp32 context the slabs, the tables and the arithmetic of a row are float (the residual
 * maxima are widened to double for the history rows and the stopping test, as raocp_cp_run
 * does there), and x0, z0, eta0 and the getters below cross the host boundary as fp64 arrays,
 * converted as the single-solve entry points convert. A context the kernel does not cover
 * (nx > 32 or nu > 16, RAOCP_CPB=0, fp32 without RAOCP_CPB_F32=1) runs the B solves one after
 * another through raocp_cp_run, with the same results (fp32: the same up to the rounding of
 * another summation order). Outputs per instance b:
 *   status[b]  0 converged / 1 not converged / 2 a NaN reached a box projection (that
 *              instance stopped there; the others are not affected)
 *   iters[b]   rows of its error caches
 *   err_hist, delta_hist: [B][max_iters+1][3] host arrays
 * The context's own iterate (raocp_get_primal / raocp_get_dual) and initial state are left
 * as they were. Errors: RAOCP_ERR_ARG for B < 1, B > 4096, a NULL pointer or z0 without eta0;
 * RAOCP_ERR_STATE on a sharded context. kernel_info op 13 names the kernel ("" when the
 * sequential solves run). */
int raocp_cp_batch_run(raocp_ctx* ctx, int B, const double* x0 /*[B][nx]*/,
                       const double* z0 /*[B][P] or NULL*/, const double* eta0 /*[B][D] or NULL*/,
                       int max_iters, double tol, double alpha,
                       int* status /*[B]*/, int* iters /*[B]*/,
                       double* err_hist /*[B][max_iters+1][3]*/, double* delta_hist);
/* raocp_cp_batch_run with Anderson acceleration of memory accel = m, 1 <= m <= 8 (kernel k_cpa,
 * one workgroup per instance). With v = (z, eta), g_k = T(v_k) one CP iteration
 * and r_k = g_k - v_k: the last m difference columns dG, dR of the pairs (g_k, r_k) are kept;
 * after iteration k with (k + 1) % accel_every == 0 and at least one column,
 * gamma = (dR'dR + accel_reg (tr / j) I)^-1 dR'r_k by Cholesky in double and the next iterate is
 * the proposal g_k - dG gamma. The iteration after it is the trial: accepted when
 * |T(v^) - v^|_2 <= accel_safeguard |r_k|_2, else the history is cleared and the solve goes on
 * from g_k. A non-positive pivot or a non-finite gamma clears the history (no proposal). Every
 * iteration, trials included, writes its history row and counts against max_iters; a rejected
 * trial never ends the solve through tol. Inputs, outputs and the follow-up calls
 * (raocp_cp_batch_get, _first_inputs, _evaluate) are those of raocp_cp_batch_run; z0 / eta0
 * start with an empty history. Errors: as raocp_cp_batch_run, RAOCP_ERR_ARG for accel outside
 * 1 .. 8, accel_every < 1 or a negative accel_reg / accel_safeguard, RAOCP_ERR_STATE on an fp32
 * context, a sharded one or one k_cpb does not cover (there is no sequential form). kernel_info
 * op 19 names the kernel. */
int raocp_cp_batch_run_aa(raocp_ctx* ctx, int B, const double* x0, const double* z0, const double* eta0,
                          int max_iters, double tol, double alpha, int accel, int accel_every, double accel_reg,
                          double accel_safeguard, int* status, int* iters, double* err_hist, double* delta_hist);
/* The acceleration's log of instance b of the last raocp_cp_batch_run_aa (or of instance b's last
 * solve of the last raocp_cp_batch_mpc_aa, iters[b] then being that solve's): iters[b] records of 12
 * doubles, one per history row: code (0 plain, 1 proposal made, 2 trial accepted, 3 trial
 * rejected, 4 solve refused), j (columns when the solve ran, else after the push), prop (what
 * followed in this iteration: 0 nothing, 1 a proposal, 2 a refused solve; it tells what an
 * accepted trial, code 2, went on to do), |r_k|_2, gamma[8] (column order, oldest first, zero
 * beyond j). RAOCP_ERR_STATE when the last batch was not accelerated. */
int raocp_cp_batch_aa_log(raocp_ctx* ctx, int b, double* out /*[iters[b]][12]*/);
/* The final primal / dual of instance b of the last batch, in the reference's flat order. */
int raocp_cp_batch_get(raocp_ctx* ctx, int b, double* z /*[P]*/, double* eta /*[D]*/);
/* The pair (z, eta) that instance b's last iteration was computed from (the final iterate is one
 * CP iteration of it, and the last history row is that iteration's): after a batch a kernel ran
 * (k_cpb, k_cpa); RAOCP_ERR_STATE after the sequential solves, which do not keep it. */
int raocp_cp_batch_get_prev(raocp_ctx* ctx, int b, double* z /*[P]*/, double* eta /*[D]*/);
/* The root's input u_0 of every instance's final primal (what an MPC loop applies). */
int raocp_cp_batch_first_inputs(raocp_ctx* ctx, double* u0 /*[B][nu]*/);

/* Closed-loop MPC simulation of a batch, resident on the device: T steps of B instances. Step t
 * solves every instance from its current state (raocp_cp_batch_run's solve, with its own
 * stopping test), applies the root's input u_0 of the final primal and moves the plant along
 * the realised scenario j = scen[b][t], an index into the root's children (node
 * i = ch_start[0] + j): x+ = A_i x + B_i u_0 with the dynamics the context was created with,
 * realised stage cost |sqrtQ_i x|^2 + |sqrtR_i u_0|^2. The next solve starts from x+ and, with
 * warm != 0, from this step's final iterate (warm = 0: from zero). One kernel launch per step
 * (k_mpc_step, raocp_cpb.hip) records the step and restarts the instances inside their slabs;
 * besides the done poll of the k_cpb launches nothing crosses the host boundary inside the
 * loop. On an fp32 context the plant step and the stage cost are computed in float (the
 * root-children table A_i | B_i is held in float) and recorded as doubles. A context k_cpb does
 * not cover (see raocp_cp_batch_run) runs the same loop on the host over sequential solves, with
 * the same outputs. Outputs (fp64 arrays and ints on a context of either precision):
 *   X[b][t]       the state step t was solved from (X[b][0] = x0[b]), X[b][T] the last x+
 *   U[b][t]       the input applied, cost[b][t] the realised stage cost
 *   status[b][t]  0 / 1 / 2 and iters[b][t] as raocp_cp_batch_run, err[b][t][0..2] the last row
 *                 of that solve's error cache
 * An instance whose solve let a NaN reach a box projection is frozen: that step records status 2
 * and its iterations, every later step status 2 and 0 iterations (err NaN); U, cost and the
 * following X are NaN from that step on; the other instances are not affected.
 * Afterwards raocp_cp_batch_get / raocp_cp_batch_first_inputs describe every instance's last
 * solve. The context's own iterate and initial state are left as they were. Errors:
 * RAOCP_ERR_ARG for a NULL pointer, B outside 1 .. 4096, T < 1, max_iters < 0 or a scen entry
 * outside [0, nch[0]) (checked before anything is launched); RAOCP_ERR_STATE on a sharded
 * context. kernel_info op 14 names the step kernel ("" when the loop runs on the host). */
int raocp_cp_batch_mpc(raocp_ctx* ctx, int B, int T, const double* x0 /*[B][nx]*/, const int* scen /*[B][T]*/,
                       int max_iters, double tol, double alpha, int warm,
                       double* X /*[B][T+1][nx]*/, double* U /*[B][T][nu]*/, double* cost /*[B][T]*/,
                       int* status /*[B][T]*/, int* iters /*[B][T]*/, double* err /*[B][T][3]*/);
/* raocp_cp_batch_mpc with every step of every instance solved by raocp_cp_batch_run_aa's kernel
 * (k_cpa; accel = m in 1 .. 8 and accel_every, accel_reg, accel_safeguard as there). Every step
 * starts with an empty acceleration history (no columns, no previous pair, no pending trial)
 * whatever warm is: a new x0 is a new fixed-point map; warm != 0 still carries the iterate over.
 * One launch per step (k_mpc_step_aa) does what k_mpc_step does, reduces the log of the solve that
 * has just ended to aa_counts[b][t][0..3] = proposals made, trials accepted, trials rejected,
 * solves refused (log records with prop == 1, code == 2, code == 3, prop == 2) and clears the
 * instance's acceleration state for the next step; no log is downloaded inside the loop. The
 * counts of a step a frozen instance did not solve are zero; the step that froze it has the
 * counts of that solve. The other outputs, the freezing rule and the follow-up calls are those of
 * raocp_cp_batch_mpc; raocp_cp_batch_aa_log then serves every instance's last solve. Errors: those
 * of raocp_cp_batch_mpc (aa_counts NULL included), then those of raocp_cp_batch_run_aa:
 * RAOCP_ERR_ARG for accel outside 1 .. 8, accel_every < 1 or a negative accel_reg /
 * accel_safeguard, RAOCP_ERR_STATE on an fp32 context or one k_cpb does not cover (there is no
 * sequential form and no fp32 form). kernel_info op 20 names the step kernel. */
int raocp_cp_batch_mpc_aa(raocp_ctx* ctx, int B, int T, const double* x0 /*[B][nx]*/, const int* scen /*[B][T]*/,
                          int max_iters, double tol, double alpha, int warm, int accel, int accel_every,
                          double accel_reg, double accel_safeguard,
                          double* X /*[B][T+1][nx]*/, double* U /*[B][T][nu]*/, double* cost /*[B][T]*/,
                          int* status /*[B][T]*/, int* iters /*[B][T]*/, double* err /*[B][T][3]*/,
                          int* aa_counts /*[B][T][4]*/);

/* Evaluate a primal: the risk-averse cost of its policy and how far it is from feasible
 * (raocp_eval.hip). With l_j = |sqrtQ_j x_anc(j)|^2 + |sqrtR_j u_anc(j)|^2 the stage cost of
 * node j >= 1 and V_l = |sqrtPf_l x_l|^2 the terminal cost of leaf l, the cost-to-go of a
 * nonleaf node is V_i = AVaR_{alpha_i, cond}((l_j + V_j) over the children j of i), the maximum
 * of mu'Z over {alpha mu <= p, mu >= 0, 1'mu = 1} (risks.py:28-35; alpha = 0 the plain maximum,
 * alpha = 1 the expectation). out[]:
 *   RAOCP_EVAL_COST  V_0
 *   RAOCP_EVAL_S0    the primal's own epigraph variable s_0 (equals V_0 only at convergence)
 *   RAOCP_EVAL_BOX   the largest max(lo - w, w - hi, 0) over every active box (nonleaf rows
 *                    w = [x_i; u_i], leaf rows w = x_l); 0 without boxes, infinite bounds never
 *                    violate
 *   RAOCP_EVAL_DYN   max(|x_0 - x0|_inf, max_j |x_j - A_j x_anc(j) - B_j u_anc(j)|_inf), x0 the
 *                    initial state of raocp_set_initial_state / the last raocp_cp_run
 * A NaN in the primal surfaces: the maxima keep it and the cost becomes NaN. Values are loaded
 * in the context's scalar type; all arithmetic is double on a context of either precision.
 * z NULL: the context's current primal; else a flat primal (host, or device with
 * RAOCP_DEVICE_PTR in `flags`: double* on an fp64 context, float* on an fp32 one).
 * node_values NULL or a host array [n]: V_i of every node (leaves: the terminal cost).
 * Nothing of the context changes (iterate, initial state, batch slabs, captured graphs).
 * Errors: RAOCP_ERR_ARG for a NULL out; RAOCP_ERR_STATE without an initial state or on a
 * sharded context. kernel_info op 17 names the kernels. */
#define RAOCP_EVAL_COST 0
#define RAOCP_EVAL_S0   1
#define RAOCP_EVAL_BOX  2
#define RAOCP_EVAL_DYN  3
#define RAOCP_EVAL_N    4
int raocp_evaluate(raocp_ctx* ctx, const double* z, int flags, double* out /*[RAOCP_EVAL_N]*/,
                   double* node_values /*[n] or NULL*/);
/* The same four values for the final primal of every instance of the last raocp_cp_batch_run /
 * raocp_cp_batch_mpc, x0 being the state the instance's last solve was solved from. One launch,
 * one workgroup per instance (k_eval_batch) when k_cpb ran the batch; the kernels of
 * raocp_evaluate over each stored primal when it ran as sequential solves, with the same
 * values. Errors: RAOCP_ERR_ARG for a NULL out; RAOCP_ERR_STATE before any batch or on a
 * sharded context. kernel_info op 18 names the kernel. */
int raocp_cp_batch_evaluate(raocp_ctx* ctx, double* out /*[B][RAOCP_EVAL_N]*/);

/* Benchmark helpers (bench.py): raocp_cp_bench runs exactly `iters` CP iterations
 * (tol = 0) from (x0 at node 0, zeros) / 0 on the device, graph-replayed (whole
 * batches of 24 iterations, then one remainder batch), without host syncs inside;
 * returns device ms. raocp_cp_prepare captures the graphs a run of `iters` iterations
 * uses and, given x0, also resets the iterate for it, so that a following
 * raocp_cp_bench(ctx, NULL, iters, alpha, &ms) only launches the iterations. */
int raocp_cp_prepare(raocp_ctx* ctx, const double* x0, int iters, double alpha);
int raocp_cp_bench(raocp_ctx* ctx, const double* x0, int iters, double alpha, float* ms);
/* Time `reps` back-to-back launches of L (op=0) or L^T (op=1) on device-resident
 * vectors with HIP events on the context's stream; returns average ms per launch.
 * op=17: the launches of one raocp_evaluate on the context's current primal (k_eval_nodes and
 * the sweep), reps evaluations between the two events; needs an initial state and leaves the
 * context as it was. */
int raocp_op_bench(raocp_ctx* ctx, int op, int reps, float* ms_per_launch);
/* The same for L (op 0) / L^T (op 1) with the launches cycling over `nsets` (<= 16) freshly
 * allocated input / output buffer pairs, so that a working set beyond the 256 MiB Infinity
 * Cache is read from HBM on every launch. */
int raocp_op_bench_rot(raocp_ctx* ctx, int op, int reps, int nsets, float* ms_per_launch);
/* Diagnostics: one dynamics projection with in-kernel s_memrealtime stamps (100 MHz). */
int raocp_debug_dyn_stamps(raocp_ctx* ctx, unsigned long long* stamps, int cap);

/* Subtree sharding across GPUs (north_star "scenarios shard naturally
 * by subtree"). Shard `rank` of `nranks` owns a contiguous block of the subtrees rooted
 * at the boundary stage of the replicated top of the tree; the CP iteration then runs on
 * the owned nodes only, with two all-gathers per iteration: the q rows of the roots
 * (dynamics backward sweep), and the roots' eta2 / xi2 entries together with the previous
 * iteration's residual record (the stopping test runs one iteration late, so the residual
 * reduction needs no collective of its own).
 * raocp_shard_setup restricts this context to its shard; raocp_comm_init binds an RCCL
 * communicator (one process per GPU; the 128-byte id comes from raocp_comm_unique_id on
 * one rank); raocp_cp_run / raocp_cp_bench then run the sharded iteration.
 * raocp_group_cp_run runs the shards of one process (tests: shards sharing a device),
 * exchanging through device copies; raocp_group_cp_run_warm is the same loop with a warm flag
 * (warm != 0: every shard continues from its own current primal / dual, as raocp_cp_run does;
 * raocp_group_cp_run is the cold start, warm = 0). raocp_shard_owned: owned id range per stage. */
int raocp_shard_setup(raocp_ctx* ctx, int nranks, int rank);
int raocp_shard_owned(raocp_ctx* ctx, int32_t* stage_lo, int32_t* stage_hi, int cap);
int raocp_comm_unique_id(unsigned char* id128);
int raocp_comm_init(raocp_ctx* ctx, const unsigned char* id128, int nranks, int rank);
int raocp_group_cp_run(raocp_ctx** ctxs, int nranks, const double* x0, int max_iters, double tol, double alpha,
                       int* status, int* iters, double* err_hist, double* delta_hist);
int raocp_group_cp_run_warm(raocp_ctx** ctxs, int nranks, const double* x0, int max_iters, double tol, double alpha,
                            int warm, int* status, int* iters, double* err_hist, double* delta_hist);

#ifdef __cplusplus
}
#endif
#endif /* RAOCP_HIP_H */
