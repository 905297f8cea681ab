/*
 * daqp_amd.h -- C ABI of the MI355X-native batched dual active-set QP path.
 *
 *   minimize   1/2 x'Hx + f'x      subject to   blower <= [x(1:ms); A x] <= bupper
 *
 * Two layers, both exported by libdaqp_amd.so (plain pointers and sizes only):
 *
 *  (1) The single-problem entry points of DAQP v0.9.1, same names, argument
 *      meaning, struct layouts and exit flags, so that a binding written against
 *      the reference's api.h links against this library unchanged.  Each call
 *      is a batch of one on the GPU.
 *        reference include/api.h:29-30   daqp_solve, daqp_quadprog
 *        reference include/api.h:33-34   setup_daqp, setup_daqp_main
 *        reference include/utils.h:11    daqp_update_ldp
 *        reference include/api.h:40-52   allocate_/free_ helpers, daqp_default_settings
 *        reference include/api.h:56-58   daqp_primal_init_active, daqp_dual_init_active
 *        reference include/api.h:35,54, include/daqp.h:12-13   setup_daqp_ldp, daqp_extract_result, daqp_ldp, ldp2qp_solution
 *
 *  (2) The additive batch entry points (daqp_batch_* / daqp_quadprog_batch):
 *      N independent problems of one shape (n, m, ms), stored back to back,
 *      solved by one wavefront each with the working set and LDL' factors in LDS.
 *
 * Only the hot path is implemented: dense convex H (a singular one, and an LP
 * with H == NULL, go through the reference's proximal outer loop, daqp_prox.c);
 * sense bits ACTIVE/LOWER/IMMUTABLE/SOFT.  Solutions are differentiable (daqp_batch_backward, daqp_batch_backward_soft; problems
 * that went through the proximal loop, n <= 64: daqp_batch_backward_nullspace).  Binary constraints, hierarchies and AVIs
 * (the reference's bnb/hiqp/avi loops) return DAQP_EXIT_UNSUPPORTED.  There is NO CPU fallback: without a HIP device every
 * entry point fails with DAQP_EXIT_UNSUPPORTED and daqp_amd_last_error() says why.
 */
#ifndef DAQP_AMD_H
#define DAQP_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

typedef double c_float; /* the path computes in fp64 only (reference types.h:8-12 default) */

/* ---- exit flags (reference include/constants.h:42-51) ---- */
#define DAQP_EXIT_SOFT_OPTIMAL 2
#define DAQP_EXIT_OPTIMAL 1
#define DAQP_EXIT_INFEASIBLE -1
#define DAQP_EXIT_CYCLE -2
#define DAQP_EXIT_UNBOUNDED -3
#define DAQP_EXIT_ITERLIMIT -4
#define DAQP_EXIT_NONCONVEX -5
#define DAQP_EXIT_OVERDETERMINED_INITIAL -6
#define DAQP_EXIT_TIMELIMIT -7
#define DAQP_EXIT_UNSUPPORTED -8
/* per-problem status of daqp_batch_backward / daqp_batch_backward_soft only (never an exit flag of a solve): the Gram matrix of the active rows is numerically
   singular (a pivot of its Cholesky factor below settings->zero_tol) -- linearly dependent active constraints, no unique adjoint.
   daqp_batch_backward_nullspace reports it for the same reason (R_jj^2 < zero_tol in the QR of the unit active rows) and when H is
   not positive definite on the null space of the active rows (a pivot of Z'HZ <= zero_tol max(1, max_i H_ii)) */
#define DAQP_BACKWARD_SINGULAR -20

/* ---- daqp_update_ldp masks (reference include/constants.h:54-61) ---- */
#define DAQP_UPDATE_Rinv 1
#define DAQP_UPDATE_M 2
#define DAQP_UPDATE_v 4
#define DAQP_UPDATE_d 8
#define DAQP_UPDATE_sense 16
#define DAQP_UPDATE_hierarchy 32
#define DAQP_UPDATE_unconstrained 64
#define DAQP_UPDATE_eliminate 128

/* ---- constraint sense bits (reference include/constants.h:64-96) ---- */
#define DAQP_ACTIVE 1
#define DAQP_LOWER 2
#define DAQP_IMMUTABLE 4
#define DAQP_SOFT 8
#define DAQP_BINARY 16

#define DAQP_EMPTY_IND -1
#define DAQP_UNCONSTRAINED_OPTIMAL -2
#define DAQP_INF ((c_float)1e30)

/* Problem descriptor: layout of reference include/types.h:14-50 (80 bytes). */
typedef struct {
    int n, m, ms;            /* variables, constraints (simple first), simple bounds */
    c_float *H;              /* n x n, row-major */
    c_float *f;              /* n */
    c_float *A;              /* (m-ms) x n, row-major */
    c_float *bupper, *blower; /* m each: [simple; general] */
    int *sense;              /* m, or NULL (= all 0) */
    int *break_points;       /* must be NULL (hierarchies unsupported) */
    int nh;                  /* 0 or 1 */
    int problem_type;        /* must be 0 */
} DAQPProblem;

/* Settings: layout of reference include/types.h:52-74 (120 bytes). */
typedef struct {
    c_float primal_tol, dual_tol, zero_tol, pivot_tol, progress_tol;
    int cycle_tol, iter_limit;
    c_float fval_bound;         /* the dual-objective stop (daqp.c:10,20): at every dual-feasible iterate the least-distance problem's
                                   1/2 (|u|^2 + soft slack) -- the fval this library reports plus 1/2 f'H^-1 f -- is compared with fval_bound,
                                   and the first iterate where it is strictly greater ends the solve with DAQP_EXIT_INFEASIBLE (-1): the
                                   optimal value cannot be below that (weak duality).  At this exit, as in the reference (api.c:27 skips
                                   ldp2qp_solution): fval is the dual value of that iterate, a lower bound of the optimum; lam holds its
                                   multipliers in the least-distance problem's units (row k of the QP: lam_k / sqrt(c_k H^-1 c_k')), zero
                                   off the working set; soft_slack belongs to the same iterate; x is the iterate in the least-distance
                                   problem's coordinates, not a point of the QP, and iter counts up to the stop.  A later daqp_solve /
                                   daqp_batch_solve with a larger bound continues from the kept working set.  On a cold default-mode
                                   batch solve the problems stopped this way report -1 and so take the second pass in the exact
                                   arithmetic with the others of that verdict (daqp_batch_rechecked counts them; see below), under
                                   the same bound: their outputs are the exact mode's.  Inside the proximal loop (singular H, LPs) the
                                   bound applies to each inner least-distance problem.  DAQP_INF: off. */
    c_float eps_prox, eta_prox; /* shift / stationarity tolerance of the proximal loop (singular H); < 0: automatic */
    c_float rho_soft;
    c_float rel_subopt, abs_subopt;
    c_float sing_tol, refactor_tol;
    c_float time_limit;         /* seconds, 0 = none: checked every 32nd iteration on the device clock, per problem
                                   from the start of its solve (daqp.c:95-103) -> DAQP_EXIT_TIMELIMIT */
} DAQPSettings;

/* Result: layout of reference include/api.h:15-27 (64 bytes). x and lam are caller-owned. */
typedef struct {
    c_float *x, *lam;
    c_float fval, soft_slack;
    int exitflag, iter, nodes;
    c_float solve_time, setup_time;
} DAQPResult;

/* Workspace: field order and offsets of reference include/types.h:187-264
 * (288 bytes), so that sizeof/offsetof match for bindings that mirror it.
 * In this implementation the numerical state lives on the GPU: the array
 * members below are HOST MIRRORS refreshed by setup/solve (NULL where no
 * mirror is kept); `timer` carries the opaque device handle. */
typedef struct DAQPWorkspace {
    DAQPProblem *qp;
    int n, m, ms;
    c_float *M, *dupper, *dlower, *Rinv, *v;   /* READ-ONLY host mirrors of the device-resident LDP (refreshed by setup / update_ldp;
                                                  layouts of the reference: M (m-ms) x n row-major, Rinv packed upper; Rinv is NULL
                                                  for a diagonal H (then RinvD) and for an LP) */
    int *sense;                                /* host mirror, m */
    c_float *scaling, *RinvD;                  /* host mirrors (see above) */
    c_float *x, *xold;                         /* x: host mirror of the last primal solution */
    c_float *lam, *lam_star, *u;               /* lam_star: host mirror (n_active multipliers) */
    c_float fval;
    c_float *L, *D, *xldl, *zldl;              /* NULL */
    int reuse_ind;
    int *WS;                                   /* host mirror of the working set */
    int n_active, iterations, sing_ind;
    int *prox_mask;                            /* NULL */
    int n_prox;                                /* > 0: H was shifted, daqp_solve runs the proximal loop (host mirror) */
    c_float soft_slack;
    DAQPSettings *settings;
    void *bnb;                                 /* NULL */
    int nh;
    int *break_points;
    void *avi, *eq;                            /* NULL */
    void *timer;                               /* opaque: DAQPBatch* of size 1 */
    c_float *Mu;                               /* NULL */
} DAQPWorkspace;

/* ------------------------------------------------------------------ */
/* (1) single-problem drop-in entry points                             */
/* ------------------------------------------------------------------ */
/* LATENCY: each of these is a batch of ONE on the GPU -- two kernels and mapped result slabs: daqp_quadprog 0.13 ms (n = 20, m = 40) to
   0.25 ms (n = 50, m = 150), daqp_update_ldp(UPDATE_v) + daqp_solve on a kept workspace 0.05-0.06 ms (profiles/r05zzzz_latency_one.txt), where
   the reference needs ~0.02 ms on one core for a small problem.
   STALE MIRRORS: daqp_update_ldp(UPDATE_v | UPDATE_d) on a kept workspace is checked on the host and applied by the NEXT daqp_solve's launch; until
   that solve returns, work->v, work->dupper and work->dlower (read-only host copies for bindings that look at them) still hold the previous LDP.  They exist so that bindings written against the reference's api.h
   link and behave; a caller that loops over many QPs of one shape should hand them over at once: section (2), daqp_quadprog_batch. */
void daqp_quadprog(DAQPResult *res, DAQPProblem *qp, DAQPSettings *settings); /* api.c:62-79 */
void daqp_solve(DAQPResult *res, DAQPWorkspace *work);                         /* api.c:8-59 */
int setup_daqp(DAQPProblem *qp, DAQPWorkspace *work, c_float *setup_time);     /* api.c:88-90 */
int setup_daqp_main(DAQPProblem *qp, DAQPWorkspace *work, c_float *setup_time, int init_mask); /* api.c:93-160 */
int daqp_update_ldp(const int mask, DAQPWorkspace *work, DAQPProblem *qp);     /* utils.c:58-221 */
void daqp_default_settings(DAQPSettings *settings);                            /* api.c:505-527 */
void allocate_daqp_settings(DAQPWorkspace *work);                              /* api.c:277-282 */
void free_daqp_workspace(DAQPWorkspace *work);                                 /* api.c:393-420 (the device side of a freed workspace is PARKED for the next one of its shape, up to 8: daqp_amd_release_pool() really frees, DAQP_AMD_NO_POOL=1 never parks) */
void free_daqp_ldp(DAQPWorkspace *work);                                       /* api.c:243-275 */
void daqp_primal_init_active(DAQPProblem *qp, c_float *x);                     /* api.c:579-616 */
void daqp_dual_init_active(DAQPProblem *qp, c_float *lam);                     /* api.c:620-633 */
void daqp_set_primal_start(DAQPWorkspace *work, c_float *x);                   /* api.c:636-641 (first centre of the proximal loop) */
void allocate_daqp_workspace(DAQPWorkspace *work, int n, int ns);                /* api.h:41 (records n; state is created by setup_daqp) */
void allocate_daqp_ldp(DAQPWorkspace *work, int n, int m, int ms, int alloc_R, int alloc_v);   /* api.h:42 (records n, m, ms) */
int daqp_first_violating(c_float *x, c_float *A, c_float *bu, c_float *bl, int n, int m, int ms, c_float tol);   /* api.c:562-574, host-only */
/* api.h:55, api.c:531-558: which rows of {x : A x <= b} are redundant (is_redundant[i] = 1) -- b holds the ms simple bounds x_i <= b_i first,
 * A the m - ms general rows.  One polyhedron from host memory through daqp_minrep_batch below (default settings, the current device); without
 * a device, or for a shape daqp_batch_create cannot take (working sets of up to n + 1 rows), is_redundant is filled with -1 and
 * daqp_amd_last_error() says why.  There is no CPU path. */
void daqp_minrep(int *is_redundant, c_float *A, c_float *b, int n, int m, int ms);
/* P polyhedra of one shape at once: A is P*(m-ms)*n row-major, b is P*m, is_redundant is P*m; `memory` (DAQP_MEM_HOST / DAQP_MEM_DEVICE) applies to
 * all three arrays, device arrays are used in place.  Every row is tested on its own (one LDP with the row pinned as an equality; INFEASIBLE means
 * the face is empty, the row redundant), all P*m tests as ONE batch whose m problems per polyhedron read one image of A.  Differences from
 * the reference's sequential loop (utils.c:808-835), all documented in DESIGN.md:
 *  - rows of A are normalised to unit length first (as the QP setup does), so settings->primal_tol is compared with the NORMALISED slack;
 *    verdicts agree with the reference's wherever the redundancy margin is clear of the tolerance;
 *  - an EMPTY polyhedron gives all ones (the reference's answer there depends on the order of the rows): all ones = the polyhedron is empty;
 *  - a vanishing row of A (|A_i|^2 < zero_tol) takes no part and is reported as -1.
 * Returns the number of row tests that ended with a flag other than OPTIMAL / INFEASIBLE (iteration limit, cycling: reported as not redundant,
 * daqp_amd_last_error() names the count) -- 0 when every verdict is clean -- or a negative exit flag.
 * Device memory: per row test the iterate of an ordinary problem of that shape plus its own d (2 m doubles) and sense; per polyhedron one image of A. */
int daqp_minrep_batch(int *is_redundant, const c_float *A, const c_float *b, int P, int n, int m, int ms, int memory, const DAQPSettings *settings, int device);
/* this thread's last daqp_minrep_batch: device bytes it held, and (environment DAQP_AMD_MINREP_TIMES=1) its setup / solve launches in ms from HIP events */
int daqp_minrep_batch_info(float *setup_ms, float *solve_ms, unsigned long long *device_bytes);
/* daqp.c:142-146: sing_ind = EMPTY, reuse_ind = 0, n_active = 0, iterations = 0 -- on the device state of a kept workspace and its host mirrors */
void reset_daqp_workspace(DAQPWorkspace *work);
/* auxiliary.c:482-497: the ACTIVE bit of every working-set row that is not IMMUTABLE is cleared; here the working set is emptied with it
 * (n_active = 0; the stored factor and multipliers count as empty), so the two calls may come in either order.  The next daqp_solve starts
 * cold on the LDP as it stands. */
void daqp_deactivate_constraints(DAQPWorkspace *work);
int setup_daqp_ldp(DAQPWorkspace *work, DAQPProblem *qp, const int init_mask);      /* api.c:161-209 (api.h:35) */
int daqp_ldp(DAQPWorkspace *work);                                                  /* daqp.c:6-108 (daqp.h:12): iterate from the workspace's state; returns the exit flag */
void ldp2qp_solution(DAQPWorkspace *work);                                          /* daqp.c:111-139 (daqp.h:13): done on the device by daqp_ldp -- a no-op kept for callers of the pair */
void daqp_extract_result(DAQPResult *res, DAQPWorkspace *work);                     /* api.c:455-495 (api.h:54): x, lam (from WS / lam_star / n_active), fval, iter, soft_slack from the workspace's fields */

/* ------------------------------------------------------------------ */
/* (2) batch entry points (additive; not in the reference)             */
/* ------------------------------------------------------------------ */
#define DAQP_MEM_HOST 0    /* pointers are host memory: the library stages them over PCIe */
#define DAQP_MEM_DEVICE 1  /* pointers are device memory on the batch's GPU: used in place */

/* N problems of one shape, each array the N per-problem arrays back to back
 * (H: N*n*n, f: N*n, A: N*(m-ms)*n, bupper/blower/sense: N*m).  sense may be NULL. */
typedef struct {
    int N, n, m, ms;
    const c_float *H, *f, *A, *bupper, *blower;
    const int *sense;
    int memory; /* DAQP_MEM_HOST or DAQP_MEM_DEVICE, applies to every pointer above */
} DAQPBatchProblem;

/* Per-problem outputs, back to back (x: N*n, lam: N*m, others: N).  Any pointer may be NULL. */
typedef struct {
    c_float *x, *lam, *fval, *soft_slack;
    int *exitflag, *iter;
    int memory;
    c_float setup_time, solve_time; /* host wall clock of the last call, seconds (includes device sync) */
} DAQPBatchResult;

typedef struct DAQPBatch DAQPBatch; /* device-resident workspaces of N problems */

/* Allocate device workspaces for N problems of shape (n, m, ms) with at most ns_max soft
 * constraints each, on HIP device `device` (-1: current).  settings NULL = defaults.
 * Returns 0 or a negative exit flag. */
int daqp_batch_create(DAQPBatch **out, int N, int n, int m, int ms, int ns_max,
                      const DAQPSettings *settings, int device);
void daqp_batch_free(DAQPBatch *b);
/* A freed batch of ONE problem (what daqp_quadprog and setup_daqp / free_daqp_workspace create and free per call -- reference
 * api.c:61-104) is parked and handed to the next daqp_batch_create of the same shape, device and environment switches, so that
 * repeated single solves do not pay ~40 hipMalloc / hipFree each.  At most 8 are kept; this releases them all now.
 * Environment DAQP_AMD_NO_POOL=1 switches the parking off. */
void daqp_amd_release_pool(void);
/* waits for everything this library has in flight on every device it touched (frees nothing; any number of calls).  Registered with atexit() at
   the first batch / workspace creation, so that a process that exits right after its last solve does not meet the HIP runtime's own teardown with
   commands still retiring (INTEGRATION.md "Process exit"); DAQP_AMD_NO_EXIT_SYNC=1 leaves that to the host. */
void daqp_amd_shutdown(void);
/* hipStream_t the batch launches on (NULL: the legacy default stream). */
void daqp_batch_set_stream(DAQPBatch *b, void *hip_stream);
void daqp_batch_set_settings(DAQPBatch *b, const DAQPSettings *settings);
/* exact != 0: form M = A R^-1 in the reference's operation order (VALU; the whole LDP is then bit-identical
 * to the reference's strict-IEEE build).  0 (default, or env DAQP_AMD_EXACT unset): MFMA f64 matrix cores,
 * M equal to ~1e-16 relative; active sets/iterations identical, x within 1e-9 (tests/test_gpu_fast_mode.py). */
void daqp_batch_set_exact(DAQPBatch *b, int exact);

/* setup_daqp_main for every problem (QP -> LDP: Cholesky, R^-1, M = A R^-1, v, d, initial working
 * set).  init_mask 0 = setup_daqp, DAQP_UPDATE_unconstrained = the daqp_quadprog variant.
 * Returns 0 when launched; per-problem flags (1 ok, <0 exit flag) via daqp_batch_setup_flags. */
int daqp_batch_setup(DAQPBatch *b, const DAQPBatchProblem *p, int init_mask);
/* Shared-structure batches (condensed MPC; SURVEY.md 8f rank 3, docs/docs/linearmpc.md:18-21 of the reference): p->H is
 * ONE n x n matrix and p->A ONE (m-ms) x n matrix for all N problems; f, bupper, blower (and sense) are per problem.
 * This is the reference's MPC usage, batched: setup_daqp once (api.c:88-151, open bounds), then for every problem
 * daqp_update_ldp(DAQP_UPDATE_v|DAQP_UPDATE_d) (utils.c:58-221) with its f and bounds -- bit for bit.  The factorisation
 * runs once and every solve reads one shared image of M.  Follow with daqp_batch_solve / daqp_batch_update as usual. */
int daqp_batch_setup_shared(DAQPBatch *b, const DAQPBatchProblem *p, int init_mask);
/* daqp_update_ldp (utils.c:58-221) for every problem, ANY mask of DAQP_UPDATE_Rinv | M | v | d | sense -- each bit's step on its
 * own, as the reference runs them and as its bindings send them (daqp.pyx:513-571 builds the mask field by field):
 *   v, d          new f and / or bounds on the kept factors and working sets: the warm path (applied by the next solve launch)
 *   sense         the caller's sense replaces the workspace's (p->sense == NULL: zeros) and, if one was given, the working sets are
 *                 rebuilt from its ACTIVE bits (utils.c:84-91,199-211)
 *   M             new A on the kept R^-1 (its rows < ms stay normalised: utils.c:447-452); working sets emptied (utils.c:470);
 *                 the workspace's sense -- the ACTIVE bits of the last solve included -- is kept unless the sense bit is set too
 *   Rinv          new H: factor, then v, M, the normalisations and d follow as in a setup (utils.c:122,135,142,150); sense as for M
 *   all five      a re-setup (the setup kernels; the iterate of a proximal problem is kept, api.c:318 does not run)
 * DAQP_UPDATE_unconstrained / _eliminate may ride along as in setup_daqp_main.  Arrays of `p` that the mask's steps do not read may
 * be NULL; one that they read and that is NULL stays as the batch has it (device-resident arrays were adopted, not copied: they must
 * still be valid).  Per-problem outcome: daqp_batch_setup_flags (1, or the flag daqp_update_ldp would have returned: -1 for crossed
 * bounds -- that problem's LDP is then untouched and its next solve reports the -1 instead of solving -- -5, ...).
 * Masks with the Rinv or M bit but not all five run the generic one-wave setup kernel in the reference's operation order in both
 * arithmetic modes; they are not available after daqp_batch_setup_shared (one H and A for the whole batch: set it up again). */
int daqp_batch_update(DAQPBatch *b, int mask, const DAQPBatchProblem *p);
/* daqp_solve for every problem: dual active-set iteration from the current working sets, then
 * x, lam, fval, exitflag, iter.  Blocks until results are in `r` unless r->memory is DEVICE
 * (then they are ordered on the batch's stream). */
int daqp_batch_solve(DAQPBatch *b, DAQPBatchResult *r);
/* Singular Hessians (daqp_prox.c:21-221, utils.c:223-432): with eps_prox != 0 (default -1e-6:
 * automatic) a problem whose Hessian Cholesky finds numerically singular is factorised from H + eps*I (eps doubling
 * while still ill-conditioned; a diagonal H is shifted in its singular coordinates only), and daqp_batch_solve runs the
 * reference's proximal-point outer loop for it: inner LDPs warm-started from each other until ||x - x_old||_inf <
 * eta_prox/eps.  iter is the sum over the inner solves.  eps_prox > 0 forces the shift for every problem.
 * daqp_batch_set_primal_start: api.c:636-641 for every problem (x: N*n), the centre of the first outer iteration.
 * daqp_batch_prox_info: n_prox per problem (types.h:229), outer iterations of the last solve, eps; returns the number
 * of proximal problems.  An LP batch: p->H == NULL in daqp_batch_setup (every problem of the batch; R = I, adaptive
 * smoothing weight, gradient steps, exit flag -3 for an unbounded one: daqp_prox.c LP branch). */
int daqp_batch_set_primal_start(DAQPBatch *b, const c_float *x, int memory);
int daqp_batch_prox_info(DAQPBatch *b, int *n_prox_host, int *outer_host, c_float *eps_host);
/* copy out per-problem setup flags (host int[N]) */
int daqp_batch_setup_flags(DAQPBatch *b, int *flags_host);
/* copy out working sets: n_active (host int[N]) and WS (host int[N*(n+ns_max+1)], -1 padded); either may be NULL */
int daqp_batch_working_sets(DAQPBatch *b, int *n_active_host, int *ws_host);
/* daqp_deactivate_constraints + reset_daqp_workspace for every problem of the batch: the next daqp_batch_solve starts from empty working sets
 * (a daqp_batch_update(UPDATE_v|UPDATE_d) that the next solve launch still owes stays owed) */
int daqp_batch_reset(DAQPBatch *b);
/* Derivative of the solutions of the last daqp_batch_solve: the adjoint (backward) pass of implicit differentiation.
 * With C = [first ms rows of I; A], W the rows of the stored working set, C_W those rows (unsigned) and lam the signed multipliers
 * the solve returned, the optimum satisfies  H x + f + C_W' lam_W = 0,  C_W x = b_W.  For an upstream gradient g = dl/dx per
 * problem (grad_x: N*n) the call solves
 *
 *        [ H    C_W' ] [ dz  ]   [ g ]
 *        [ C_W  0    ] [ dnu ] = [ 0 ]
 *
 * on the kept factor of H (nothing is factored again but the n_active x n_active Gram matrix of the active rows) and returns
 *   dz       N*n   the caller forms   dl/df = -dz,   dl/dH = -1/2 (dz x' + x dz'),
 *                                     dl/dA_i = -(lam_i dz + dnu_i x)' for the general rows i in W, zero for every other row
 *   dbupper  N*m   dl/dbupper: dnu_i for the rows of W held at their upper bound, zero elsewhere
 *   dblower  N*m   dl/dblower: dnu_i for the rows of W held at their lower bound, zero elsewhere
 *                  (every dnu_i goes to exactly one of the two; an equality row, bupper == blower, may appear on either side;
 *                   dnu = dbupper + dblower)
 *   status   N     0: done.  The problem's exit flag when its solve (or setup / update) did not end DAQP_EXIT_OPTIMAL;
 *                  DAQP_EXIT_UNSUPPORTED when it went through the proximal loop (singular H, LP: daqp_batch_backward_nullspace
 *                  below differentiates those); DAQP_BACKWARD_SINGULAR when
 *                  the active rows are linearly dependent.  All three outputs of such a problem are zero.
 * x and lam are those of the solve, in the caller's units like everything here.  A problem that took the unconstrained shortcut
 * has W empty: dz = H^-1 g.  A batch set up with shared H and A is supported; the outputs are per problem (dl/dH and dl/dA of
 * the shared matrices are the sums over the batch).
 * `memory` (DAQP_MEM_HOST / DAQP_MEM_DEVICE) applies to all five arrays.  The call runs on the batch's stream; with device memory
 * it only enqueues (no host synchronisation), with host memory it returns when the results are there.
 * Returns nonzero, with the reason in the last-error string and without any device work, when
 *   - the last operation on the batch was not a successful daqp_batch_solve (a setup, update or reset since then invalidates
 *     the stored optimum),
 *   - the batch was created with ns_max > 0: SOFT CONSTRAINTS ARE OUT OF SCOPE of this entry point (they change the (2,2) block
 *     of the system and need more outputs): daqp_batch_backward_soft below takes such batches,
 *   - a pointer is NULL.
 * Gradients through lam and fval: daqp_batch_backward_dual below. */
int daqp_batch_backward(DAQPBatch *b, const c_float *grad_x, c_float *dz, c_float *dbupper, c_float *dblower, int *status, int memory);
/* Fixed-precision iterative refinement of (x, lam) at the working set of the last daqp_batch_solve.  The solve works in the
 * least-distance coordinates and transforms back through the computed R^-1, so its optimum carries an error of about
 * cond(H) 2^-53; this call removes it.  Held fixed: the stored working set W (WS, n_active, the DAQP_LOWER bit of the workspace's
 * sense), its rows C_W of C = [first ms rows of I; A] (unsigned) and b_W = bupper_k or blower_k by side.  x (N*n) and lam (N*m) come
 * in as the caller has them -- normally what daqp_batch_solve returned, but any starting point is allowed, zeros included; lam is
 * read on W only -- and go out refined.  One step:
 *
 *        r1 = -(H x + f + C_W' lam_W),  r2 = b_W - C_W x     in twice the working precision (error-free products, pairs summed,
 *                                                            rounded once) on the caller's own H, f, A, bupper, blower: arrays
 *                                                            adopted from device memory must still be valid and unchanged
 *        [ H    C_W' ] [ dx   ]   [ r1 ]
 *        [ C_W  0    ] [ dlam ] = [ r2 ]                     in fp64 on the kept factor of H, as daqp_batch_backward solves its system
 *        x += dx,  lam_W += dlam
 *
 * Merit:  mu = max( |r1|_inf / max(1, |Hx|_inf, |f|_inf, |C_W'|lam_W||_inf),  max_k |r2_k| / max(1, |b_k|, sum_j |c_kj x_j|) ),
 * the residuals in it being the doubled-precision ones.  A step is kept only if it lowers mu.  The loop ends at the first rejected
 * step, at mu <= 2^-50, after a kept step that gained less than a factor 2, or after max_steps steps (1..8).  THE RETURNED PAIR NEVER
 * HAS A LARGER mu THAN THE PAIR THAT CAME IN.
 *   x, lam    N*n, N*m   in / out; lam off W is set to 0
 *   fval      N          1/2 x'Hx + f'x of the returned x, formed as a pair and rounded once; may be NULL
 *   residual  N*2        {mu of the pair that came in, mu of the pair that is returned}; may be NULL
 *   steps     N          kept steps; may be NULL
 *   status    N          0: done.  Otherwise the rules of daqp_batch_backward: the setup / update / exit flag of a problem that did not
 *                        end DAQP_EXIT_OPTIMAL; DAQP_EXIT_UNSUPPORTED when it went through the proximal loop (the kept factor is that
 *                        of H + eps I); DAQP_BACKWARD_SINGULAR when a pivot of the Gram matrix of the active rows falls below
 *                        settings->zero_tol.  Such a problem's x and lam are left exactly as they came in, its steps are 0, both
 *                        residuals NaN and its fval is not written.
 * `memory` (DAQP_MEM_HOST / DAQP_MEM_DEVICE) applies to all six arrays.  The call runs on the batch's stream; with device memory it
 * only enqueues (no host synchronisation), with host memory it returns when the results are there.  It reads the batch's state and
 * writes none of it: a daqp_batch_backward, a daqp_batch_solve or an update followed by a warm solve return the same bits with the
 * call and without it.  A batch set up with shared H and A is supported.
 * Returns nonzero, with the reason in the last-error string and without any device work, when
 *   - the last operation on the batch was not a successful daqp_batch_solve,
 *   - the batch was created with ns_max > 0 (soft rows change the (2,2) block of the system),
 *   - x, lam or status is NULL,
 *   - max_steps is not in 1..8. */
int daqp_batch_refine(DAQPBatch *b, c_float *x /* N*n, in/out */, c_float *lam /* N*m, in/out */,
                      c_float *fval /* N, out, may be NULL */, c_float *residual /* N*2 out: before, after; may be NULL */,
                      int *steps /* N, may be NULL */, int *status /* N */, int max_steps, int memory);
/* The same refinement WITHOUT a factor of H: the correction solved by the null-space method on the caller's own Hessian, for the
 * problems that went through the proximal loop (singular H; an LP batch, H == NULL).  Their kept factor is that of H + eps I, so
 * daqp_batch_refine answers DAQP_EXIT_UNSUPPORTED for them -- and they are the problems whose (x, lam) are limited by the outer
 * fixed-point tolerance eta_prox / eps, not by the arithmetic.  The arrays, their in / out meaning, `memory`, the residuals in twice
 * the working precision, the merit mu, the acceptance rule, the end conditions, max_steps in 1..8, lam off W set to 0 and fval as a
 * pair rounded once are those of daqp_batch_refine: THE RETURNED PAIR NEVER HAS A LARGER mu THAN THE PAIR THAT CAME IN.  What differs
 * is how the step is solved.  Per problem (one wavefront, fp64), once: the k = n_active rows of C_W scaled to unit length (norms s);
 * Householder QR C_W' = Q [R; 0] without pivoting; Hr = Z'HZ with Z the last n - k columns of Q, Cholesky.  Then per step
 *
 *        y  = R^-T (r2 / s)
 *        z  = Hr^-1 (Q'(r1 - H Q [y; 0]))[k:]                (n - k entries; none at a vertex)
 *        dx = Q [y; z],   dlam = R^-1 (Q'(r1 - H dx))[:k] / s
 *
 *   which == 0   daqp_batch_refine's kernel runs first; the null-space kernel then runs on the same stream for the problems with
 *                n_prox > 0 only and overwrites their outputs.  Every other problem comes out bit for bit as daqp_batch_refine
 *                gives it.
 *   which == 1   every problem goes through the null-space kernel: a second, independent algorithm for positive definite H.
 *   status       the rules of daqp_batch_backward_nullspace: the setup / update / exit flag of a problem that did not end
 *                DAQP_EXIT_OPTIMAL; DAQP_BACKWARD_SINGULAR when R_jj^2 < settings->zero_tol (dependent active rows; more than n rows
 *                are dependent) or a pivot of Hr <= zero_tol max(1, max_i H_ii) (H not positive definite on the null space of C_W:
 *                the optimum is not locally unique).  An LP has H = 0 -- the identity the batch stores for it is not H --: its
 *                optimum must be a vertex (k == n), anything else is singular.  With a non-zero status x, lam and fval are left
 *                exactly as they came in, steps is 0 and both residuals are NaN.
 * The call runs on the batch's stream (two launches for which == 0); with device memory it only enqueues, with host memory it returns
 * when the results are there.  It reads the batch's state and writes none of it.  H, f, A, bupper and blower are read where the last
 * setup / update left them: device-resident inputs were adopted, not copied, so THEY MUST STILL BE VALID AND UNCHANGED AT THIS CALL.
 * H is taken symmetric.  A batch set up with shared H and A is supported.
 * Returns nonzero, with the reason in the last-error string and without any device work, in the cases of daqp_batch_refine (the last
 * operation was not a successful daqp_batch_solve; ns_max > 0; x, lam or status NULL; max_steps not in 1..8), when which is neither
 * 0 nor 1, and for which == 1 with n > 64: the kernel holds a problem in one wavefront.  With which == 0 the proximal problems of a
 * batch with n > 64 keep DAQP_EXIT_UNSUPPORTED. */
int daqp_batch_refine_nullspace(DAQPBatch *b, c_float *x /* N*n, in/out */, c_float *lam /* N*m, in/out */,
                                c_float *fval /* N, out, may be NULL */, c_float *residual /* N*2 out: before, after; may be NULL */,
                                int *steps /* N, may be NULL */, int *status /* N */, int max_steps, int which, int memory);
/* The same adjoint for batches with soft rows (created with ns_max > 0; DAQP_SOFT in a row's sense).  An active soft row k is not
 * held at its bound b_k but at  c_k x - b_k = rho_soft q_k lam_k  with  q_k = c_k H^-1 c_k'  (the solver adds settings->rho_soft to
 * the diagonal of the NORMALISED M_W M_W'; lam is in the caller's units).  The optimum therefore solves
 *
 *        [ H    C_W' ] [ x   ]   [ -f  ]
 *        [ C_W  -S   ] [ lam ] = [ b_W ],      S = diag(rho_soft q_k for the SOFT rows of W, 0 for the others)
 *
 * and the adjoint for g = dl/dx is the same symmetric matrix:  H dz + C_W' dnu = g,  C_W dz - S dnu = 0.  dz, dbupper, dblower and
 * status are as above, with DAQP_EXIT_SOFT_OPTIMAL a differentiable end state like DAQP_EXIT_OPTIMAL.  S depends on H and A through
 * q_k, which adds a term to their gradients; with  dsig_k = dnu_k lam_k  on the SOFT rows of W and  u_k = H^-1 c_k':
 *
 *        dl/df        = -dz                         dl/dbupper, dl/dblower = dbupper, dblower
 *        dl/drho_soft = sum_k dsig_k q_k
 *        dl/dH        = -1/2 (dz x' + x dz')  -  rho_soft sum_k dsig_k u_k u_k'
 *        dl/dA_i      = -(lam_i dz + dnu_i x)'  +  2 rho_soft dsig_i u_i'      general rows i in W; the second term for SOFT ones only
 *
 * (a soft simple bound, k < ms, has c_k = e_k: its u_k term goes to dl/dH only).  Leaving the u_k terms out keeps dl/df and the
 * bound gradients right and makes dl/dH and dl/dA wrong.  What they need comes back in three more arrays, each of which may be NULL:
 *   qsoft     N*m          q_k for the SOFT rows of W, zero for every other row
 *   usoft     N*ns_max*n   u_k, one n-vector per SOFT row of W, in working-set order; unused slots are zero
 *   usoft_id  N*ns_max     the row ids k of those vectors; unused slots are -1
 * Preconditions, stream and memory semantics are those of daqp_batch_backward (`memory` applies to all eight arrays); ns_max > 0
 * is not a refusal here, and for ns_max == 0 dz, dbupper, dblower and status are bit for bit those of daqp_batch_backward (qsoft is
 * zero, usoft and usoft_id are empty).  Gradients through lam, fval and soft_slack: daqp_batch_backward_soft_dual below.  Per-row
 * soft weights do not exist here. */
int daqp_batch_backward_soft(DAQPBatch *b, const c_float *grad_x, c_float *dz, c_float *dbupper, c_float *dblower,
                             c_float *qsoft /* N*m */, c_float *usoft /* N*ns_max*n */, int *usoft_id /* N*ns_max */,
                             int *status, int memory);
/* The same adjoint WITHOUT a factor of H: the null-space method on the caller's own Hessian, for the problems that went through the
 * proximal loop (singular H; an LP batch, H == NULL).  Their kept factor is that of H + eps I, so daqp_batch_backward answers
 * DAQP_EXIT_UNSUPPORTED for them; the system
 *
 *        [ H    C_W' ] [ dz  ]   [ g ]
 *        [ C_W  0    ] [ dnu ] = [ 0 ]
 *
 * is nonsingular all the same whenever the optimum is locally unique: C_W of full row rank and Z'HZ positive definite, Z a basis of
 * the null space of C_W.  Per problem (one wavefront, fp64): the k = n_active rows of C_W scaled to unit length; Householder QR
 * C_W' = Q [R; 0] without pivoting; Hr = Z'HZ with Z the last n - k columns of Q, Cholesky; then
 *
 *        dz = Z Hr^-1 Z' g          dnu = R^-1 Q1' (g - H dz), row scaling undone
 *
 * Singularity tests, both DAQP_BACKWARD_SINGULAR: R_jj^2 < settings->zero_tol (dependent active rows: what daqp_batch_backward's
 * Gram Cholesky tests on the same unit rows; more than n rows are dependent), and a pivot of Hr <= zero_tol max(1, max_i H_ii) (H
 * is not positive definite on the null space: no unique adjoint).  An LP has H = 0: its optimum must be a vertex (k == n, dz = 0),
 * anything else is singular.  The system contains neither x nor lam: the outputs depend on H, A and W only, not on how tightly the
 * proximal loop converged.  dz, dbupper, dblower and status mean what they mean for daqp_batch_backward (the formulas for dl/df,
 * dl/dH, dl/dA, dl/dbupper, dl/dblower are the same, with the x and lam of the solve; an LP has no dl/dH); a nonzero status --
 * the setup / update / exit flag of a problem that did not end DAQP_EXIT_OPTIMAL, or DAQP_BACKWARD_SINGULAR -- zeroes all three.
 *   which == 0   daqp_batch_backward runs first; the null-space kernel then runs on the same stream for the problems with
 *                n_prox > 0 only and overwrites their outputs.  Every other problem comes out bit for bit as daqp_batch_backward
 *                gives it.
 *   which == 1   every problem goes through the null-space kernel: a second, independent algorithm for positive definite H.
 * Preconditions, stream, memory semantics and refusals are those of daqp_batch_backward (`memory` applies to all five arrays).
 * The kernel reads H and A where the last setup / update left them: device-resident inputs were adopted, not copied, so -- as for
 * the second pass of INFEASIBLE verdicts (daqp_batch_set_recheck) -- THEY MUST STILL BE VALID AT THIS CALL.  H is taken symmetric.
 * Left as it is:
 *   - n > 64: the kernel holds a problem in one wavefront.  With which == 0 proximal problems of such a batch keep
 *     DAQP_EXIT_UNSUPPORTED; which == 1 is refused for it.
 *   - batches created with ns_max > 0 are refused: q_k = c_k H^-1 c_k' of a soft row does not exist for a singular H. */
int daqp_batch_backward_nullspace(DAQPBatch *b, const c_float *grad_x, c_float *dz, c_float *dbupper, c_float *dblower, int *status,
                                  int which, int memory);
/* The adjoint with a DUAL right-hand side: a loss l(x, lam, fval) that also depends on the signed multipliers the solve returned
 * (lam_k > 0 at an upper bound, < 0 at a lower one; the rows C_W are unsigned, as everywhere here).  With g_x = dl/dx (grad_x: N*n)
 * and g_lamW[k] = grad_lam[WS[k]] (grad_lam: N*m, dl/dlam in the caller's units) the call solves, at the stored working set W,
 *
 *        [ H    C_W' ] [ dz  ]   [ g_x    ]
 *        [ C_W  0    ] [ dnu ] = [ g_lamW ]
 *
 * -- the system of daqp_batch_backward with a second block in its right-hand side; on the kept factor H = R'R only the Gram system
 * changes, (N_W N_W') dnu = N_W w - g_lamW, and on the null-space route the solve becomes y = R^-T (g_lamW / s),
 * z = Hr^-1 (Q'(g_x - H Q [y; 0]))[k:], dz = Q [y; z], dnu = R^-1 (Q'(g_x - H dz))[:k] / s (at an LP vertex, k = n, dz is no longer zero).
 * THE FIVE GRADIENT FORMULAS ARE UNCHANGED:  dl/df = -dz,  dl/dH = -1/2 (dz x' + x dz'),  dl/dA_i = -(lam_i dz + dnu_i x)' for the general
 * rows i in W,  dl/dbupper = dbupper,  dl/dblower = dblower  (dnu_i on the side where the row sits).  grad_lam is read on W only: the
 * multiplier of a row off W is identically 0 near the optimum and has no derivative.  A problem with W empty (the unconstrained
 * shortcut) ignores grad_lam.
 * A gradient g_fval = dl/dfval through  fval = 1/2 x'Hx + f'x  needs no solve (envelope theorem); the caller adds
 *
 *        dl/df += g_fval x        dl/dH += 1/2 g_fval x x'
 *        dl/dbupper_i, dl/dblower_i += -g_fval lam_i   (on the side where row i of W sits)
 *        dl/dA_i += g_fval lam_i x'                    (general rows i in W)
 *
 *   which == -1   the Gram route only: outputs, status rules, stream, memory semantics and preconditions of daqp_batch_backward
 *   which == 0/1  as daqp_batch_backward_nullspace: 0 -- the Gram kernel first, then the null-space kernel for the problems with
 *                 n_prox > 0; 1 -- the null-space kernel for every problem.  Status rules, singularity tests and the validity of the
 *                 adopted H and A are those of that entry.
 * grad_x may be NULL (= 0), grad_lam may be NULL (= 0), not both.  With grad_lam == NULL the outputs are bit for bit those of the
 * existing entry for the same `which`; with grad_lam all zeros they compare equal to them.  `memory` applies to all six arrays.
 * Returns nonzero, with the reason in the last-error string and without any device work, when both gradients are NULL, an output is
 * NULL, which is outside -1..1, which == 1 with n > 64, the last operation on the batch was not a successful daqp_batch_solve, or the
 * batch was created with ns_max > 0.
 * Not built: soft rows (ns_max > 0 is refused), soft_slack gradients -- daqp_batch_backward_soft_dual below has both --,
 * Jacobians and multi-RHS solves, n > 64 on the null-space route, MultiBatchModel.  An eliminated batch (EliminatedBatchModel) has
 * its own entry: daqp_batch_eliminate_backward. */
int daqp_batch_backward_dual(DAQPBatch *b, const c_float *grad_x /* N*n, may be NULL = 0 */,
                             const c_float *grad_lam /* N*m, may be NULL = 0 */,
                             c_float *dz, c_float *dbupper, c_float *dblower, int *status,
                             int which /* -1: Gram only; 0 / 1: as daqp_batch_backward_nullspace */, int memory);
/* Both extensions at once: the adjoint of a batch WITH SOFT ROWS for a loss l(x, lam, fval, soft_slack).  The optimum solves
 * K [x; lam_W] = [-f; b_W] with the symmetric K = [H C_W'; C_W -S], S = diag(rho_soft q_k on the SOFT rows of W, 0 elsewhere),
 * q_k = c_k H^-1 c_k' (daqp_batch_backward_soft), and the solve reports
 *
 *        soft_slack = sum_k S_k lam_k^2  (SOFT rows of W)        fval = 1/2 x'Hx + f'x + 1/2 soft_slack
 *
 * With g_x = dl/dx (grad_x: N*n), g_lam = dl/dlam (grad_lam: N*m, read on W only), g_s = dl/dsoft_slack (grad_slack: N) and lam the
 * signed multipliers the solve returned (lam: N*m, read on the SOFT rows of W), the call solves ONE system,
 *
 *        [ H    C_W' ] [ dz  ]   [ g_x       ]        ghat_lam[k] = g_lam[WS[k]] + 2 g_s rho_soft q_k lam_k   on the SOFT rows of W
 *        [ C_W  -S   ] [ dnu ] = [ ghat_lamW ],       ghat_lam[k] = g_lam[WS[k]]                              elsewhere
 *
 * -- on the kept factor only the right-hand side of the Gram system changes, (C_W H^-1 C_W' + S) dnu = C_W H^-1 g_x - ghat_lamW.
 * THE FIVE GRADIENT FORMULAS ARE UNCHANGED:  dl/df = -dz,  dl/dH = -1/2 (dz x' + x dz'),  dl/dA_i = -(lam_i dz + dnu_i x)' for the
 * general rows i in W,  dl/dbupper = dbupper,  dl/dblower = dblower.  The terms of the q_k-dependence of S keep their form with a
 * wider dsig, the caller's to form as for daqp_batch_backward_soft (g_f = dl/dfval):
 *
 *        dsig_k       = dnu_k lam_k - 1/2 g_f lam_k^2 + g_s lam_k^2        on the SOFT rows of W
 *        dl/drho_soft = sum_k dsig_k q_k
 *        dl/dH       -= rho_soft sum_k dsig_k u_k u_k'
 *        dl/dA_i     += 2 rho_soft dsig_i u_i'
 *
 * g_s lam_k^2 is the direct dependence of soft_slack on S_k.  -1/2 g_f lam_k^2 is the envelope theorem: fval is the optimal value of
 * the penalised problem with penalty s_k^2 / (2 rho_soft q_k), s_k = rho_soft q_k lam_k, so dfval/d(rho_soft q_k) = -1/2 lam_k^2.  The
 * other envelope terms of g_f need no solve and are those of daqp_batch_backward_dual:  dl/df += g_f x,  dl/dH += 1/2 g_f x x',
 * dl/dbupper_i, dl/dblower_i += -g_f lam_i (the row's side),  dl/dA_i += g_f lam_i x'.
 *   dz, dbupper, dblower, status, qsoft, usoft, usoft_id    as daqp_batch_backward_soft; the last three may each be NULL
 * Preconditions, stream, memory semantics (`memory` applies to all twelve arrays), status rules (DAQP_EXIT_SOFT_OPTIMAL is
 * differentiable) and zeroed outputs on a non-zero status are those of daqp_batch_backward_soft.  grad_x, grad_lam and grad_slack may
 * each be NULL (= 0).  With grad_lam == NULL and grad_slack == NULL the outputs are bit for bit those of daqp_batch_backward_soft; with
 * zeros in them they compare equal to it.  A batch created with ns_max == 0 has no soft row and no soft_slack: grad_slack meets nothing
 * there, and dz, dbupper, dblower and status are bit for bit those of daqp_batch_backward_dual(which = -1) (qsoft is zero).  The kernels
 * are the SOFT ones with the DUAL right-hand side; they need no more LDS than either, so every shape runs on the path it ran on.
 * Returns nonzero, with the reason in the last-error string and without any device work, when all three gradients are NULL (on a batch
 * with ns_max == 0: grad_x and grad_lam), grad_slack is given without lam, an output other than the three soft arrays is NULL, or the
 * last operation on the batch was not a successful daqp_batch_solve.
 * Not built: the null-space route (q_k does not exist for a singular H), eliminated batches with SOFT rows, MultiBatchModel, per-row
 * soft weights, Jacobians. */
int daqp_batch_backward_soft_dual(DAQPBatch *b, const c_float *grad_x /* N*n, may be NULL */, const c_float *grad_lam /* N*m, may be NULL */,
                                  const c_float *grad_slack /* N, may be NULL */,
                                  const c_float *lam /* N*m, required iff grad_slack != NULL */,
                                  c_float *dz, c_float *dbupper, c_float *dblower,
                                  c_float *qsoft, c_float *usoft, int *usoft_id,
                                  int *status, int memory);
/* ---- the certificate of a batch of (x, lam) pairs: KKT residuals and Farkas measures, on the device, in twice the working precision
 * (certify.hip.h).  Stateless: no DAQPBatch, no exit flags -- it reads the caller's H, f, A, bupper, blower, sense, x and lam and nothing
 * else, so it certifies the answer of any solver and depends on no adopted pointer.  With C = [I_ms ; A] and the reference's sign
 * convention (H x + f + C'lam = 0, lam_k > 0 on an upper bound), in the problem's own units (no row is scaled), per problem:
 *   stationarity        max_j |(H x + f + C'lam)_j|
 *   stationarity_scale  max(1, max_j |(H x)_j|, max_j |f_j|, max_j |(C'|lam|)_j|) with C'|lam| = sum_k c_kj |lam_k| (C keeps its signs);
 *                       stationarity / stationarity_scale is the relative residual
 *   primal              the largest of max(c_k x - bupper_k, blower_k - c_k x, 0) over the rows that are HELD: every row but the
 *                       DAQP_IMMUTABLE ones that are no equality (bupper_k == blower_k), and the DAQP_SOFT ones with lam_k != 0
 *   primal_row          the row where that maximum is reached (the first of equals); -1 when primal is 0 (or NaN)
 *   complementarity     the largest of: for rows that are neither soft nor an equality and have lam_k != 0, the distance |c_k x - b_k| from
 *                       the bound the sign of lam_k names; for equality rows (DAQP_IMMUTABLE, bupper_k == blower_k), |c_k x - bupper_k|
 *   wrong_sign          the number of non-equality rows with lam_k != 0 whose nearer bound (c_k x - bupper_k >= blower_k - c_k x: the upper
 *                       one) is not the one the sign of lam_k names
 *   objective           1/2 x'Hx + f'x
 *   ray_residual        max_j |(C'lam)_j|      ray_scale  max_j |(C'|lam|)_j|
 *   ray_support         sum over lam_k > 0 of lam_k bupper_k  +  sum over lam_k < 0 of lam_k blower_k
 * The last three read lam as a Farkas ray: for every feasible x, 0 = lam'Cx <= ray_support when C'lam = 0, so ray_residual == 0 together
 * with ray_support < 0 proves {blower <= Cx <= bupper} empty.  DAQP_SOFT rows enter them as they are: a soft row may be violated, so A RAY
 * WITH WEIGHT ON A SOFT ROW PROVES NOTHING.  Every quantity is computed for every problem; the caller reads the residuals of the OPTIMAL
 * problems and the ray measures of the INFEASIBLE ones.
 * Accuracy: every inner product and sum is accumulated as a (hi, lo) pair -- error-free products through fma, error-free sums, pairs
 * across lanes and waves -- and rounded once.  For a quantity that is a sum of K terms with S = sum |terms|,
 *       |computed - exact| <= 2^-52 |exact| + (K + 2)^2 2^-104 S
 * (the bound of a compensated dot product, Ogita-Rump-Oishi 2005; derived in certify.hip.h, not measured); a max over rows or columns
 * inherits the bound of its rows.  K: n + 1 + (m - ms) + 1 for a component of the stationarity residual, n for c_k x, n^2 + n for the
 * objective, m for ray_support.  A NaN in x makes every output that depends on x NaN; non-finite inputs give non-finite outputs.
 * Arguments: p->N problems of p->n variables and p->m rows, the first p->ms of them simple bounds; p->H == NULL: an LP (no H term);
 * p->sense == NULL: all zero; shared != 0: p->H and p->A are ONE matrix each for all N problems (as daqp_batch_setup_shared takes
 * them).  x is N*n, lam N*m.  p->memory applies to EVERY array -- the problem's, x, lam and the outputs: host arrays are staged and the
 * call returns when the results are there; device arrays (on `device`; -1: the current one) are used in place and the call only
 * enqueues one kernel on hip_stream (a hipStream_t; NULL: the null stream).  n <= 64 runs one wavefront per problem, n <= 511 one
 * workgroup per problem.  Returns 0, or DAQP_EXIT_UNSUPPORTED with the reason in daqp_amd_last_error() and no device work: a NULL out,
 * p, x or lam (or f, a needed A, bounds); N < 1, n outside 1..511, m outside 0..2^24, ms > n or ms > m; no HIP device. */
typedef struct {
    c_float *stationarity, *stationarity_scale, *primal, *complementarity, *objective,
            *ray_residual, *ray_scale, *ray_support;   /* N each; any may be NULL */
    int *wrong_sign, *primal_row;                       /* N each; any may be NULL */
} DAQPBatchCertificate;
int daqp_certify_batch(DAQPBatchCertificate *out, const DAQPBatchProblem *p, const c_float *x, const c_float *lam,
                       int shared /* p->H, p->A are one matrix each */, int device, void *hip_stream);
/* ---- equality rows of a batch eliminated on the device: reduce, solve the smaller batch, expand (eliminate.hip.h).  An additive front
 * end: DAQP_UPDATE_eliminate inside daqp_batch_setup / daqp_quadprog stays accepted and ignored.  With C = [first ms rows of I; A]
 * (m rows), the caller names the equality rows, eq_rows: neq distinct, ascending indices into 0..m-1, 1 <= neq < n, ONE row set for the
 * whole batch (a simple-bound row fixes a variable).  Per problem, E = C_eq_rows, e = bupper_eq_rows, I = the other m - neq rows
 * ("kept rows") in their original order:
 *
 *        E' = Q [R; 0],  Q = [Q1 Z]     Householder QR, no pivoting, of the rows of E scaled to unit length; Z is n x nr, nr = n - neq
 *        x0 = Q1 R^-T e                 the minimum-norm solution of E x = e (row scaling undone);   x = x0 + Z y
 *
 *   reduced problem, shape (nr, m - neq, ms = 0):
 *        H_r = Z'HZ  (one triangle, mirrored: exactly symmetric)        f_r = Z'(H x0 + f)        A_r = C_I Z
 *        bupper_r = bupper_I - C_I x0,  blower_r = blower_I - C_I x0    (a bound with |b| >= DAQP_INF stays as it is)
 *        sense_r = sense_I              (SOFT, IMMUTABLE, ACTIVE, LOWER carried over: a warm start survives)
 *                                       A SOFT kept row is weighted in the reduced problem by q_k = c_k Z H_r^-1 Z'c_k', not by c_k H^-1 c_k':
 *                                       an ACTIVE soft row sits rho_soft q_k lam_k beyond its bound with the reduced q_k, so x, lam and
 *                                       soft_slack are those of the reduced problem and differ from the unreduced solve by
 *                                       rho_soft (q_k^full - q_k^reduced) lam_k there.  Inactive soft rows change nothing.
 *        c0 = 1/2 x0'Hx0 + f'x0         LP batches (H == NULL): H_r == NULL, f_r = Z'f, c0 = f'x0
 *
 *   expansion of a reduced result (y, lam_r, fval_r):
 *        x = x0 + Z y        lam_I = lam_r (back at the original row positions)        fval = fval_r + c0
 *        lam_E = -R^-1 Q1'(H x + f + C_I'lam_I)   in the caller's units: the full pair satisfies H x + f + C'lam = 0
 *        exitflag, iter and soft_slack pass through
 *
 * Per-problem flags (daqp_batch_elimination_flags): 1; DAQP_EXIT_OVERDETERMINED_INITIAL (-6) when R_jj^2 < settings->zero_tol, the
 * dependence test of daqp_batch_backward_nullspace -- every reduced array of that problem is zero; DAQP_EXIT_UNSUPPORTED (-8) when
 * bupper_k != blower_k on a row of eq_rows (no equality problem) -- its x0, f_r, c0 and reduced bounds are zero.  The rest of the batch is
 * untouched either way, and daqp_batch_expand gives such a problem its flag as exitflag and zero x, lam and fval.
 *   daqp_batch_eliminate            p: N problems with their own H and A (shared-structure batches are out of scope); eq_rows is host
 *                                   memory.  Device-resident arrays of p are BORROWED -- H, A, f, the bounds and sense must stay valid
 *                                   while the handle lives (expansion reads H, f and A); host-resident ones are copied.  One launch on
 *                                   hip_stream (a hipStream_t; NULL: the null stream) of `device` (-1: the current one).
 *                                   n <= 64: one wavefront per problem, H and the reflectors in LDS; n <= 511: one workgroup per problem.
 *                                   ONLY this call has the workgroup tier: update, expand, basis and read run one wavefront per
 *                                   problem at every n (up to eight entries per lane).
 *   daqp_batch_eliminate_update     new f and / or bounds (NULL: unchanged) on the kept Q, R: x0, f_r, the reduced bounds, c0 and the
 *                                   -8 / 1 flags only -- bit for bit what a fresh daqp_batch_eliminate on those data writes.  The warm
 *                                   path of an MPC loop: follow with daqp_batch_update(DAQP_UPDATE_v | DAQP_UPDATE_d) on the reduced batch.
 *   daqp_batch_elimination_problem  the reduced problem: device pointers owned by the handle, valid until it is freed
 *                                   (memory = DAQP_MEM_DEVICE; hand it to daqp_batch_setup of a batch of shape (nr, m - neq, 0))
 *   daqp_batch_expand               reduced -> full; both results on the same side (host or device); reduced->x, lam and exitflag
 *                                   are needed, any pointer of `full` may be NULL
 *   daqp_batch_elimination_basis    x0 (N*n), Z (N*n*nr, row-major n x nr per problem), c0 (N); any may be NULL -- for tests and for
 *                                   callers who chain derivatives through the elimination themselves
 *   daqp_batch_elimination_read     copies of the reduced arrays (N*nr*nr, N*nr, N*mr*nr, N*mr, N*mr, N*mr with nr = n - neq,
 *                                   mr = m - neq); any may be NULL, H must be NULL for an LP batch
 * Host memory: the call returns when the results are there; device memory: it only enqueues on the handle's stream.
 * Every entry returns 0, or nonzero with the reason in daqp_amd_last_error() and no device work: neq < 1 or neq >= n; rows out of
 * range or not ascending; n > 511; a NULL pointer; host and device memory mixed within one call.  Without a HIP device every entry
 * returns DAQP_EXIT_UNSUPPORTED ("no HIP device").  A failed daqp_batch_eliminate leaves *out NULL.
 * Not built: DAQP_UPDATE_eliminate in place, per-problem equality sets, shared H / A, the multi-device entry, and refine through
 * an eliminated batch.  The adjoint: daqp_batch_eliminate_backward below. */
typedef struct DAQPBatchElimination DAQPBatchElimination;
int daqp_batch_eliminate(DAQPBatchElimination **out, const DAQPBatchProblem *p, const int *eq_rows /* host, neq */, int neq,
                         const DAQPSettings *settings, int device, void *hip_stream);
int daqp_batch_eliminate_update(DAQPBatchElimination *el, const c_float *f, const c_float *bupper, const c_float *blower, int memory); /* NULL: unchanged */
int daqp_batch_elimination_problem(DAQPBatchElimination *el, DAQPBatchProblem *reduced);  /* device pointers owned by el; valid until free */
int daqp_batch_elimination_flags(DAQPBatchElimination *el, int *flags_host);              /* 1, -6, -8 per problem */
int daqp_batch_expand(DAQPBatchElimination *el, const DAQPBatchResult *reduced, DAQPBatchResult *full);
int daqp_batch_elimination_basis(DAQPBatchElimination *el, c_float *x0 /* N*n */, c_float *Z /* N*n*nr */, c_float *c0 /* N */, int memory);
int daqp_batch_elimination_read(DAQPBatchElimination *el, c_float *H, c_float *f, c_float *A, c_float *bupper, c_float *blower, int *sense, int memory);
unsigned long long daqp_batch_elimination_bytes(const DAQPBatchElimination *el);
void daqp_batch_elimination_free(DAQPBatchElimination *el);
/* The adjoint of an eliminated batch (eliminate_adjoint.hip.h): implicit differentiation needs neither dZ nor dx0, only the KKT system
 * of the FULL problem at its full working set W = E u W_I -- E the equality rows, W_I the active kept rows of the reduced solve -- and
 * that system is solved by the route of the forward pass, on the factor of the equality rows that the handle keeps and on the factor of
 * H_r that the reduced batch keeps.  Notation of daqp_batch_eliminate: C = [first ms rows of I; A]; E = C_eq_rows with unit-row QR
 * E' = Q [R; 0], Q = [Q1 Z], row norms s; I the kept rows; H_r = Z'HZ, A_r = C_I Z; W_I the stored working set of the reduced batch, its
 * rows mapped back through the kept rows.  For g_x = dl/dx (grad_x: N*n, may be NULL = 0) and g_lam = dl/dlam (grad_lam: N*m, may be
 * NULL = 0, read on W only; not both NULL) the call solves
 *
 *        [ H     E'   C_WI' ] [ dz    ]   [ g_x     ]
 *        [ E     0    0     ] [ dnu_E ] = [ g_lam_E ]
 *        [ C_WI  0    0     ] [ dnu_I ]   [ g_lam_WI]
 *
 * in three steps:
 *   1. reduce (one kernel)   y = R^-T (g_lam_E / s),  dz0 = Q [y; 0],  grad_y = (Q'(g_x - H dz0))[neq:],
 *                            grad_lam_r = g_lam_I - C_I dz0 for every kept row (the reduced adjoint reads it on W_I only).
 *                            With grad_lam == NULL: dz0 = 0, grad_y = (Q'g_x)[neq:], and no grad_lam_r is formed.
 *   2. solve                 the adjoint of the reduced batch -- what daqp_batch_backward_dual runs for it -- on grad_y and, when
 *                            grad_lam was given, grad_lam_r; `which` is passed through unchanged: dz_r, dbupper_r, dblower_r, status_r
 *   3. expand (one kernel)   dz = dz0 + Q [0; dz_r];  dnu_I = dbupper_r + dblower_r, written to the original row positions, each on
 *                            the side where the reduced call put it;  R dnu~ = (Q'(g_x - H dz - C_WI' dnu_I))[:neq],  dnu_E = dnu~ / s
 * -- the structure of the forward pass with e -> g_lam_E, f -> -g_x and the bounds -> g_lam_I.
 *   - dnu_E goes to DBUPPER of the equality rows (the elimination reads e from bupper); dblower is 0 there.  A caller whose equality
 *     right-hand side feeds both bounds adds the two, as the chain rule does.
 *   - An LP batch (H == NULL) has H = 0 in every product.
 *   - A problem whose elimination flag is -6 or -8 gets that flag as its status and zero outputs; every other problem gets status_r
 *     (the rules of daqp_batch_backward / _nullspace on the reduced batch), with zero outputs where that is non-zero.
 * dz (N*n), dbupper, dblower (N*m) and status (N) mean exactly what they mean for daqp_batch_backward: THE FIVE GRADIENT FORMULAS ARE
 * UNCHANGED -- dl/df = -dz, dl/dH = -1/2 (dz x' + x dz'), dl/dA_i = -(lam_i dz + dnu_i x)' for the general rows i in W, dl/dbupper =
 * dbupper, dl/dblower = dblower -- with the full x and lam that daqp_batch_expand returned, and so are the envelope terms of a gradient
 * through fval (daqp_batch_backward_dual).
 * `reduced` is the batch that was set up on daqp_batch_elimination_problem and solved.  Three launches on the handle's stream (one more
 * where which == 0 adds the null-space kernel).  The intermediates (grad_y, grad_lam_r, dz0, dz_r, dbupper_r, dblower_r, status_r) are
 * device buffers of the handle's, allocated at the first call and counted by daqp_batch_elimination_bytes from then on.  `memory`
 * applies to all six arrays: with device memory the call only enqueues, with host memory it stages them and returns when the results
 * are there.  H and A are read where daqp_batch_eliminate found them: borrowed device arrays must still be valid and unchanged.
 * Returns nonzero, with the reason in the last-error string and without any device work, for
 *   - a NULL handle, batch or output; both gradients NULL; which outside -1..1;
 *   - a reduced batch whose (N, n, m, ms) is not (N, nr, mr, 0), or one on another device or another stream than the handle;
 *   - a reduced batch created with ns_max > 0 (a SOFT kept row is weighted by the reduced q_k: out of scope);
 *   - a reduced batch whose last operation was not a successful daqp_batch_solve;
 *   - which == 1 with nr > 64.
 * Not built: SOFT rows, refine through an eliminated batch, shared H / A, per-problem equality sets, the multi-device entry. */
int daqp_batch_eliminate_backward(DAQPBatchElimination *el, DAQPBatch *reduced,
                                  const c_float *grad_x /* N*n, may be NULL = 0 */, const c_float *grad_lam /* N*m, may be NULL = 0 */,
                                  c_float *dz, c_float *dbupper, c_float *dblower, int *status,
                                  int which /* -1, 0, 1: as daqp_batch_backward_dual, applied to the reduced batch */, int memory);
/* one-shot: create + setup(DAQP_UPDATE_unconstrained) + solve + free == N x daqp_quadprog */
int daqp_quadprog_batch(DAQPBatchResult *r, const DAQPBatchProblem *p, const DAQPSettings *settings);

/* ---- several GPUs of this host (independent problems, no exchange step) -------------------------------------------
 * A DAQPMultiBatch is G device-resident shards -- each an ordinary DAQPBatch on its own device and HIP stream, driven by its own
 * persistent host thread -- over which ONE batch of N problems is dealt: problem k lives on shard k mod G (interleaved, so that the
 * spread of iteration counts averages out).  Factors, working sets and iterates stay on the devices between calls, so the
 * reference's setup_daqp -> daqp_solve -> {daqp_update_ldp -> daqp_solve}* sequence runs over G devices from one C process.
 * devices == NULL: 0 .. n_devices-1; n_devices <= 0: every visible device (a list, if passed, is then ignored).  A device may be
 * listed more than once (its shards share it).  G = min(n_devices, N).
 *   daqp_batch_setup_multi / update_multi / solve_multi take ONE host-resident batch in the caller's order (memory must be
 *     DAQP_MEM_HOST): every shard gathers its problems through pinned buffers, chunk by chunk, two deep, into its own device slots;
 *     results come back the same way, each to its own index.  update_multi: any mask of daqp_batch_update (the arrays its steps read;
 *     a full re-setup needs every array).
 *   daqp_batch_*_multi_shards take G descriptors, ps[g] / rs[g] = shard g's problems / results back to back (N = that shard's
 *     size: daqp_batch_multi_shard), host-resident or resident ON THAT SHARD'S DEVICE (used in place); the shards run side by side.
 *   daqp_batch_multi_shard hands out shard g's DAQPBatch (for the inspection calls above: setup flags, working sets, kernel times).
 * Every call returns when all shards have finished it. */
typedef struct DAQPMultiBatch DAQPMultiBatch;
int daqp_batch_create_multi(DAQPMultiBatch **out, int N, int n, int m, int ms, int ns_max, const DAQPSettings *settings,
                            const int *devices, int n_devices);
void daqp_batch_free_multi(DAQPMultiBatch *mb);
int daqp_batch_multi_shards(const DAQPMultiBatch *mb);                                           /* G */
DAQPBatch *daqp_batch_multi_shard(DAQPMultiBatch *mb, int g, int *shard_N, int *device);        /* shard g; either out-pointer may be NULL */
int daqp_batch_setup_multi(DAQPMultiBatch *mb, const DAQPBatchProblem *p, int init_mask);
int daqp_batch_update_multi(DAQPMultiBatch *mb, int mask, const DAQPBatchProblem *p);
int daqp_batch_solve_multi(DAQPMultiBatch *mb, DAQPBatchResult *r);
int daqp_batch_setup_multi_shards(DAQPMultiBatch *mb, const DAQPBatchProblem *ps /* [G] */, int init_mask);
int daqp_batch_update_multi_shards(DAQPMultiBatch *mb, int mask, const DAQPBatchProblem *ps /* [G] */);
int daqp_batch_solve_multi_shards(DAQPMultiBatch *mb, DAQPBatchResult *rs /* [G] */);
/* one-shot on top of it: create + setup(DAQP_UPDATE_unconstrained) + solve + free == N x daqp_quadprog over the listed devices;
 * problems and results host-resident; setup_time / solve_time: the slowest shard's */
int daqp_quadprog_batch_multi(DAQPBatchResult *r, const DAQPBatchProblem *p, const DAQPSettings *settings,
                              const int *devices, int n_devices);

/* device-side timing of the last setup / solve launches (HIP events on the batch's stream), ms */
int daqp_batch_kernel_ms(DAQPBatch *b, float *setup_ms, float *solve_ms);
/* Default arithmetic only: problems that the FIRST solve after a daqp_batch_setup (or after a daqp_batch_update with every bit set)
   declares infeasible are set up and solved again in the reference's own arithmetic, and that result (exit flag, iter, lam, stored
   iterate) is the one reported -- "infeasible" is decided by comparing rounding noise with dual_tol (auxiliary.c:284-287) and only the
   reference's arithmetic reproduces the reference's noise.  The second pass reads the setup's inputs again at solve time.  Host-
   resident inputs were staged into the batch's own buffers: nothing to watch.  DEVICE-resident inputs were adopted, not copied: they
   must still hold what the setup read when the solve runs -- a caller that recycles those buffers between setup and solve switches
   the pass off for that batch, daqp_batch_set_recheck(b, 0) (or DAQP_AMD_RECHECK_DEVICE=0 for the process; DAQP_AMD_NO_RECHECK=1
   switches it off for every batch).  daqp_batch_rechecked: how many problems of the last daqp_batch_solve took the second pass
   (-1: there were some and no memory for the companion batch -- the first pass's verdicts stand); daqp_batch_recheck_ms: its
   device time, which is part of the solve time daqp_batch_kernel_ms reports.  A WARM solve (after an update of f / bounds) that ends
   INFEASIBLE has no such pass: its starting point already carries the default arithmetic's rounding.  THE BOUND: the exit flag is the
   reference's; the iteration at which the verdict falls is within TWO of the reference's (tests/test_gpu_golden.py asserts it per problem).
   Which comparison it is (tools/warm_infeasible_trace.py, profiles/r06_warm_infeasible_traces.txt): the event traces of the two arithmetics are
   identical up to a singular-direction step (daqp.c:86-93); there the blocking test of auxiliary.c:284-287 compares components of the
   singular direction that are zero in exact arithmetic -- rounding noise of the size of dual_tol = 1e-12 -- with dual_tol, and one side
   removes one more row (and looks again) where the other already reports -1.  Not the fval bound of daqp.c:20-23.  DAQP_AMD_EXACT=1
   reproduces the reference's trace event for event. */
int daqp_batch_rechecked(const DAQPBatch *b);
void daqp_batch_set_recheck(DAQPBatch *b, int on);
int daqp_batch_recheck_ms(DAQPBatch *b, float *ms);
/* bytes of device memory held by the batch */
unsigned long long daqp_batch_device_bytes(const DAQPBatch *b);

/* ---- test / tuning hooks (used by tests/ and tools/; not needed by a caller of the solver) ---- */
/* per-problem add/remove event trace: `cap` ints per problem (+(id+1) add, -(id+1) remove; the last slot = event count); 0 = off */
int daqp_batch_enable_trace(DAQPBatch *b, int cap);
int daqp_batch_read_trace(DAQPBatch *b, int *host /* N*cap */);
/* cycle counters of the kernels' phases (32 x int64 per problem); on = 0 switches them off */
int daqp_batch_enable_profile(DAQPBatch *b, int on);
int daqp_batch_read_profile(DAQPBatch *b, long long *host /* N*32 */);
/* LDP of problem q as the reference stores it: M (m-ms) x n row-major, R^-1 packed upper, v, dupper, dlower, scaling; any may be NULL */
int daqp_batch_read_ldp(DAQPBatch *b, int q, c_float *M, c_float *R, c_float *v, c_float *dupper, c_float *dlower, c_float *scaling);

/* diagnostics */
const char *daqp_amd_last_error(void);
int daqp_amd_device_count(void);
const char *daqp_amd_version(void);
/* How a shape is solved: the library's plan (kernel family, register shape, fp32 image, workgroup kernel, setup kernel, LDS sizes, scratch
 * buffers: csrc/plan.hip.h) as ONE line of key=value pairs in a fixed key order, written to buf (at most len bytes, always terminated); returns
 * what snprintf would.  daqp_amd_describe_plan needs no device: it plans (N, n, m, ms, ns_max) under the current DAQP_AMD_* environment and the
 * device numbers given -- CU count, workgroups of the workgroup kernel per CU, whether its tiered variant accepts its LDS and how many of its
 * workgroups fit a CU (asked of the device only for shapes of the workgroup kernel; 0 otherwise) -- and a shape the library refuses gives
 * refused=<the text of daqp_amd_last_error>.  daqp_batch_describe writes the same line for a live batch, followed by cus= per_cu= tier_attr_ok=
 * per_cu_tier= as the batch was created with. */
int daqp_amd_describe_plan(int N, int n, int m, int ms, int ns_max, int cus, int per_cu, int tier_attr_ok, int per_cu_tier, char *buf, int len);
int daqp_batch_describe(const DAQPBatch *b, char *buf, int len);
/* always 0: the 16-problems-per-wavefront solve kernel of rounds 3-4 (slower than the default one) has been removed; kept for callers that asked */
int daqp_amd_has_tiny(void);

#ifdef __cplusplus
}
#endif
#endif /* DAQP_AMD_H */
