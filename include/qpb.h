/*
 * qpb.h -- batched dense QP solver for AMD MI355X (gfx950): the C-ABI.
 *
 * Plain C, plain pointers and sizes.  This is the drop-in boundary for the
 * reference's hot path (YangLingyuan/Embedded-qp-solver):
 *
 *   reference (one QP, CPU, fp64)                       replaced by
 *   --------------------------------------------------  ----------------------
 *   qp_solvers.h:4-16  gradient_descent_with_line_search qpb_ref_solve(QPB_REF_GD)
 *                      newton_method_with_line_search    qpb_ref_solve(QPB_REF_NEWTON)
 *                      admm (box = config.h:29-30)       qpb_ref_solve(QPB_REF_ADMM)
 *   test/qp_ref.py:35  solve_qp(P, q, G=0, h=0)          qpb_solve(m = 0)
 *   north_star active-set over (H, f, A, b)              qpb_solve(m > 0)
 *   ... with equality rows, solve_qp(P, q, G, h, A, b)    qpb_solve_eq
 *   ... differentiated (dl/dH, dl/df, dl/dA, dl/db)        qpb_solve_backward
 *   ... for a loss that reads lam too; the f / b tangent    qpb_solve_backward_dual
 *   ... the box solve (dl/dH, dl/df, dl/dlb, dl/dub)       qpb_solve_box_backward
 *   ... with ONE H and / or A for the whole batch          qpb_solve_shared, qpb_solve_shared_backward
 *   ... a box solve with ONE H for the whole batch         qpb_solve_box_shared, qpb_solve_box_shared_backward
 *   ... a box solve with that H factored ONCE              qpb_factor_box, qpb_solve_box_factored
 *   ... with that H and A factored ONCE                     qpb_factor_shared, qpb_solve_factored
 *   ... with two-sided rows bl <= A x <= bu                 qpb_solve_range
 *   ... two-sided rows beside variable bounds lb <= x <= ub   qpb_solve_range_box
 *   ... two-sided rows on the H and A factored once          qpb_solve_range_factored
 *   ... differentiated on the H and A factored once           qpb_factor_shared_backward, qpb_solve_factored_backward
 *   ... that, and the box backward, for a loss that reads lam  qpb_solve_factored_backward_dual, qpb_solve_box_backward_dual
 *   ... those two for T right-hand sides per QP in one launch    qpb_solve_factored_backward_multi, qpb_solve_box_backward_multi
 *   (absent from the reference: SURVEY.md §0)
 *   qp.h:19-24         quadratic_form_eval / _eval_grad  qpb_qf_eval
 *
 * The single-QP reference API itself (qp.h, qp_solvers.h, matrix_ops.h,
 * kmalloc.h, matrix_type.h) is re-exported, layout-compatible, by the compat
 * headers in include/compat/ on top of these entry points.
 *
 * Problem (per QP, fp64):   min 1/2 x^T H x + f^T x   s.t.   A x <= b
 *   H  n x n row-major, symmetric positive definite (the reference's P,
 *      qp.h:8-13; must be symmetric -- the kernels read the full matrix)
 *   f  n        (the reference's q)
 *   A  m x n row-major, b  m   (a box lb <= x <= ub is A = [I; -I], b = [ub; -lb])
 * Batched layout: QP k's arrays are contiguous at H + k*n*n, f + k*n,
 * A + k*m*n, b + k*m (array-of-structures, the reference's row-major
 * struct _matrix elements, matrix_type.h:20-23, one after another).
 *
 * Outputs:
 *   x       n per QP
 *   lam     m per QP: Lagrange multipliers, H x + f + A^T lam = 0, lam >= 0
 *   active  ceil(m/32) uint32 words per QP: bit i set <=> row i in the final
 *           active set
 *   status  one int32 per QP (qpb_status); never aborts the batch
 *   iters   one int32 per QP (active-set iterations), may be NULL
 *           (the other outputs do not depend on it)
 *
 * Every element of x, lam, active, status (and iters) of every QP is written
 * whatever the QP's status, and nothing outside them is.  A QP's outputs
 * depend on its own inputs only: not on the batch size, on its position, or on
 * the other QPs of the launch, failed and non-finite ones included.
 * What the outputs hold when status != QPB_OK (all kernels, qpb_solve_box
 * included; pinned by tests/test_gpu_status_contract.py):
 *   QPB_MAX_ITER    iters = max_iter.  lam, active: the dual iterate when the
 *                   cap was reached -- finite, lam >= 0, zero outside
 *                   `active`; x = -H^{-1} (f + A^T lam) for that lam, so
 *                   stationarity holds, primal feasibility in general not.
 *                   A QP that needs <= max_iter iterations is QPB_OK, with
 *                   the outputs of an uncapped solve bit for bit.
 *   QPB_INFEASIBLE  a zero row of A with b < 0 (found in the set-up,
 *                   iters = 0, lam = 0, active = 0), or a violated row that
 *                   depends linearly on the active ones and admits no step
 *                   (found by the iteration, 1 <= iters <= max_iter; lam,
 *                   active, x as for QPB_MAX_ITER).  Linearly dependent rows
 *                   of a feasible QP are not an error.
 *   QPB_NOT_SPD     iters = 0, lam = 0, active = 0; x is unspecified (it may
 *                   be non-finite).
 *   QPB_NUMERICAL   a row of A with a NaN entry, or whose squared norm is
 *                   not finite (found in the set-up: iters = 0, lam = 0,
 *                   active = 0, x unspecified), or a non-finite x after an
 *                   otherwise successful iteration.
 * Non-finite inputs: a NaN or +-Inf anywhere in H or f, or a NaN in a row of
 * A, gives a status other than QPB_OK (QPB_NOT_SPD takes precedence over
 * QPB_NUMERICAL, that over QPB_INFEASIBLE).  A NaN in b means the row is
 * absent, exactly as b = +inf (the box bounds of qpb_solve_box likewise).
 * feas_tol: row i counts as violated when a_i x - b_i > feas_tol (|a_i| + |b_i|).
 * Degenerate QPs (linearly dependent rows through the solution, duplicated
 * rows, rows that are tight with a zero multiplier, more than n tight rows, and
 * for qpb_solve_box a pinned variable lb_j == ub_j, whose two rows are both
 * tight) are ordinary inputs: QPB_OK, the same x, and every promise above.
 * lam >= 0 holds exactly, not within rounding: a multiplier that a tie in the
 * ratio test left a few ulp below zero is written as 0 and x is recovered
 * from the multipliers as written.  Which rows of a dependent tight set carry
 * the multipliers (and have their bit set) is unspecified; a row that is not
 * tight never has its bit set.  For a pinned variable lam_ub[j] - lam_lb[j] is
 * the one multiplier of x_j = lb_j, with either sign.  Pinned by
 * tests/test_gpu_degenerate.py on every kernel route.
 *
 * Equality rows (qpb_solve_eq; rows 0 .. meq-1 of A are a_i x = b_i).  The two
 * sentences above on what is written and on what a QP's outputs depend on
 * hold unchanged, and so does everything not restated here:
 *   lam             lam[i] of an equality has either sign; lam >= 0 is promised
 *                   for the rows >= meq only (so read at QPB_MAX_ITER too).
 *                   H x + f + A^T lam = 0 holds with the caller's A as given.
 *   dependent row   an equality that depends linearly on the equalities taken
 *                   before it (|d2|^2 <= 1e-24 |D_p|^2, the kernels' test; a
 *                   zero row, and any row once n independent ones are in) is
 *                   left out when |a_i x - b_i| <= feas_tol (|a_i| + |b_i|):
 *                   its bit stays clear, lam[i] = 0, and the solve goes on --
 *                   the residual cannot change later, the rows it depends on
 *                   are never dropped.  Which rows of a dependent set are kept
 *                   is unspecified; the set bits among the rows < meq number
 *                   rank(E).  With a residual outside the tolerance the QP is
 *                   QPB_INFEASIBLE (found by the iteration).
 *   zero row        an equality's zero row is infeasible iff
 *                   |b_i| > feas_tol (1 + |b_i|) (the set-up's rule with both
 *                   signs: iters = 0, lam = 0, active = 0).
 *   inequalities    a violated inequality that depends on the active rows with
 *                   no inequality among them to drop gives QPB_INFEASIBLE, as
 *                   before: an equality is never dropped.
 *   non-finite b    NaN or +-Inf in b_i of an equality gives QPB_NUMERICAL
 *                   from the set-up (iters = 0, lam = 0, active = 0): an
 *                   equality cannot be absent.  In a row >= meq a NaN still
 *                   means the row is absent.
 *   iterations      each equality taken or left out is one iteration; the
 *                   default max_iter stays 4 (n + m) + 8.
 *
 * All array pointers passed to qpb_solve / qpb_ref_solve are DEVICE pointers
 * (hipMalloc'd or torch CUDA tensors) and the call is asynchronous on
 * `stream` (a hipStream_t, NULL = default stream).  The *_host variants take
 * host pointers and synchronise.
 * Return value: 0 on success, a negative qpb_error on an invalid call.
 * Thread-safe: no global state besides the per-thread last-error string.
 */
#ifndef QPB_H
#define QPB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* qpb_version() reports "qpb MAJOR.MINOR (...)" */
#define QPB_VERSION_MAJOR 0
#define QPB_VERSION_MINOR 14

/* limits of this build's kernels: n <= 16, m <= 32 one QP per 16-lane DPP
 * row (qpb_gi.hip); n <= 32, m <= 64 one QP per wavefront (qpb_gi_wave.hip);
 * n <= 128, m <= 256 one QP per 512-thread workgroup, one workgroup per CU
 * walking the batch (qpb_gi_gram.hip) */
#define QPB_MAX_N 128
#define QPB_MAX_M 256
/* the reference-semantics replicas (qpb_ref_solve, qpb_matrix_invert) and the
 * compat solvers on them: n <= 1024 (above 128 the matrices live in a global
 * workspace, one 1024-thread workgroup per QP, qpb_ref.hip) */
#define QPB_REF_MAX_N 1024

typedef enum qpb_status {
	QPB_OK = 0,         /* KKT point found (within feas_tol) */
	QPB_MAX_ITER = 1,   /* iteration cap reached */
	QPB_NOT_SPD = 2,    /* Cholesky of H failed (pivot <= 0) */
	QPB_INFEASIBLE = 3, /* constraints proven infeasible */
	QPB_NUMERICAL = 4   /* non-finite result */
} qpb_status;

typedef enum qpb_error {
	QPB_SUCCESS = 0,
	QPB_ERR_INVALID_ARG = -1,
	QPB_ERR_UNSUPPORTED = -2, /* size outside this build's kernels */
	QPB_ERR_HIP = -3,         /* HIP runtime error (see qpb_last_error) */
	QPB_ERR_NO_DEVICE = -4
} qpb_error;

/* diagnostic flag (n <= 16, m <= 32, without QPB_FLAG_DIAG_WAVE): every QP k
 * reads the inputs of QP (k mod 512) -- kernel time without HBM latency
 * (outputs are still written for every k).  Ignored outside that size class
 * and by qpb_solve_box. */
#define QPB_FLAG_DIAG_L2 1
/* flag values 4 and 8 (round-2 diagnostic builds of the n <= 16 kernel) are
 * retired: accepted and ignored */
/* diagnostic flag (n <= 16): every QP k reads the inputs of QP (k mod 16384),
 * a 107 MB working set that stays Infinity-Cache resident across launches */
#define QPB_FLAG_DIAG_MALL 16

/* n in (16, 32], m <= 64 (BASELINE configs[4]): mixed precision -- the
 * active set is found in fp32 (factorisation and iterations), then x and lam
 * are refined in fp64 on the KKT system of that active set (fp32 factors,
 * fp64 residuals) and verified in fp64 (feasibility of every row, lam >= 0,
 * converged refinement).  QPs that fail verification are re-solved by the
 * fp64 kernel in a second launch, so results meet the fp64 path's bars.
 * Ignored outside that size class. */
#define QPB_FLAG_MIXED 32
/* diagnostic flag (with QPB_FLAG_MIXED): skip the fp64 re-solve; QPs that
 * would be re-solved keep status 100 (measures the re-solve fraction) */
#define QPB_FLAG_DIAG_NO_REDO 64

/* flag value 128 (the round-1 n <= 128 kernel) is retired: accepted and ignored */
/* diagnostic flag (n <= 16, m <= 32): solve with the one-QP-per-wavefront
 * kernel of the n <= 32 class (qpb_gi_wave.hip) instead of four QPs per
 * wavefront -- the group-size-1 endpoint of the lockstep model (DESIGN.md
 * §2.1); same answers within the parity bars, not a faster path */
#define QPB_FLAG_DIAG_WAVE 256

typedef struct qpb_desc {
	int32_t n;        /* variables, 1..QPB_MAX_N */
	int32_t m;        /* rows of A x <= b, 0..QPB_MAX_M (0: unconstrained) */
	int64_t batch;    /* number of QPs */
	int32_t max_iter; /* <= 0: default 4*(n+m)+8 */
	int32_t flags;    /* 0; QPB_FLAG_DIAG_L2 = diagnostic (see below) */
	double feas_tol;  /* <= 0: default 1e-10 (relative, per row) */
} qpb_desc;

/* Batched active-set solve (dual Goldfarb-Idnani method, one QP per 16-lane
 * row of a wavefront).  Device pointers; asynchronous on `stream`. */
int qpb_solve(const qpb_desc *desc, const double *H, const double *f,
	      const double *A, const double *b, double *x, double *lam,
	      uint32_t *active, int32_t *status, int32_t *iters, void *stream);

/* Same with host pointers (allocates device buffers, copies, synchronises). */
int qpb_solve_host(const qpb_desc *desc, const double *H, const double *f,
		   const double *A, const double *b, double *x, double *lam,
		   uint32_t *active, int32_t *status, int32_t *iters);

/* qpb_solve with equality rows: rows 0 .. meq-1 of A are a_i x = b_i, rows
 * meq .. m-1 are a_i x <= b_i (Goldfarb and Idnani's, and quadprog's, meq; for
 * solve_qp(P, q, G, h, A, b) stack [A; G], [b; h] and pass meq = rows(A)).
 * The method takes the equalities first and never drops them; their
 * multipliers are free in sign (the status contract above has the details).
 *   meq < 0, meq > m or desc->flags != 0   QPB_ERR_INVALID_ARG (the diagnostic
 *                   flags and QPB_FLAG_MIXED select nothing here)
 *   meq == 0        the call is qpb_solve: every shape, the same launches,
 *                   the same outputs bit for bit
 *   meq > 0         n <= 32 and m <= 64 (the EQ forms of qpb_gi.hip and
 *                   qpb_gi_wave.hip); above that QPB_ERR_UNSUPPORTED, which
 *                   is tested before meq > m.  The n <= 128 class
 *                   (qpb_gi_gram.hip) has no equality form yet: a follow-up.
 * Pointers, batch == 0 and a missing device as qpb_solve; qpb_desc is
 * unchanged, which is why meq is an argument. */
int qpb_solve_eq(const qpb_desc *desc, int32_t meq, const double *H,
		 const double *f, const double *A, const double *b, double *x,
		 double *lam, uint32_t *active, int32_t *status, int32_t *iters,
		 void *stream);

/* Same with host pointers, as qpb_solve_host. */
int qpb_solve_eq_host(const qpb_desc *desc, int32_t meq, const double *H,
		      const double *f, const double *A, const double *b,
		      double *x, double *lam, uint32_t *active, int32_t *status,
		      int32_t *iters);

/* The backward pass of qpb_solve / qpb_solve_eq: the vector-Jacobian product
 * of x*(H, f, A, b).  Given a solve's x, lam, active and status and the
 * cotangent gx = dl/dx (n per QP), one KKT solve per QP at FIXED active set:
 * W = the rows whose bit is set in `active`, A_W their rows,
 *
 *     [ H    A_W^T ] [ dx   ]     [ gx ]
 *     [ A_W   0    ] [ dlam ] = - [ 0  ]
 *
 *     gf = dx                             (n per QP)
 *     gH = 1/2 (dx x^T + x dx^T)          (n x n; symmetric bit for bit, as
 *                                          the H this header requires)
 *     gA_i = dlam_i x^T + lam_i dx^T      (m x n; row i in W, 0 otherwise)
 *     gb_i = -dlam_i                      (m;     row i in W, 0 otherwise)
 *
 * An equality row of qpb_solve_eq is simply a row whose bit is set and whose
 * multiplier may have either sign.  H is factored and the rows of
 * A_W L^{-T} are orthogonalised in row order; the Schur complement is never
 * formed.  This is the derivative at fixed active set:
 *   weakly active   a row with its bit set and lam_i = 0 counts as active, so
 *                   the result is one of the two one-sided derivatives.
 *   left-out row    a dependent equality the forward solve left out has its
 *                   bit clear and gets zero gradients.
 *   dependent row   the forward solve never marks one, a caller's own mask
 *                   can: a row whose part orthogonal to the set rows before it
 *                   has |d2|^2 <= 1e-24 |d|^2 (the kernels' test) is skipped,
 *                   dlam_i = 0: gb_i = 0 and gA_i = lam_i dx^T.  At most n rows
 *                   count; with more than n bits set the rows met after
 *                   them, in row order, are skipped in the same way.
 *   bits >= m       bits at positions >= m in the last word of `active` are
 *                   ignored.
 * desc is the forward call's: n, m and batch are used, max_iter and feas_tol
 * are ignored, flags must be 0.  Layouts are the forward's.
 *   required        H, x and gx; with m > 0 also A, lam and active.
 *   status          may be NULL: every QP then counts as QPB_OK.
 *   gH, gf, gA, gb  each may be NULL: that gradient is neither computed nor
 *                   stored; at least one must be given.  With m == 0, gA and
 *                   gb are ignored.
 * Every element of every non-NULL output of every QP is written, and nothing
 * else; a QP whose status is not QPB_OK gets zeros in all of them; a QP's
 * outputs depend on its own inputs only.
 * Errors, in order: the descriptor as qpb_solve; flags != 0
 * QPB_ERR_INVALID_ARG; n > 32 or m > 64 QPB_ERR_UNSUPPORTED; batch == 0
 * returns 0 before the pointers are looked at; missing pointers
 * QPB_ERR_INVALID_ARG; a missing device last.
 * Limits: n <= 16, m <= 32 runs four QPs per wavefront, the rest of n <= 32,
 * m <= 64 one QP per wavefront (qpb_kkt_bwd.hip).  The n <= 128 class needs a
 * workgroup-level kernel: a follow-up.  The backward of qpb_solve_box is
 * qpb_solve_box_backward, below.
 * Device pointers; asynchronous on `stream`. */
int qpb_solve_backward(const qpb_desc *desc, const double *H, const double *A,
		       const double *x, const double *lam,
		       const uint32_t *active, const int32_t *status,
		       const double *gx, double *gH, double *gf, double *gA,
		       double *gb, void *stream);

/* Same with host pointers, as qpb_solve_host. */
int qpb_solve_backward_host(const qpb_desc *desc, const double *H,
			    const double *A, const double *x,
			    const double *lam, const uint32_t *active,
			    const int32_t *status, const double *gx, double *gH,
			    double *gf, double *gA, double *gb);

/* One H and / or one A for the whole batch: the condensed plant model of an MPC
 * loop, or the learned weights of a QP layer, with f and b per QP.  `shared` is
 * a combination of the two bits; a shared operand is ONE matrix, read from one
 * copy (its QP stride is 0), the other is batched as everywhere else.  f, b and
 * every output are per QP in qpb_solve's layouts. */
#define QPB_SHARED_H 1 /* H is ONE n x n matrix for the whole batch */
#define QPB_SHARED_A 2 /* A is ONE m x n matrix for the whole batch */

/* qpb_solve_eq with a shared H and / or A.  Every output of every QP equals,
 * bit for bit, what qpb_solve_eq writes for that QP on materialised copies of
 * the shared operands: for every status of the contract above, and for NaN and
 * +-Inf inputs as well (the kernels are qpb_solve_eq's with other addresses:
 * the SH forms of qpb_gi.hip and qpb_gi_wave.hip; H is factored per QP).
 *   shared == 0     the call is qpb_solve_eq, with all its rules.
 *   m == 0          QPB_SHARED_A is ignored.
 * Errors, in order: the descriptor as qpb_solve; meq < 0, desc->flags != 0, a
 * bit of `shared` outside QPB_SHARED_H | QPB_SHARED_A, each
 * QPB_ERR_INVALID_ARG; with a shared operand, n > 32 or m > 64
 * QPB_ERR_UNSUPPORTED (with none, qpb_solve_eq's limit: meq > 0 above that
 * size); meq > m QPB_ERR_INVALID_ARG; batch == 0 returns 0 before the pointers
 * are looked at; missing pointers QPB_ERR_INVALID_ARG; a missing device last.
 * Limits: the two wavefront-level classes, n <= 16 with m <= 32 and n <= 32
 * with m <= 64.  Follow-ups: the n <= 128 Gram class (qpb_gi_gram.hip) has no
 * shared form (a shared-H qpb_solve_box is qpb_solve_box_shared).  This call factors H per QP on purpose,
 * so that bit-for-bit equality with qpb_solve_eq is its test; factoring a
 * shared H ONCE is qpb_factor_shared and qpb_solve_factored below.
 * Device pointers; asynchronous on `stream`. */
int qpb_solve_shared(const qpb_desc *desc, int32_t meq, int32_t shared,
		     const double *H, const double *f, const double *A,
		     const double *b, double *x, double *lam, uint32_t *active,
		     int32_t *status, int32_t *iters, void *stream);

/* Same with host pointers, as qpb_solve_host (a shared operand is one matrix). */
int qpb_solve_shared_host(const qpb_desc *desc, int32_t meq, int32_t shared,
			  const double *H, const double *f, const double *A,
			  const double *b, double *x, double *lam,
			  uint32_t *active, int32_t *status, int32_t *iters);

/* One H and one A for the whole batch, factored ONCE.  With both shared, the
 * set-up of every QP -- H = L L^T and D = A L^-T -- is the same numbers;
 * qpb_factor_shared computes them once into a factor buffer, and
 * qpb_solve_factored starts every QP from it: what is left per QP is
 * y = L^-1 f and s = b + D y.  An MPC loop factors once per model and solves
 * every tick; a QP layer factors once per forward pass.
 *
 * The buffer `fac` is self-contained: L, D, per row |a_r|^2, |a_r| and
 * |D_r|^2, a copy of A (the x recovery re-reads the active rows) and the two
 * findings of the set-up that do not depend on b, a non-SPD H and a NaN or
 * overflowing row of A.  The solve takes neither H nor A.  Its layout is
 * internal (csrc/qpb_factor.h) and belongs to one (n, m): a
 * buffer made for another shape is the caller's error, like any wrongly sized
 * array.  `fac` must be 16-byte aligned (hipMalloc's and torch's allocations
 * are), else QPB_ERR_INVALID_ARG. */

/* doubles a factor buffer for (n, m) holds; < 0: a qpb_error (n < 1, m < 0:
 * QPB_ERR_INVALID_ARG; n > 32 or m > 64: QPB_ERR_UNSUPPORTED).  Pure host
 * arithmetic. */
int64_t qpb_factor_doubles(int32_t n, int32_t m);

/* Factor ONE H (n x n) and ONE A (m x n; NULL with m == 0) into `fac`
 * (qpb_factor_doubles(n, m) doubles, device).  One small launch, asynchronous
 * on `stream`: a solve queued behind it on the same stream needs no host
 * synchronisation.  fstatus (one int32, device, may be NULL): QPB_OK,
 * QPB_NOT_SPD, or QPB_NUMERICAL for a row of A with a NaN entry or a non-finite
 * squared norm.  L and D are the values the unfactored kernels compute: each
 * class's factor kernel runs that class's own load and sweep.
 * Errors, in order: n < 1 or m < 0 QPB_ERR_INVALID_ARG; n > 32 or m > 64
 * QPB_ERR_UNSUPPORTED; H or fac missing, or A missing with m > 0,
 * QPB_ERR_INVALID_ARG; a missing device last. */
int qpb_factor_shared(int32_t n, int32_t m, const double *H, const double *A,
		      double *fac, int32_t *fstatus, void *stream);

/* Same with host pointers; fac (host) receives the buffer. */
int qpb_factor_shared_host(int32_t n, int32_t m, const double *H,
			   const double *A, double *fac, int32_t *fstatus);

/* qpb_solve_shared(shared = QPB_SHARED_H | QPB_SHARED_A) without the per-QP
 * set-up, on a buffer of qpb_factor_shared for (desc->n, desc->m).  The
 * contract is that call's: what is written for every status, a NaN b as an
 * absent row, the equality rows' rules (rows 0 .. meq-1), lam >= 0 exactly on
 * the rows >= meq, the default max_iter 4 (n + m) + 8, feas_tol per call; a
 * QP's outputs depend on its own f and b and on fac only, not on the batch
 * size or its position in the batch.  Two things differ.  The outputs are not
 * bit for bit qpb_solve_eq's: L and D are the same numbers, but s = b + D y is
 * formed from them and no longer inside the sweep, so x and lam differ by
 * rounding; on a non-degenerate QP status and active are the same.  And iters
 * may differ from the unfactored solve's.
 * A buffer whose H was not SPD gives every QP QPB_NOT_SPD, one with a NaN row
 * of A gives every QP QPB_NUMERICAL; a zero row of A is judged against each
 * QP's own b.  The buffer is only read: any number of solves, on any streams,
 * may use it at once.
 * Errors, in order: the descriptor as qpb_solve; meq < 0 or desc->flags != 0
 * QPB_ERR_INVALID_ARG; n > 32 or m > 64 QPB_ERR_UNSUPPORTED; meq > m
 * QPB_ERR_INVALID_ARG; batch == 0 returns 0 before the pointers are looked at;
 * missing pointers QPB_ERR_INVALID_ARG (fac, f, x and status always; b, lam and
 * active with m > 0; iters may be NULL); a missing device last.
 * The backward without the per-QP set-up is qpb_solve_factored_backward, below,
 * on a buffer of its own (qpb_factor_shared_backward).  Follow-up: a shared H
 * with a per-QP A.  Two-sided rows on the same buffer:
 * qpb_solve_range_factored, below.
 * Device pointers; asynchronous on `stream`. */
int qpb_solve_factored(const qpb_desc *desc, int32_t meq, const double *fac,
		       const double *f, const double *b, double *x, double *lam,
		       uint32_t *active, int32_t *status, int32_t *iters,
		       void *stream);

/* Same with host pointers (fac included: the call uploads it). */
int qpb_solve_factored_host(const qpb_desc *desc, int32_t meq,
			    const double *fac, const double *f, const double *b,
			    double *x, double *lam, uint32_t *active,
			    int32_t *status, int32_t *iters);

/* qpb_solve_backward with a shared H and / or A: the gradient of a shared
 * operand is ONE matrix, the sum over the batch.
 *   gf (B x n), gb (B x m)   qpb_solve_backward's, bit for bit.
 *   batched operand          its gradient is per QP (B x n x n, B x m x n),
 *                            qpb_solve_backward's bit for bit.
 *   shared H                 gH is n x n: 1/2 sum_k (dx_k x_k^T + x_k dx_k^T),
 *                            symmetric bit for bit.
 *   shared A                 gA is m x n: sum_k over the rows i in W_k of
 *                            (dlam_ki x_k^T + lam_ki dx_k^T).
 * A QP whose status is not QPB_OK contributes exactly 0 to a sum, even where
 * its x or lam holds NaN; lam outside W is ignored, whatever it holds.
 * Two passes: qpb_solve_backward's kernels without the summed gradients'
 * stores, then the sums on the fp64 matrix cores (qpb_kkt_bwd_sum.hip): one
 * wavefront per slice of the batch into its own slot of a workspace, and a
 * second kernel that adds the slots in order.  The slices are a function of
 * `batch` alone and there are no floating-point atomics: a summed output's
 * bits depend on the inputs and on (n, m, batch) only -- not on the stream, on
 * the state of the workspace cache or on the device's CU count.  They differ
 * from a sum of qpb_solve_backward's per-QP outputs by rounding (the order of
 * the additions) only.
 *   shared == 0     the call is qpb_solve_backward, with all its rules.
 *   m == 0          QPB_SHARED_A is ignored.
 *   gH, gf, gA, gb  each may be NULL, as in qpb_solve_backward.
 *   workspace       a summed gradient takes the per-(device, stream) scratch
 *                   buffer (qpb_release_workspaces): at most 1024 slots of
 *                   256 (ceil(n/16) + ceil(m/16)) ceil(n/16) doubles (24 MiB at
 *                   n = 32, m = 64 from 131 072 QPs on), plus B n doubles for
 *                   dx when gf is NULL, plus B m doubles for dlam when a
 *                   summed gA is wanted and gb is NULL.  It is retained, as the
 *                   other kernels' scratch is.
 * Errors, in order: the descriptor as qpb_solve; flags != 0 and a bit of
 * `shared` outside QPB_SHARED_H | QPB_SHARED_A QPB_ERR_INVALID_ARG; n > 32 or
 * m > 64 QPB_ERR_UNSUPPORTED; batch == 0 returns 0 before the pointers are
 * looked at; missing pointers QPB_ERR_INVALID_ARG; a missing device last.
 * Limits and follow-ups as qpb_solve_shared.
 * Device pointers; asynchronous on `stream`. */
int qpb_solve_shared_backward(const qpb_desc *desc, int32_t shared,
			      const double *H, const double *A, const double *x,
			      const double *lam, const uint32_t *active,
			      const int32_t *status, const double *gx, double *gH,
			      double *gf, double *gA, double *gb, void *stream);

/* Same with host pointers, as qpb_solve_host (a shared operand and its
 * gradient are one matrix). */
int qpb_solve_shared_backward_host(const qpb_desc *desc, int32_t shared,
				   const double *H, const double *A,
				   const double *x, const double *lam,
				   const uint32_t *active,
				   const int32_t *status, const double *gx,
				   double *gH, double *gf, double *gA,
				   double *gb);

/* qpb_solve_shared_backward for a loss l(x, lam) that also reads the
 * multipliers: the same KKT system at FIXED active set with a full right-hand
 * side,
 *
 *     [ H    A_W^T ] [ dx   ]     [ gx     ]
 *     [ A_W   0    ] [ dlam ] = - [ glam_W ]
 *
 * and qpb_solve_backward's output formulas on its solution, unchanged:
 * gf = dx, gH = 1/2 (dx x^T + x dx^T), gb_i = -dlam_i,
 * gA_i = dlam_i x^T + lam_i dx^T (i in W, else 0).  K is symmetric, so the same
 * call is the forward sensitivity (the tangent) of (x*, lam*) along a change
 * (df, db) of f and b: with gx = df and glam = -db, gf is dx* and -gb is dlam*.
 *   glam            B x m, in lam's layout and lam's sign convention
 *                   (H x + f + A^T lam = 0 with the caller's A): the signed lam
 *                   of qpb_solve_range needs nothing special.
 *   glam == NULL,   the call is qpb_solve_shared_backward: the same kernels,
 *   or m == 0       the same outputs bit for bit (shared == 0:
 *                   qpb_solve_backward).
 *   glam outside W  ignored, whatever it holds, NaN included.  So is the glam
 *                   of a row the orthogonalisation skips (a dependent row, a
 *                   row met after n independent ones): dlam_i = 0 there and
 *                   its equation is dropped, as in qpb_solve_backward.
 *   status          a QP whose status is not QPB_OK gets zeros in every output
 *                   and contributes exactly 0 to a sum, whatever its glam holds.
 *   shared          qpb_solve_shared_backward's: a shared operand's gradient is
 *                   ONE matrix, the sum over the batch; QPB_SHARED_A is ignored
 *                   at m == 0.
 *   required        H, x and gx; with m > 0 also A, lam and active.  status may
 *                   be NULL (every QP counts as QPB_OK).
 *   gH, gf, gA, gb  each may be NULL; at least one must be given.  With m == 0,
 *                   gA and gb are ignored.
 * Every element of every non-NULL output is written, and nothing else; a QP's
 * per-QP outputs depend on its own inputs only; gH is symmetric bit for bit.
 * With glam the kernels are the DU forms of qpb_solve_backward's
 * (qpb_kkt_bwd.hip): glam_W goes to the rows' positions, R^T w = glam is one
 * more substitution on the R the orthogonalisation left, Q w leaves the
 * projected right-hand side and w joins the right-hand side of the R solve.
 * Pass 2 and the workspace are qpb_solve_shared_backward's: the summed outputs'
 * bits depend on the inputs and on (n, m, batch) only.
 * Errors, in order: the descriptor as qpb_solve; flags != 0 and a bit of
 * `shared` outside QPB_SHARED_H | QPB_SHARED_A QPB_ERR_INVALID_ARG; n > 32 or
 * m > 64 QPB_ERR_UNSUPPORTED; batch == 0 returns 0 before the pointers are
 * looked at; missing pointers QPB_ERR_INVALID_ARG; a missing device last.
 * The factored form (glam on a qpb_factor_shared_backward buffer) is
 * qpb_solve_factored_backward_dual and the box form qpb_solve_box_backward_dual,
 * both below.  Follow-up: the n <= 128 Gram class.
 * Device pointers; asynchronous on `stream`. */
int qpb_solve_backward_dual(const qpb_desc *desc, int32_t shared,
			    const double *H, const double *A, const double *x,
			    const double *lam, const uint32_t *active,
			    const int32_t *status, const double *gx,
			    const double *glam, double *gH, double *gf,
			    double *gA, double *gb, void *stream);

/* Same with host pointers, as qpb_solve_host (a shared operand and its
 * gradient are one matrix). */
int qpb_solve_backward_dual_host(const qpb_desc *desc, int32_t shared,
				 const double *H, const double *A,
				 const double *x, const double *lam,
				 const uint32_t *active, const int32_t *status,
				 const double *gx, const double *glam,
				 double *gH, double *gf, double *gA,
				 double *gb);

/* Two-sided rows, the form OSQP and qpOASES state their constraints in:
 *   min 1/2 x^T H x + f^T x   s.t.   a_i x = bu_i            (rows i < meq; bl_i is not read)
 *                                    bl_i <= a_i x <= bu_i   (rows meq <= i < m)
 * Layouts are qpb_solve_eq's, with bl and bu each m per QP; `shared` is
 * qpb_solve_shared's bit set for H and A (bl and bu are always per QP).  A row
 * is taken natively -- one row of A L^-T and an orientation bit, in the RG forms
 * of qpb_gi.hip and qpb_gi_wave.hip -- where the pair a x <= bu, -a x <= -bl
 * would double m.  That pair rewrite through qpb_solve_eq is the specification
 * wherever this text is silent.
 * Outputs
 *   x, status, iters   as qpb_solve_eq.
 *   lam (m per QP)     signed, in OSQP's convention: H x + f + A^T lam = 0 with
 *                      the caller's A.  lam_i >= 0 exactly on a row active at
 *                      its upper bound, lam_i <= 0 exactly on a row active at
 *                      its lower bound (a tie's -eps of the side held is
 *                      written as 0 before the sign), free on an equality,
 *                      0 outside `active`.
 *   active             ceil(m/32) words per QP: bit i is set when row i is in
 *                      the final active set, on either side -- exactly the
 *                      array qpb_solve_backward and qpb_solve_shared_backward
 *                      read, with this lam.
 *   lower              ceil(m/32) words per QP, may be NULL: bit i is set when
 *                      row i is active at its LOWER bound.  lower is a subset
 *                      of active bit for bit; bits of rows < meq are always
 *                      clear.  It settles the side of a weakly active row
 *                      (lam_i = 0), which the sign of lam cannot.
 * Every element of every non-NULL output of every QP is written, whatever the
 * status, and a QP's outputs depend on its own inputs only.
 * Semantics
 *   absent bounds      a bu_i that is NaN or +inf is no upper bound, a bl_i that
 *                      is NaN or -inf no lower bound; with both absent the row
 *                      is absent.  bu_i = -inf or bl_i = +inf on a row >= meq
 *                      is an absent side as well: that is what the pair rewrite
 *                      makes of it (a row with b = -inf is never violated).  A
 *                      non-finite bu_i on a row < meq is QPB_NUMERICAL, as in
 *                      qpb_solve_eq.  bl or bu may be NULL: every row lacks
 *                      that side.
 *   tolerance          a row is violated on a side when the violation exceeds
 *                      feas_tol (|a_i| + beta_i), beta_i the larger of the
 *                      finite |bl_i| and |bu_i|: one threshold per row.
 *   crossed bounds     bl_i - bu_i above that threshold: QPB_INFEASIBLE from
 *                      the set-up (iters = 0, lam = 0, active = 0, lower = 0).
 *                      A negative width inside the threshold is a zero width.
 *   zero row of A      infeasible iff 0 lies outside [bl_i, bu_i] by more than
 *                      feas_tol (1 + |bound|): qpb_solve's rule, both signs.
 *   zero width         bl_i == bu_i on a row >= meq is legal: the row is taken
 *                      on whichever side is violated and may be dropped and
 *                      taken again, with the x of the meq form.  Sorting such
 *                      rows first and passing meq is the faster way to say it.
 *   QPB_MAX_ITER, QPB_INFEASIBLE found by the iteration: the contract's
 *                      sentences hold with the signed lam,
 *                      x = -H^-1 (f + A^T lam).
 *   default max_iter   4 (n + m) + 8.
 *   m == 0             the call is qpb_solve; `lower` has no words and is not
 *                      written.
 * Errors, in order: the descriptor as qpb_solve; meq < 0, desc->flags != 0, a bit
 * of `shared` outside QPB_SHARED_H | QPB_SHARED_A, each QPB_ERR_INVALID_ARG;
 * n > 32 or m > 64 QPB_ERR_UNSUPPORTED; meq > m QPB_ERR_INVALID_ARG; batch == 0
 * returns 0 before the pointers are looked at; missing pointers
 * QPB_ERR_INVALID_ARG (H, f, x and status always; with m > 0 A, lam, active and
 * at least one of bl and bu); a missing device last.
 * Limits: the two wavefront-level classes, n <= 16 with m <= 32 and n <= 32
 * with m <= 64.  Follow-ups: the n <= 128 Gram class, QPB_FLAG_MIXED and
 * qpb_solve_sections have no range form.  Rows beside variable bounds
 * lb <= x <= ub need no rows of the identity in A: qpb_solve_range_box, below.
 * With one H and A for every call of a loop, the set-up need not be repeated
 * per QP: qpb_solve_range_factored, below.
 * Device pointers; asynchronous on `stream`. */
int qpb_solve_range(const qpb_desc *desc, int32_t meq, int32_t shared,
		    const double *H, const double *f, const double *A,
		    const double *bl, const double *bu, double *x, double *lam,
		    uint32_t *active, uint32_t *lower, int32_t *status,
		    int32_t *iters, void *stream);

/* Same with host pointers, as qpb_solve_host (a shared operand is one matrix). */
int qpb_solve_range_host(const qpb_desc *desc, int32_t meq, int32_t shared,
			 const double *H, const double *f, const double *A,
			 const double *bl, const double *bu, double *x,
			 double *lam, uint32_t *active, uint32_t *lower,
			 int32_t *status, int32_t *iters);

/* Two-sided rows beside variable bounds, qpOASES's and OSQP's whole form:
 *   min 1/2 x^T H x + f^T x   s.t.   g_i x = bu_i            (rows i < meq; bl_i is not read)
 *                                    bl_i <= g_i x <= bu_i   (rows meq <= i < mg)
 *                                    lb_j <= x_j <= ub_j     (every variable j < n)
 * desc->m is mg, the number of general rows; mg = 0 is legal, and G may then be
 * NULL.  G is mg x n per QP (one matrix for the batch with QPB_SHARED_A), bl and
 * bu mg per QP, lb and ub n per QP.  Any of the four bound arrays may be NULL:
 * that side is absent everywhere; at least one must be given.
 * Specification: the materialised problem.  For every QP every output equals,
 * bit for bit, what qpb_solve_range(meq, shared) writes on m' = mg + n rows,
 * A' = [G; I_n], bl' = [bl; lb], bu' = [bu; ub] (a NULL half of bl' or bu' being
 * -inf or +inf), in that call's layouts with m':
 *   lam     mg + n per QP: the rows first, then variable j at mg + j, >= 0 at
 *           ub_j and <= 0 at lb_j
 *   active, lower   ceil((mg + n) / 32) words per QP, row i at bit i and
 *           variable j at bit mg + j; lower may be NULL
 * Every sentence of qpb_solve_range's contract therefore holds unchanged: what
 * is written at every status; NaN and +-inf bounds as absent sides; crossed
 * bounds (lb_j > ub_j beyond the threshold is QPB_INFEASIBLE from the set-up); a
 * pinned variable lb_j == ub_j as a zero-width row; lower a subset of active; a
 * QP's outputs depend on its own inputs only; the default max_iter is
 * 4 (n + m') + 8.  lam, active and lower go to qpb_solve_range_box_backward,
 * below, unchanged: the gradients without A' as well.
 * What the call saves is A' itself: the identity's rows are made in registers by
 * the BX forms of the range kernels (qpb_gi.hip, qpb_gi_wave.hip), neither
 * allocated nor filled by the caller, nor read by the kernel, nor gathered again
 * for x -- n n doubles per QP, 2 KB at n = 16.
 * Errors, in order: the descriptor as qpb_solve, with m = mg; meq < 0,
 * desc->flags != 0, a bit of `shared` outside QPB_SHARED_H | QPB_SHARED_A, each
 * QPB_ERR_INVALID_ARG; n > 32 or mg + n > 64 QPB_ERR_UNSUPPORTED; meq > mg
 * QPB_ERR_INVALID_ARG; batch == 0 returns 0 before the pointers are looked at;
 * missing pointers QPB_ERR_INVALID_ARG (H, f, x, lam, active and status always;
 * G with mg > 0; at least one of bl, bu, lb and ub); a missing device last.
 * Limits: the two wavefront-level classes by the materialised shape, n <= 16
 * with mg + n <= 32 and n <= 32 with mg + n <= 64.  Follow-ups: the n <= 128
 * Gram class, a factored form (with H and G shared, qpb_factor_shared on
 * [G; I] serves qpb_solve_range_factored today) and QPB_FLAG_MIXED.
 * Device pointers; asynchronous on `stream`. */
int qpb_solve_range_box(const qpb_desc *desc, int32_t meq, int32_t shared,
			const double *H, const double *f, const double *G,
			const double *bl, const double *bu, const double *lb,
			const double *ub, double *x, double *lam,
			uint32_t *active, uint32_t *lower, int32_t *status,
			int32_t *iters, void *stream);

/* Same with host pointers, as qpb_solve_host (a shared operand is one matrix). */
int qpb_solve_range_box_host(const qpb_desc *desc, int32_t meq, int32_t shared,
			     const double *H, const double *f, const double *G,
			     const double *bl, const double *bu,
			     const double *lb, const double *ub, double *x,
			     double *lam, uint32_t *active, uint32_t *lower,
			     int32_t *status, int32_t *iters);

/* The backward of qpb_solve_range_box: the gradients of a loss l with respect to
 * H, f, G and the four bound arrays from gx = dl/dx and, where it is not NULL,
 * glam = dl/dlam, without A' = [G; I] in memory.  desc->m is mg, as in the
 * forward; lam, active, lower and glam are in that call's layouts on
 * m' = mg + n rows (row i at i, variable j at mg + j, ceil(m' / 32) words).
 * `shared` is the QPB_SHARED_H | QPB_SHARED_A bit set.  There is no meq: an
 * equality row is a row whose bit is set in `active` and clear in `lower`.
 * Specification: the materialised problem.  Let (gH', gf', gA', gb') be what
 * qpb_solve_backward_dual(shared, H, A' = [G; I], x, lam, active, status, gx,
 * glam) writes on m' rows (with glam == NULL that call is
 * qpb_solve_shared_backward, with shared == 0 qpb_solve_backward).  Then, bit
 * for bit:
 *   gH, gf   gH' and gf'; a shared H gives ONE n x n matrix, symmetric bit for bit
 *   gG       rows 0 .. mg-1 of gA': mg x n per QP, or with QPB_SHARED_A ONE
 *            mg x n matrix, the first mg rows of that call's summed gA'.  The
 *            identity rows' gradient is neither computed for storing nor stored.
 *   gbl, gbu (mg per QP), glb, gub (n per QP)   gb' routed by the `lower` bits:
 *            an element goes to the lower-bound array where the row's bit is
 *            set and to the upper-bound array otherwise; the other array gets
 *            +0.0 (selected, never multiplied).  A `lower` bit on a row whose
 *            `active` bit is clear routes that row's zero.
 * Every sentence of qpb_solve_backward's contract therefore holds unchanged:
 * weakly active and dependent rows (a row of G equal to +-e_j beside variable
 * j's bit is the natural dependent row; the test runs in row order, so the skip
 * lands on the variable), masks with more than n bits, bits >= m' ignored, lam
 * and glam outside the active set ignored (NaN included), zeros for a QP whose
 * status is not QPB_OK and its exact-zero share of a sum, status NULL, every
 * element of every non-NULL output written and nothing else, the summed outputs'
 * bits a function of the inputs and (n, mg, batch) only.
 * mg == 0: G may be NULL and gG is ignored.  Each of the seven outputs may be
 * NULL; at least one must be given.  lower may be NULL only when gbl and glb
 * both are: every routed element then goes to the upper arrays.
 * The kernels are the BX forms of qpb_solve_backward's (qpb_kkt_bwd.hip), in the
 * class of the materialised shape: a unit row is made in registers where the
 * other forms load a row of A, and nothing differs from the factorisation on.
 * A summed gG or gH takes the second pass of qpb_solve_shared_backward over the
 * rows of G (workspace: the slots, B n doubles where gf is NULL, B mg where gG
 * is summed).
 * Errors, in order: the descriptor as qpb_solve, with m = mg; desc->flags != 0 or
 * a bit of `shared` outside QPB_SHARED_H | QPB_SHARED_A, QPB_ERR_INVALID_ARG;
 * n > 32 or mg + n > 64 QPB_ERR_UNSUPPORTED; batch == 0 returns 0 before the
 * pointers are looked at; missing pointers QPB_ERR_INVALID_ARG (H, x, lam,
 * active and gx always; G with mg > 0; lower as above; one output); a missing
 * device last.
 * Follow-ups: a tangent helper, a form on a factor buffer, T directions per QP
 * and the n <= 128 Gram class.
 * Device pointers; asynchronous on `stream`. */
int qpb_solve_range_box_backward(const qpb_desc *desc, int32_t shared,
				 const double *H, const double *G,
				 const double *x, const double *lam,
				 const uint32_t *active, const uint32_t *lower,
				 const int32_t *status, const double *gx,
				 const double *glam, double *gH, double *gf,
				 double *gG, double *gbl, double *gbu,
				 double *glb, double *gub, void *stream);

/* Same with host pointers, as qpb_solve_backward_host (a shared operand and its
 * gradient are one matrix). */
int qpb_solve_range_box_backward_host(const qpb_desc *desc, int32_t shared,
				      const double *H, const double *G,
				      const double *x, const double *lam,
				      const uint32_t *active,
				      const uint32_t *lower,
				      const int32_t *status, const double *gx,
				      const double *glam, double *gH,
				      double *gf, double *gG, double *gbl,
				      double *gbu, double *glb, double *gub);

/* qpb_solve_range(shared = QPB_SHARED_H | QPB_SHARED_A) without the per-QP
 * set-up: two-sided rows on a buffer of qpb_factor_shared for (desc->n,
 * desc->m) -- the buffer qpb_solve_factored takes, unchanged, so one buffer
 * serves both calls, in any order and at once.  This is the MPC call: the plant
 * model H and A is factored once, the state and rate limits are two-sided
 * rows, and every tick solves with its own f, bl and bu.
 * The contract is qpb_solve_range's on the H and A the buffer was made from,
 * every sentence of it: the signed lam, `active` as the backward reads it,
 * `lower` (may be NULL), NaN and +-inf bounds as absent sides, bl or bu NULL,
 * one threshold per row with the larger finite |bound|, crossed bounds and a
 * zero row of A judged against each QP's own bl and bu, zero width, the
 * equality rows' rules, and what is written at every status; a QP's outputs
 * depend on its own f, bl and bu and on fac only.  The thresholds are the
 * unfactored call's bit for bit: they are formed from the |a_r| the buffer
 * stores.  Two things differ, the two that qpb_solve_factored has against
 * qpb_solve_shared: x and lam may differ by rounding (s = b + D y is formed from
 * the stored L and D; a row whose only bound is the lower one takes the negated
 * stored row of D), and iters may differ.  On a non-degenerate QP status,
 * active and lower are the same.
 * A buffer whose H was not SPD gives every QP QPB_NOT_SPD, one with a NaN row
 * of A gives every QP QPB_NUMERICAL; in both cases iters = 0, lam = 0,
 * active = 0 and lower = 0.  The buffer is only read.
 *   m == 0   the call is qpb_solve_factored, its outputs bit for bit; `lower`
 *            has no words and is not written.
 * Errors, in order: the descriptor as qpb_solve; meq < 0 or desc->flags != 0
 * QPB_ERR_INVALID_ARG; n > 32 or m > 64 QPB_ERR_UNSUPPORTED; meq > m
 * QPB_ERR_INVALID_ARG; batch == 0 returns 0 before the pointers are looked at;
 * missing pointers QPB_ERR_INVALID_ARG (fac, f, x and status always; with m > 0
 * lam, active and at least one of bl and bu; lower and iters may be NULL); a fac
 * that is not 16-byte aligned QPB_ERR_INVALID_ARG; a missing device last.
 * Limits as qpb_solve_factored.  The backward of this call is
 * qpb_solve_shared_backward on H and A, or, without the per-QP set-up,
 * qpb_solve_factored_backward on the backward's own buffer, below.  Follow-up:
 * the Gram class.
 * Device pointers; asynchronous on `stream`. */
int qpb_solve_range_factored(const qpb_desc *desc, int32_t meq,
			     const double *fac, const double *f,
			     const double *bl, const double *bu, double *x,
			     double *lam, uint32_t *active, uint32_t *lower,
			     int32_t *status, int32_t *iters, void *stream);

/* Same with host pointers (fac included: the call uploads it). */
int qpb_solve_range_factored_host(const qpb_desc *desc, int32_t meq,
				  const double *fac, const double *f,
				  const double *bl, const double *bu, double *x,
				  double *lam, uint32_t *active,
				  uint32_t *lower, int32_t *status,
				  int32_t *iters);

/* The backward of a solve on one H and one A, factored ONCE.
 * qpb_solve_shared_backward(shared = QPB_SHARED_H | QPB_SHARED_A) factors the
 * same H and re-forms A_W L^-T for every QP; everything its kernels compute from
 * H and A alone is the same numbers for the whole batch.
 * qpb_factor_shared_backward computes them once into a buffer of the backward's
 * own, `bfac`, and qpb_solve_factored_backward starts every QP from it.
 *
 * `bfac` is NOT qpb_factor_shared's `fac`: it is written by the backward
 * kernels' own set-up (the forward's D of the n <= 16 class comes from another
 * sweep), and it holds L, 1 / L_kk, D = A L^-T and, in the
 * n <= 16 class, the sweep's elimination multipliers -- neither H nor A: no
 * output reads them.  What remains per QP is the unfactored kernel's operations
 * on the unfactored kernel's numbers, so the outputs are that call's bit for
 * bit.  The layout is internal (csrc/qpb_factor.h) and belongs
 * to one (n, m): a buffer made for another shape, or a forward `fac` passed
 * here, is the caller's error, like any wrongly sized array.  `bfac` must be
 * 16-byte aligned (hipMalloc's and torch's allocations are), else
 * QPB_ERR_INVALID_ARG. */

/* doubles a backward buffer for (n, m) holds; < 0: a qpb_error (n < 1, m < 0:
 * QPB_ERR_INVALID_ARG; n > 32 or m > 64: QPB_ERR_UNSUPPORTED).  Pure host
 * arithmetic. */
int64_t qpb_factor_backward_doubles(int32_t n, int32_t m);

/* Factor ONE H (n x n) and ONE A (m x n; NULL with m == 0) into `bfac`
 * (qpb_factor_backward_doubles(n, m) doubles, device), every element of which
 * is written.  One small launch, asynchronous on `stream`: a solve queued behind
 * it on the same stream needs no host synchronisation.  fstatus (one int32,
 * device, may be NULL): QPB_OK, or QPB_NOT_SPD when a pivot is not a positive
 * finite number.  The rows of A are not judged: the backward never judges them.
 * Errors, in order: n < 1 or m < 0 QPB_ERR_INVALID_ARG; n > 32 or m > 64
 * QPB_ERR_UNSUPPORTED; H or bfac missing, or A missing with m > 0,
 * QPB_ERR_INVALID_ARG; a bfac that is not 16-byte aligned QPB_ERR_INVALID_ARG;
 * a missing device last. */
int qpb_factor_shared_backward(int32_t n, int32_t m, const double *H,
			       const double *A, double *bfac, int32_t *fstatus,
			       void *stream);

/* Same with host pointers; bfac (host) receives the buffer. */
int qpb_factor_shared_backward_host(int32_t n, int32_t m, const double *H,
				    const double *A, double *bfac,
				    int32_t *fstatus);

/* qpb_solve_shared_backward(shared = QPB_SHARED_H | QPB_SHARED_A) without H and
 * A, on a buffer of qpb_factor_shared_backward for (desc->n, desc->m).  Every
 * non-NULL output equals, bit for bit, what that call writes for the same x,
 * lam, active, status and gx on the H and A the buffer was made from.  Its
 * contract, restated:
 *   gH (n x n)      ONE matrix, 1/2 sum_k (dx_k x_k^T + x_k dx_k^T) over the
 *                   batch, symmetric bit for bit.
 *   gA (m x n)      ONE matrix, the sum over the batch of qpb_solve_backward's
 *                   per-QP gA.
 *   gf (B x n), gb (B x m)   per QP, qpb_solve_backward's.
 *   gH, gf, gA, gb  each may be NULL; at least one must be given.
 *   status          may be NULL: every QP counts as QPB_OK.  A QP whose status
 *                   is not QPB_OK gets zeros in gf and gb and contributes
 *                   exactly 0 to the sums, even where its x or lam holds NaN.
 *   lam, active     lam outside W is ignored, whatever it holds; bits >= m are
 *                   ignored.  Weakly active rows, dependent rows and masks with
 *                   more than n bits are treated as in qpb_solve_backward.
 *   m == 0          gA and gb are ignored.
 *   workspace       what qpb_solve_shared_backward takes with both operands
 *                   shared: the slots, B n doubles when gf is NULL, B m doubles
 *                   when gA is wanted and gb is NULL.
 *   reproducible    the summed outputs' bits depend on the inputs and on
 *                   (n, m, batch) only, as qpb_solve_shared_backward's.
 * A buffer whose H was not SPD gives zeros in every non-NULL output of every
 * QP, whatever `status` says (x and the lam in W finite, as for any QP that
 * counts as QPB_OK).  The buffer is only read: any number of calls, on any
 * streams, may use it at once.
 * Pass 1 is the factored forms of qpb_kkt_bwd.hip -- no Cholesky, no sweep and
 * no per-row substitution per QP -- and pass 2 the sums of
 * qpb_solve_shared_backward, unchanged.
 * Errors, in order: the descriptor as qpb_solve; desc->flags != 0
 * QPB_ERR_INVALID_ARG; n > 32 or m > 64 QPB_ERR_UNSUPPORTED; batch == 0 returns
 * 0 before the pointers are looked at; missing pointers QPB_ERR_INVALID_ARG
 * (bfac, x and gx always; lam and active with m > 0; at least one output); a
 * bfac that is not 16-byte aligned QPB_ERR_INVALID_ARG; a missing device last.
 * Limits as qpb_solve_factored.  Follow-ups: the Gram class, a shared H with a
 * per-QP A, a factored qpb_solve_box_backward.
 * Device pointers; asynchronous on `stream`. */
int qpb_solve_factored_backward(const qpb_desc *desc, const double *bfac,
				const double *x, const double *lam,
				const uint32_t *active, const int32_t *status,
				const double *gx, double *gH, double *gf,
				double *gA, double *gb, void *stream);

/* Same with host pointers (bfac included: the call uploads it). */
int qpb_solve_factored_backward_host(const qpb_desc *desc, const double *bfac,
				     const double *x, const double *lam,
				     const uint32_t *active,
				     const int32_t *status, const double *gx,
				     double *gH, double *gf, double *gA,
				     double *gb);

/* qpb_solve_backward_dual(shared = QPB_SHARED_H | QPB_SHARED_A) on a buffer of
 * qpb_factor_shared_backward, without H and A: qpb_solve_factored_backward for a
 * loss l(x, lam) that also reads the multipliers, and the f / b tangent on the
 * path that factors once (gx = df, glam = -db: gf is dx*, -gb is dlam*).
 *   glam            B x m, in lam's layout and sign convention, as
 *                   qpb_solve_backward_dual's.
 *   outputs         every non-NULL output equals BIT FOR BIT what
 *                   qpb_solve_backward_dual writes with both operands shared,
 *                   for the same x, lam, active, status, gx and glam on the H
 *                   and A the buffer was made from.
 *   glam == NULL,   the call is qpb_solve_factored_backward: the same launches,
 *   or m == 0       the same outputs bit for bit.
 *   glam outside W  ignored, whatever it holds, NaN included; so is the glam of
 *                   a row the orthogonalisation skips and of a QP whose status
 *                   is not QPB_OK (zeros everywhere, exactly 0 to the sums).
 * Everything else is qpb_solve_factored_backward's: a buffer whose H was not
 * SPD gives zeros everywhere, the workspace, the reproducibility of the sums,
 * the buffer only read, bfac 16-byte aligned.  The layout of the buffer does
 * not change: R and Q are per QP and come from the orthogonalisation.
 * Pass 1 is the DU forms of the factored forms of qpb_kkt_bwd.hip -- the
 * factored load and u recursion, then qpb_solve_backward_dual's four steps
 * after the orthogonalisation, the same code -- and pass 2 is unchanged.
 * Errors, in order, are qpb_solve_factored_backward's; glam is never required.
 * Device pointers; asynchronous on `stream`. */
int qpb_solve_factored_backward_dual(const qpb_desc *desc, const double *bfac,
				     const double *x, const double *lam,
				     const uint32_t *active,
				     const int32_t *status, const double *gx,
				     const double *glam, double *gH, double *gf,
				     double *gA, double *gb, void *stream);

/* Same with host pointers (bfac included: the call uploads it). */
int qpb_solve_factored_backward_dual_host(const qpb_desc *desc,
					  const double *bfac, const double *x,
					  const double *lam,
					  const uint32_t *active,
					  const int32_t *status,
					  const double *gx, const double *glam,
					  double *gH, double *gf, double *gA,
					  double *gb);

/* Box-constrained batched solve, lb <= x <= ub: the constraint class of the
 * reference's admm() (qp_solvers.c:146-319, bounds config.h:29-30), solved
 * exactly with A = [I; -I], b = [ub; -lb] kept implicit (qpb_gi_box.hip for
 * n <= 16, four QPs per wavefront; the BOX form of qpb_gi_wave.hip for
 * 16 < n <= 32, one QP per wavefront; the BOX form of qpb_gi_gram.hip for
 * 32 < n <= 128, one QP per workgroup).  Replaces admm()'s box QP the way
 * qpb_solve replaces the dense path.  desc->n <= QPB_MAX_N (128;
 * QPB_ERR_UNSUPPORTED above); desc->m must be 2n.  lb, ub: B x n, either may be NULL,
 * and +-inf entries are absent bounds.  lam: B x 2n (upper bounds' multipliers
 * first, then the lower bounds'); active: B x ceil(2n/32) uint32 words in the
 * same row order -- ONE word per QP for n <= 16, TWO for 16 < n <= 32, up to
 * EIGHT at n = 128 (size it as qpb_solve's ceil(m/32) with m = 2n; the n > 16
 * kernels write every word);
 * x, status, iters as qpb_solve.  Device pointers; asynchronous on `stream`. */
int qpb_solve_box(const qpb_desc *desc, const double *H, const double *f,
		  const double *lb, const double *ub, double *x, double *lam,
		  uint32_t *active, int32_t *status, int32_t *iters, void *stream);

/* The backward pass of qpb_solve_box: the vector-Jacobian product of
 * x*(H, f, lb, ub).  Given a box solve's x, active and status and the cotangent
 * gx = dl/dx (n per QP), the KKT system of qpb_solve_backward at FIXED active
 * set with the rows of A = [I; -I] as unit vectors.  Variable j is fixed when
 * its upper-bound bit (j) or its lower-bound bit (n + j) is set in `active`,
 * F are the free variables:
 *
 *     dx_fixed = 0,   H_FF dx_F = -gx_F,   r = gx + H dx   (zero on F)
 *
 *     gf  = dx                            (n per QP)
 *     gH  = 1/2 (dx x^T + x dx^T)         (n x n; symmetric bit for bit)
 *     gub_j = r_j  if the upper bound of j is active, else 0           (n)
 *     glb_j = r_j  if the lower bound of j is active and the upper
 *                  is not, else 0                                      (n)
 *
 * One Cholesky of H with the fixed variables' rows and columns replaced by
 * the identity, two triangular solves and one matrix-vector product per QP.
 * lam, f, lb and ub are not arguments: no output depends on them.  These are
 * qpb_solve_backward's gradients on the same QP written with A = [I; -I],
 * b = [ub; -lb]: gub = gb[:n], glb = -gb[n:].  At fixed active set:
 *   weakly active   a set bit counts as active whatever its multiplier, so
 *                   the result is one of the two one-sided derivatives.
 *   both bits set   (a variable pinned by lb = ub, or a caller's own mask)
 *                   the upper bound counts and the lower bound gets 0:
 *                   qpb_solve_backward's row-order rule for a dependent row.
 *   all fixed       gf = 0, gH = 0 and r = gx.
 *   none fixed      dx = -H^{-1} gx and glb = gub = 0.
 *   bits >= 2n      bits at positions >= 2n in the last word of `active` are
 *                   ignored.
 * desc is the forward qpb_solve_box call's: n, m (which must be 2n) and batch
 * are used, max_iter and feas_tol are ignored, flags must be 0.  x and active
 * (ceil(2n/32) words per QP; bits 0..n-1 the upper bounds, n..2n-1 the lower
 * bounds) in qpb_solve_box's layouts.
 *   required        H, x, active and gx.
 *   status          may be NULL: every QP then counts as QPB_OK.
 *   gH, gf, glb, gub  each may be NULL: that gradient is neither computed nor
 *                   stored; at least one must be given.
 * Every element of every non-NULL output of every QP is written, and nothing
 * else; a QP whose status is not QPB_OK gets zeros in all of them; a QP's
 * outputs depend on its own inputs only.
 * Errors, in order: the descriptor as qpb_solve_box (m != 2n
 * QPB_ERR_INVALID_ARG); flags != 0 QPB_ERR_INVALID_ARG; n > 32
 * QPB_ERR_UNSUPPORTED; batch == 0 returns 0 before the pointers are looked
 * at; missing pointers QPB_ERR_INVALID_ARG; a missing device last.
 * Limits: n <= 16 runs four QPs per wavefront, 16 < n <= 32 one QP per
 * wavefront (qpb_kkt_bwd_box.hip).  The n in (32, 128] class of qpb_solve_box
 * needs the workgroup-level kernel that qpb_solve_backward also lacks: a
 * follow-up.
 * Device pointers; asynchronous on `stream`. */
int qpb_solve_box_backward(const qpb_desc *desc, const double *H,
			   const double *x, const uint32_t *active,
			   const int32_t *status, const double *gx, double *gH,
			   double *gf, double *glb, double *gub, void *stream);

/* Same with host pointers, as qpb_solve_host. */
int qpb_solve_box_backward_host(const qpb_desc *desc, const double *H,
				const double *x, const uint32_t *active,
				const int32_t *status, const double *gx,
				double *gH, double *gf, double *glb,
				double *gub);

/* qpb_solve_box with ONE H (n x n) for the whole batch, read from one copy (its
 * QP stride is 0): an MPC loop's condensed Hessian with input bounds, or a QP
 * layer's learned weight with a box.  f, lb, ub and every output are per QP in
 * qpb_solve_box's layouts, at every shape it takes (n <= 128, m = 2n).
 * Every output of every QP equals, bit for bit, what qpb_solve_box writes for
 * that QP on B materialised copies of H: for every status of the contract
 * above, and for NaN and +-Inf inputs as well (the kernels are qpb_solve_box's
 * with another address: the SH forms of qpb_gi_box.hip and of the BOX kernels
 * of qpb_gi_wave.hip and qpb_gi_gram.hip; H is factored per QP).  H is only
 * read.  The flags select nothing, as there.
 * Errors, in order, are qpb_solve_box's: the descriptor; m != 2n
 * QPB_ERR_INVALID_ARG; batch == 0 returns 0 before the pointers are looked at;
 * missing H, f, x, lam, active or status QPB_ERR_INVALID_ARG (lb, ub and iters
 * may be NULL); a missing device last.
 * This call factors H per QP on purpose (bit-for-bit equality with
 * qpb_solve_box is its test); with the shared H factored ONCE, so that L and
 * L^-T are the same numbers for every QP: qpb_factor_box and
 * qpb_solve_box_factored, below (n <= 32).  General rows beside a box, with
 * one H or one per QP: qpb_solve_range_box, above (n <= 32, mg + n <= 64).
 * Device pointers; asynchronous on `stream`. */
int qpb_solve_box_shared(const qpb_desc *desc, const double *H, const double *f,
			 const double *lb, const double *ub, double *x,
			 double *lam, uint32_t *active, int32_t *status,
			 int32_t *iters, void *stream);

/* Same with host pointers, as qpb_solve_host (H is one matrix). */
int qpb_solve_box_shared_host(const qpb_desc *desc, const double *H,
			      const double *f, const double *lb,
			      const double *ub, double *x, double *lam,
			      uint32_t *active, int32_t *status, int32_t *iters);

/* qpb_solve_box_backward with ONE H (n x n): the gradient of the shared H is
 * ONE matrix, the sum over the batch.
 *   gf, glb, gub (B x n)   qpb_solve_box_backward's, bit for bit.
 *   gH (n x n)             1/2 sum_k (dx_k x_k^T + x_k dx_k^T), symmetric bit
 *                          for bit.
 * A QP whose status is not QPB_OK contributes exactly 0 to the sum, even where
 * its x holds NaN.  Each output may be NULL, at least one must be given; status
 * may be NULL (every QP then counts as QPB_OK).  The rules of
 * qpb_solve_box_backward at fixed active set (weakly active, both bits set,
 * bits >= 2n) hold unchanged.
 * Two passes, as in qpb_solve_shared_backward.  Pass 1 is the SH forms of
 * qpb_kkt_bwd_box.hip launched without gH -- the factorisation of H masked by
 * each QP's fixed variables differs per QP and stays per QP -- with dx going to
 * gf or, when gf is NULL, to the workspace.  Pass 2 is that call's batch sum on
 * the fp64 matrix cores (qpb_kkt_bwd_sum.hip), unchanged, with m = 0: once on
 * the whole batch, also when pass 1 walks it in chunks.
 *   workspace       sum_plan(B).slots * sum_slot_doubles(n, 0) doubles
 *                   (csrc/qpb_route.h), plus B n when gf is NULL; cached per
 *                   stream like every workspace.  gH NULL: no pass 2 and no
 *                   workspace.
 *   reproducible    no atomics: the bits of gH depend on the inputs and on
 *                   (n, batch) only, whatever the stream, the workspace's
 *                   history or the device.
 * Errors, in order, are qpb_solve_box_backward's: the descriptor (m != 2n
 * QPB_ERR_INVALID_ARG); flags != 0 QPB_ERR_INVALID_ARG; n > 32
 * QPB_ERR_UNSUPPORTED; batch == 0 returns 0 before the pointers are looked at;
 * missing pointers QPB_ERR_INVALID_ARG (H, x, active and gx; at least one
 * output); a missing device last.
 * The outputs of qpb_solve_box_factored, below, go to this call with the H the
 * buffer was made from.
 * Follow-ups: the box backward above n = 32; a factored box backward.
 * Device pointers; asynchronous on `stream`. */
int qpb_solve_box_shared_backward(const qpb_desc *desc, const double *H,
				  const double *x, const uint32_t *active,
				  const int32_t *status, const double *gx,
				  double *gH, double *gf, double *glb,
				  double *gub, void *stream);

/* Same with host pointers (H and gH are one matrix each). */
int qpb_solve_box_shared_backward_host(const qpb_desc *desc, const double *H,
				       const double *x, const uint32_t *active,
				       const int32_t *status, const double *gx,
				       double *gH, double *gf, double *glb,
				       double *gub);

/* qpb_solve_box_backward and qpb_solve_box_shared_backward for a loss l(x, lam)
 * that also reads the multipliers: the KKT system of qpb_solve_backward_dual on
 * A = [I; -I] at FIXED active set, with the unit rows eliminated.  There glam
 * is a prescribed dx on the fixed variables.  S: the fixed variables, F: the
 * free ones,
 *
 *     d_j = -glam[j]        the upper bit of j is set
 *     d_j = +glam[n + j]    only the lower bit of j is set
 *     d_j = 0               j is free
 *     dx_S = d_S (exactly those bits)      H_FF dx_F = -gx_F - H_FS d_S
 *     r = gx + H dx
 *
 * and the box backward's output formulas, unchanged: gf = dx,
 * gH = 1/2 (dx x^T + x dx^T) (symmetric bit for bit), gub_j = r_j on an active
 * upper bound, glb_j = r_j on a lower bound that is active without the upper.
 * The same call is the tangent of (x*, lam*) along (df, dlb, dub): with gx = df,
 * glam[:n] = -dub and glam[n:] = +dlb, gf is dx*, -gub is dlam* of the upper
 * bounds and +glb of the lower ones.
 *   glam            B x 2n in qpb_solve_box's lam layout: the upper bounds'
 *                   entries, then the lower bounds'.
 *   shared          0: H is B x n x n and gH per QP, as qpb_solve_box_backward.
 *                   QPB_SHARED_H: H is n x n and gH ONE n x n sum, exactly as
 *                   qpb_solve_box_shared_backward -- pass 1 without the gH
 *                   stores, pass 2 with m = 0, the same workspace, the same
 *                   reproducible bits; gf, glb and gub are the unshared call's
 *                   bit for bit.
 *   both bits set   the upper bound counts; the lower row is the dependent one:
 *                   its glam is ignored and glb_j = 0 (qpb_solve_box_backward's
 *                   rule).
 *   ignored         the glam of a bit that is clear, of bits >= 2n and of a QP
 *                   whose status is not QPB_OK, whatever it holds, NaN included.
 *                   Such a QP gets zeros and contributes exactly 0 to the sum.
 *   glam == NULL    the call is qpb_solve_box_backward (shared == 0) or
 *                   qpb_solve_box_shared_backward: the same launches, the same
 *                   outputs bit for bit.
 * The kernels are the DU forms of qpb_kkt_bwd_box.hip, plain and SH.  The masked
 * Cholesky is untouched; per QP the new work is d from glam and the mask, one
 * product of the untouched rows of H (held for r) with d, and d in place of 0
 * on the fixed variables.
 * Errors, in order: the descriptor as qpb_solve_box (m != 2n
 * QPB_ERR_INVALID_ARG); flags != 0 and a bit of `shared` other than
 * QPB_SHARED_H QPB_ERR_INVALID_ARG; n > 32 QPB_ERR_UNSUPPORTED; batch == 0
 * returns 0 before the pointers are looked at; missing pointers
 * QPB_ERR_INVALID_ARG (H, x, active and gx; at least one output); a missing
 * device last.  glam is never required.
 * Device pointers; asynchronous on `stream`. */
int qpb_solve_box_backward_dual(const qpb_desc *desc, int32_t shared,
				const double *H, const double *x,
				const uint32_t *active, const int32_t *status,
				const double *gx, const double *glam,
				double *gH, double *gf, double *glb,
				double *gub, void *stream);

/* Same with host pointers (with QPB_SHARED_H, H and gH are one matrix each). */
int qpb_solve_box_backward_dual_host(const qpb_desc *desc, int32_t shared,
				     const double *H, const double *x,
				     const uint32_t *active,
				     const int32_t *status, const double *gx,
				     const double *glam, double *gH, double *gf,
				     double *glb, double *gub);

/* ONE H for a batch of box QPs, factored ONCE.  With H shared, the set-up of
 * every QP -- H = L L^T and the rows of L^-T, which are the rows of
 * D = A L^-T for A = [I; -I] up to sign -- is the same numbers; qpb_factor_box
 * computes them once into a box factor buffer, and qpb_solve_box_factored
 * starts every QP from it: what is left per QP is y = L^-1 f, e = L^-T y and
 * the slacks ub + e and -lb - e.
 *
 * The buffer `bxfac` holds a header ([0] 0 or QPB_NOT_SPD as a double, [1] n,
 * [2] the padded n), L, the rows of L^-T and per row its squared norm, in the
 * order the solve's lanes load them; it holds neither H nor A (the recovery
 * x = -H^-1 (f + lam_u - lam_l) reads neither).  Its layout is internal
 * (csrc/qpb_factor.h, bxfct) and belongs to one n: n <= 16 is
 * qpb_gi_box.hip's, 16 < n <= 32 the BOX form of qpb_gi_wave.hip's.  It is NOT
 * qpb_factor_shared's `fac`: a buffer of the other kind, or one made for
 * another n, is the caller's error, like any wrongly sized array.  `bxfac` must
 * be 16-byte aligned (hipMalloc's and torch's allocations are), else
 * QPB_ERR_INVALID_ARG. */

/* doubles a box factor buffer for n holds; < 0: a qpb_error (n < 1:
 * QPB_ERR_INVALID_ARG; n > 32: QPB_ERR_UNSUPPORTED).  Pure host arithmetic. */
int64_t qpb_factor_box_doubles(int32_t n);

/* Factor ONE H (n x n) into `bxfac` (qpb_factor_box_doubles(n) doubles,
 * device).  One small launch of one workgroup, asynchronous on `stream`: a
 * solve queued behind it on the same stream needs no host synchronisation.
 * Every element of the buffer is written, and nothing else.  fstatus (one
 * int32, device, may be NULL): QPB_OK or QPB_NOT_SPD; a NaN in H gives
 * QPB_NOT_SPD, as it does in the solve kernels.  L and L^-T are the values the
 * unfactored kernels compute: each class's factor kernel runs that class's own
 * load and sweep.  H is only read.
 * Errors, in order: n < 1 QPB_ERR_INVALID_ARG; n > 32 QPB_ERR_UNSUPPORTED; H or
 * bxfac missing QPB_ERR_INVALID_ARG; a misaligned bxfac QPB_ERR_INVALID_ARG; a
 * missing device last. */
int qpb_factor_box(int32_t n, const double *H, double *bxfac, int32_t *fstatus,
		   void *stream);

/* Same with host pointers; bxfac (host, any alignment) receives the buffer. */
int qpb_factor_box_host(int32_t n, const double *H, double *bxfac,
			int32_t *fstatus);

/* qpb_solve_box_shared without the per-QP set-up, on a buffer of
 * qpb_factor_box for desc->n.  The contract is that call's on the H the buffer
 * was made from: the layouts with m = 2n (lam: upper bounds' multipliers
 * first; active: ceil(2n/32) words per QP), what is written at every status,
 * NaN and +-inf bounds or a NULL lb / ub as absent bounds, pinned variables and
 * crossed bounds, lam >= 0 exactly, the default max_iter 4 (n + m) + 8,
 * feas_tol per call.  A QP's outputs depend on its own f, lb and ub and on
 * bxfac only: not on the batch size, on the QP's position, or on the other QPs
 * of the launch, non-finite ones included.  Two things differ.  The outputs are
 * not bit for bit qpb_solve_box_shared's: L and L^-T are the same numbers, but
 * the slacks are formed from the stored rows and no longer inside the sweep, so
 * x and lam differ by rounding; on a non-degenerate QP status and active are
 * the same.  And iters may differ from the unfactored solve's.
 * A buffer whose H was not SPD gives every QP QPB_NOT_SPD, with iters = 0,
 * lam = 0 and active = 0.  The buffer is only read: any number of solves, on
 * any streams, may use it at once.
 * Errors, in order: the descriptor as qpb_solve_box (m != 2n
 * QPB_ERR_INVALID_ARG); desc->flags != 0 QPB_ERR_INVALID_ARG; n > 32
 * QPB_ERR_UNSUPPORTED; batch == 0 returns 0 before the pointers are looked at;
 * missing pointers QPB_ERR_INVALID_ARG (bxfac, f, x, lam, active and status;
 * lb, ub and iters may be NULL); a misaligned bxfac QPB_ERR_INVALID_ARG; a
 * missing device last.
 * The backward is qpb_solve_box_shared_backward on the H the buffer was made
 * from, unchanged.  Limit: n <= 32.  Follow-up: the Gram class, 32 < n <= 128,
 * whose set-up runs on the matrix cores and whose buffer would be a different
 * object.
 * Device pointers; asynchronous on `stream`. */
int qpb_solve_box_factored(const qpb_desc *desc, const double *bxfac,
			   const double *f, const double *lb, const double *ub,
			   double *x, double *lam, uint32_t *active,
			   int32_t *status, int32_t *iters, void *stream);

/* Same with host pointers (bxfac included: the call uploads it). */
int qpb_solve_box_factored_host(const qpb_desc *desc, const double *bxfac,
				const double *f, const double *lb,
				const double *ub, double *x, double *lam,
				uint32_t *active, int32_t *status,
				int32_t *iters);

/* T right-hand sides per QP in ONE launch: qpb_solve_factored_backward_dual
 * (gH = gA = NULL) and qpb_solve_box_backward_dual (gH = NULL) for T = nrhs
 * directions (gx, glam) at a time.  Because K is symmetric these are also T
 * tangents of (x*, lam*): the columns of a Jacobian dx* / df (gx = I), or of
 * the local affine law of an MPC tick.  Everything that does
 * not depend on the right-hand side -- the load of the buffer or of H, the
 * orthogonalisation D_W^T = Q R, the masked Cholesky -- runs once per QP; one
 * more direction costs the projections and the triangular solves.
 *
 * Layouts.  The right-hand sides of QP k are contiguous and direction-major:
 * direction t is at gx + (k T + t) n and glam + (k T + t) m (m = 2n for the box
 * call).  The outputs likewise: gf is B x T x n, gb B x T x m, glb and gub
 * B x T x n.  T = 1 gives the single-direction calls' layouts.
 *   QPB_SHARED_RHS  gx is T x n and glam T x m: ONE set of right-hand sides
 *                   that every QP reads (df = F e_j, db = G e_j of the affine
 *                   law; gx = I of the Jacobian).  The outputs equal those on
 *                   B materialised copies bit for bit.
 *   QPB_SHARED_H    box call only, as in qpb_solve_box_backward_dual: ONE
 *                   n x n H.
 * x and lam are not arguments: neither gf nor gb depends on them.  There is no
 * gH or gA: they are outer products with one x; the single-direction calls
 * have them.
 *
 * Contract.  For every QP k and direction t the outputs of direction t equal
 * BIT FOR BIT what the single-direction call writes into the same outputs for
 * that QP with gx[k, t] and glam[k, t]: qpb_solve_factored_backward_dual on the
 * same buffer, active and status, qpb_solve_box_backward_dual on the same H,
 * shared & QPB_SHARED_H, active and status.  Each direction runs the same
 * operations on the same numbers in the same order.  Everything those calls
 * say holds per direction: the glam of a row outside W, of a skipped row, of a
 * clear bit and of a QP that is not QPB_OK is ignored, NaN included; such a QP,
 * and every QP on a buffer whose H was not positive definite, gets zeros in
 * every direction; both bits of a box variable set: the upper bound counts;
 * bits >= m (>= 2n) are ignored; dx is -+glam exactly on a fixed box variable;
 * status == NULL counts as QPB_OK; every element of every non-NULL output is
 * written and nothing else; a QP's outputs depend on its own inputs only.
 * And: direction t's outputs depend on direction t's right-hand side only --
 * not on T, on t, or on what the other directions hold, NaN included.
 *   glam == NULL    (or m == 0 in the factored call) the forms without the DU
 *                   steps: each direction is qpb_solve_factored_backward's or
 *                   qpb_solve_box_backward's bit for bit.
 *   m == 0          gb is ignored.
 *   outputs         each may be NULL; at least one must be given.
 * The kernels are the MU forms of qpb_kkt_bwd.hip's factored forms and of
 * qpb_kkt_bwd_box.hip's kernels.
 * Errors, in order: the descriptor as qpb_solve; box call: m != 2n
 * QPB_ERR_INVALID_ARG; flags != 0, a bit of `shared` outside QPB_SHARED_RHS
 * (box call: QPB_SHARED_H | QPB_SHARED_RHS), nrhs < 1 or > QPB_MAX_RHS
 * QPB_ERR_INVALID_ARG; n > 32 or m > 64 QPB_ERR_UNSUPPORTED; batch == 0
 * returns 0 before the pointers are looked at; missing pointers
 * QPB_ERR_INVALID_ARG (bfac or H, gx, active -- factored call: when m > 0 --
 * and at least one output); a bfac that is not 16-byte aligned
 * QPB_ERR_INVALID_ARG; a missing device last.
 * Follow-ups: the unfactored qpb_solve_backward_dual with T directions (its u
 * comes out of the set-up sweep and needs another construction), the n <= 128
 * Gram class, qpb.diff (torch's batched gradients need a vmap rule), and the
 * version bump to 0.15.
 * Device pointers; asynchronous on `stream`. */
#define QPB_SHARED_RHS 4 /* gx and glam are ONE set of T right-hand sides for the whole batch */
#define QPB_MAX_RHS 256  /* >= n + m at the largest shape: every column of K^-1 in one call */

int qpb_solve_factored_backward_multi(const qpb_desc *desc, const double *bfac,
				      const uint32_t *active,
				      const int32_t *status, int32_t nrhs,
				      int32_t shared, const double *gx,
				      const double *glam, double *gf,
				      double *gb, void *stream);

/* Same with host pointers (bfac included: the call uploads it). */
int qpb_solve_factored_backward_multi_host(const qpb_desc *desc,
					   const double *bfac,
					   const uint32_t *active,
					   const int32_t *status,
					   int32_t nrhs, int32_t shared,
					   const double *gx,
					   const double *glam, double *gf,
					   double *gb);

int qpb_solve_box_backward_multi(const qpb_desc *desc, int32_t shared,
				 const double *H, const uint32_t *active,
				 const int32_t *status, int32_t nrhs,
				 const double *gx, const double *glam,
				 double *gf, double *glb, double *gub,
				 void *stream);

/* Same with host pointers (with QPB_SHARED_H, H is one matrix). */
int qpb_solve_box_backward_multi_host(const qpb_desc *desc, int32_t shared,
				      const double *H, const uint32_t *active,
				      const int32_t *status, int32_t nrhs,
				      const double *gx, const double *glam,
				      double *gf, double *glb, double *gub);

/* Reference-semantics solvers (qp_solvers.c replicas). */
typedef enum qpb_ref_mode {
	QPB_REF_NEWTON = 1, /* qp_solvers.c:103-144 (explicit LU inverse, Armijo quirk) */
	QPB_REF_ADMM = 2,   /* qp_solvers.c:255-319 (rho = 1, alpha = 1, returns x) */
	QPB_REF_GD = 3      /* qp_solvers.c:65-101 */
} qpb_ref_mode;

typedef struct qpb_ref_desc {
	int32_t n;          /* variables (N_DIM of the reference) */
	int32_t mode;       /* qpb_ref_mode */
	int64_t batch;
	int32_t iterations; /* the reference's `iterations` argument */
	int32_t flags;      /* reserved, 0 */
	double box_min;     /* ADMM box (config.h:29-30 ADMM_BOX_CONSTRAINT_MIN/MAX) */
	double box_max;
} qpb_ref_desc;

/* P n*n, q n, x0 n per QP (device), 1 <= n <= QPB_REF_MAX_N; writes x n per
 * QP and the iteration count per QP (may be NULL).  x0 is ignored by ADMM, as in the reference
 * (qp_solvers.c:256). */
int qpb_ref_solve(const qpb_ref_desc *desc, const double *P, const double *q,
		  const double *x0, double *x, int32_t *iters, void *stream);

int qpb_ref_solve_host(const qpb_ref_desc *desc, const double *P,
		       const double *q, const double *x0, double *x,
		       int32_t *iters);

/* Batched matrix_invert (matrix_ops.c:551-630): Pinv = P^{-1} per matrix,
 * n <= 128, device pointers, n*n doubles each.  The reference's partial-pivot
 * LU (first strict maximum, physical row swaps, :434-536) and per-column
 * forward / back solves, unfused, in its order: bitwise equal to the
 * reference's result.  n <= QPB_REF_MAX_N.  A singular pivot stops the LU as in the reference
 * (:511-515); the result is then garbage, as there. */
int qpb_matrix_invert(int32_t n, int64_t batch, const double *P, double *Pinv,
		      void *stream);

/* f(x) = 1/2 x^T P x + q^T x + r per QP (qp.c:9-27), batched, device. */
int qpb_qf_eval(int32_t n, int64_t batch, const double *P, const double *q,
		double r, const double *x, double *out, void *stream);

/* Diagnostic: same solve (n = 16 with 16 < m <= 32, 16 < n <= 32 with
 * m <= 64, or the n <= 128 Gram class in one launch; QPB_ERR_UNSUPPORTED
 * otherwise, and for sections == NULL; array pointers checked as by
 * qpb_solve) by a build of the kernel with s_memrealtime stamps (100 MHz); adds
 * each wavefront's ticks per kernel section into row (workgroup index mod 256)
 * of sections[256][20] (zero it first; sum the rows for the totals).
 * sections_len is the device buffer's length in elements: below
 * QPB_SECTIONS_LEN the call fails with QPB_ERR_INVALID_ARG (no write).
 * n = 16: load, cholesky, substitution, init, select, exchange, back-solve,
 * step, add, drop, loop-exit, output.  16 < n <= 32: load, sweep, init,
 * select, exchange, back-solve, step, add, drop, loop-exit, x, stores. */
#define QPB_SECTIONS_LEN (256 * 20)
int qpb_solve_sections(const qpb_desc *desc, const double *H, const double *f,
		       const double *A, const double *b, double *x, double *lam,
		       uint32_t *active, int32_t *status, int32_t *iters,
		       unsigned long long *sections, int64_t sections_len, void *stream);

/* ------------------------------------------------------------------------
 * On-device input generators.
 *
 * qpb_ref_generate: the reference's generator bit for bit -- srand(seed),
 * then per QP P = matirx_random_pos_def (matrix_ops.c:699-734), q, x0 =
 * matrix_random (main.c:37-39 order), glibc TYPE_3 rand().  QPs
 * [first, first + batch) of that sequence (each QP jumps ahead to its own
 * offset), so any shard equals the same QPs of one sequential run.
 * P n*n, q n, x0 n per QP, device pointers.  1 <= n <= 128.             */
typedef struct qpb_ref_gen_desc {
	int32_t n;      /* N_DIM */
	uint32_t seed;  /* srand() argument */
	int64_t batch;
	uint64_t first; /* index of the first QP in the sequence */
	double p_min, p_max; /* random_pos_def range (main.c:37: -1e3, 1e3) */
	double q_min, q_max; /* q range (main.c:38) */
	double x_min, x_max; /* x0 range (main.c:39) */
} qpb_ref_gen_desc;

int qpb_ref_generate(const qpb_ref_gen_desc *desc, double *P, double *q, double *x0, void *stream);

/* qpb_generate: the benchmark families of SURVEY.md §8d from a counter-based
 * Philox4x32-10 stream keyed by (seed, QP index): QP first + k of any launch
 * is the same QP.  H = B^T B / (1e3 n) + shift I with B ~ U[-1e3, 1e3]^{n x n}
 * (product on the fp64 matrix cores), f ~ U[-1e3, 1e3];
 *   QPB_FAMILY_BOX:   A = [I; -I] (m = 2n), b = box
 *   QPB_FAMILY_DENSE: rows of A ~ N(0, I) normalised, b ~ U[0.1, 1) box
 * Device pointers H n*n, f n, A m*n, b m per QP.  1 <= n <= 128; for
 * n > 16, m >= n (B is staged in A's rows).                             */
typedef enum qpb_family { QPB_FAMILY_BOX = 0, QPB_FAMILY_DENSE = 1 } qpb_family;

typedef struct qpb_gen_desc {
	int32_t n, m;
	int64_t batch;
	uint64_t first; /* QP index of the first QP generated */
	uint64_t seed;
	int32_t family; /* qpb_family */
	int32_t flags;  /* reserved, 0 */
	double shift;   /* added to H's diagonal (0: the heavy-tailed "ref" family) */
	double box;     /* box half-width / b scale */
} qpb_gen_desc;

int qpb_generate(const qpb_gen_desc *desc, double *H, double *f, double *A, double *b, void *stream);

/* ------------------------------------------------------------------------
 * Wire format, host memory, native-endian fp64.
 * The reference's single QP (test/test.c:108-126 -> test/qp_ref.py:8-30):
 *     [n][P n*n][q n]
 * Batched:  [n][m][B] then B records [H n*n][f n][A m*n][b m].
 * qpb_wire_write emits the reference form when m == 0 and batch == 1; the
 * readers accept both (told apart by the file size).                    */
int qpb_wire_write(const char *path, int32_t n, int32_t m, int64_t batch, const double *H, const double *f,
		   const double *A, const double *b);
int qpb_wire_read_header(const char *path, int32_t *n, int32_t *m, int64_t *batch);
/* H B*n*n, f B*n, A B*m*n, b B*m host buffers sized from the header */
int qpb_wire_read(const char *path, double *H, double *f, double *A, double *b);

/* housekeeping */
int qpb_device_count(void);
int qpb_set_device(int device);
int qpb_synchronize(void *stream);
/* Scratch buffers are cached per (device, stream) and reused across calls
 * (the n <= 128 kernels and the reference replicas at n > 64 need one);
 * this synchronises those streams and frees them all.  The cache frees a
 * stream's buffer stream-ordered ON that stream, so release a stream's
 * buffer (qpb_release_stream_workspace) before destroying the stream.  Calls
 * from several host threads are safe, sharing a stream included: a buffer is
 * handed to a launch only while the cache is locked. */
int qpb_release_workspaces(void);
int qpb_release_stream_workspace(void *stream);
const char *qpb_last_error(void);
const char *qpb_version(void);

#ifdef __cplusplus
}
#endif

#endif /* QPB_H */
