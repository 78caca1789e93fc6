// qpb_launch.h -- the kernel launchers behind the C-ABI: the only place one is
// declared.  Every file that defines or calls a launcher includes this header,
// so the compiler checks each definition against its declaration.  The
// launchers take a hipStream_t and check nothing; they are internal to
// libqpb.so (hidden visibility), qpb_api.hip validates before it calls them.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qpb.h"

#define QPB_LAUNCHER __attribute__((visibility("hidden")))

extern "C" {
// ---- the active-set solvers: one launch over d->batch QPs -------------------
// The box forms (d->m == 2 d->n) take lb and ub, either may be NULL, where the
// others take A and b.
typedef hipError_t qpb_gi_launcher(const qpb_desc *d, const double *H, const double *f, const double *A,
                                   const double *b, double *x, double *lam, uint32_t *active, int32_t *status,
                                   int32_t *iters, hipStream_t stream);
QPB_LAUNCHER qpb_gi_launcher qpb_launch_gi,  // n <= 16, m <= 32 (qpb_gi.hip)
    qpb_launch_gi_wave,                      // n <= 32, m <= 64 (qpb_gi_wave.hip)
    qpb_launch_gi_wave_redo,                 // ... only the QPs whose status is qpb::kRedoStatus
    qpb_launch_gi_mixed,                     // 16 < n <= 32: fp32, fp64 refinement, the redo launch (qpb_gi_mixed.hip)
    qpb_launch_gi_box,                       // lb <= x <= ub, n <= 16 (qpb_gi_box.hip)
    qpb_launch_gi_wave_box,                  // ... n <= 32 (qpb_gi_wave.hip)
    qpb_launch_gi_gram_box;                  // ... n <= 128 (qpb_gi_gram.hip)
// qpb_solve_eq: rows 0 .. meq-1 of A are equalities (1 <= meq <= d->m, d->flags == 0)
typedef hipError_t qpb_gi_eq_launcher(const qpb_desc *d, int meq, const double *H, const double *f, const double *A,
                                      const double *b, double *x, double *lam, uint32_t *active, int32_t *status,
                                      int32_t *iters, hipStream_t stream);
QPB_LAUNCHER qpb_gi_eq_launcher qpb_launch_gi_eq,  // n <= 16, m <= 32 (qpb_gi.hip)
    qpb_launch_gi_wave_eq;                         // n <= 32, m <= 64 (qpb_gi_wave.hip)
// qpb_solve_backward: n <= 32, m <= 64 (qpb_kkt_bwd.hip); any of gH, gf, gA, gb may be NULL
QPB_LAUNCHER hipError_t qpb_launch_kkt_bwd(const qpb_desc *d, const double *H, const double *A, const double *x,
                                           const double *lam, const uint32_t *active, const int32_t *status,
                                           const double *gx, double *gH, double *gf, double *gA, double *gb,
                                           hipStream_t stream);
// qpb_solve_box_backward: d->m == 2 d->n, n <= 32 (qpb_kkt_bwd_box.hip); any of gH, gf, glb, gub may be NULL
QPB_LAUNCHER hipError_t qpb_launch_kkt_bwd_box(const qpb_desc *d, const double *H, const double *x,
                                               const uint32_t *active, const int32_t *status, const double *gx,
                                               double *gH, double *gf, double *glb, double *gub, hipStream_t stream);
// qpb_solve_box_shared: the box launchers with H's QP stride in doubles at run
// time (0: one copy for the whole batch, else n n) -- the SH forms of the three
// box kernels
typedef hipError_t qpb_gi_box_shared_launcher(const qpb_desc *d, const double *H, const double *f, const double *lb,
                                              const double *ub, double *x, double *lam, uint32_t *active,
                                              int32_t *status, int32_t *iters, long long strideH, hipStream_t stream);
QPB_LAUNCHER qpb_gi_box_shared_launcher qpb_launch_gi_box_shared,  // n <= 16 (qpb_gi_box.hip)
    qpb_launch_gi_wave_box_shared,                                 // ... n <= 32 (qpb_gi_wave.hip)
    qpb_launch_gi_gram_box_shared;                                 // ... n <= 128 (qpb_gi_gram.hip)
// qpb_factor_box: ONE H (n x n) into the class's box factor buffer (qpb_factor.h,
// bxfct), one small launch of the class's own kernel in its factor form; fstatus
// may be NULL
typedef hipError_t qpb_gi_box_factor_launcher(int n, const double *H, double *bxfac, int32_t *fstatus,
                                              hipStream_t stream);
QPB_LAUNCHER qpb_gi_box_factor_launcher qpb_launch_gi_box_factor,  // n <= 16 (qpb_gi_box.hip)
    qpb_launch_gi_wave_box_factor;                                 // ... n <= 32 (qpb_gi_wave.hip)
// qpb_solve_box_factored: the box launchers on such a buffer in place of H
typedef hipError_t qpb_gi_box_factored_launcher(const qpb_desc *d, const double *bxfac, const double *f,
                                                const double *lb, const double *ub, double *x, double *lam,
                                                uint32_t *active, int32_t *status, int32_t *iters,
                                                hipStream_t stream);
QPB_LAUNCHER qpb_gi_box_factored_launcher qpb_launch_gi_box_factored,  // n <= 16 (qpb_gi_box.hip)
    qpb_launch_gi_wave_box_factored;                                   // ... n <= 32 (qpb_gi_wave.hip)
// qpb_solve_box_shared_backward, pass 1: qpb_launch_kkt_bwd_box with that stride
// (gH NULL: pass 2, qpb_launch_kkt_bwd_sum with m == 0, sums the gradient)
QPB_LAUNCHER hipError_t qpb_launch_kkt_bwd_box_shared(const qpb_desc *d, long long strideH, const double *H,
                                                      const double *x, const uint32_t *active, const int32_t *status,
                                                      const double *gx, double *gH, double *gf, double *glb,
                                                      double *gub, hipStream_t stream);
// qpb_solve_shared: H and A with run-time QP strides in doubles (0: one copy for
// the whole batch, else n n and m n); meq == 0 is the plain form, meq > 0 the EQ form
typedef hipError_t qpb_gi_shared_launcher(const qpb_desc *d, int meq, long long strideH, long long strideA,
                                          const double *H, const double *f, const double *A, const double *b,
                                          double *x, double *lam, uint32_t *active, int32_t *status, int32_t *iters,
                                          hipStream_t stream);
QPB_LAUNCHER qpb_gi_shared_launcher qpb_launch_gi_shared,  // n <= 16, m <= 32 (qpb_gi.hip)
    qpb_launch_gi_wave_shared;                             // n <= 32, m <= 64 (qpb_gi_wave.hip)
// qpb_solve_range: two-sided rows bl <= A x <= bu (either of bl, bu may be NULL:
// no row has that side), equality rows 0 .. meq-1 (meq >= 0) and the shared
// launchers' strides; d->m >= 1, d->flags == 0; lower may be NULL
typedef hipError_t qpb_gi_range_launcher(const qpb_desc *d, int meq, long long strideH, long long strideA,
                                         const double *H, const double *f, const double *A, const double *bl,
                                         const double *bu, double *x, double *lam, uint32_t *active, uint32_t *lower,
                                         int32_t *status, int32_t *iters, hipStream_t stream);
QPB_LAUNCHER qpb_gi_range_launcher qpb_launch_gi_range,  // n <= 16, m <= 32 (qpb_gi.hip)
    qpb_launch_gi_wave_range;                            // n <= 32, m <= 64 (qpb_gi_wave.hip)
// qpb_solve_range_box: the BX forms of the range forms.  d->m counts all rows,
// mg + n: the mg general rows of G (mg >= 0; G, bl, bu: mg per QP, G unread at
// mg == 0, strideA 0 or mg n), then the variables' bounds lb <= x <= ub (n per
// QP) as rows mg .. d->m-1.  Any of bl, bu, lb, ub and lower may be NULL.
typedef hipError_t qpb_gi_range_box_launcher(const qpb_desc *d, int mg, int meq, long long strideH, long long strideA,
                                             const double *H, const double *f, const double *G, const double *bl,
                                             const double *bu, const double *lb, const double *ub, double *x,
                                             double *lam, uint32_t *active, uint32_t *lower, int32_t *status,
                                             int32_t *iters, hipStream_t stream);
QPB_LAUNCHER qpb_gi_range_box_launcher qpb_launch_gi_range_box,  // n <= 16, mg + n <= 32 (qpb_gi.hip)
    qpb_launch_gi_wave_range_box;                                // n <= 32, mg + n <= 64 (qpb_gi_wave.hip)
// qpb_factor_shared: ONE H (n x n) and ONE A (m x n, NULL at m == 0) into the
// class's factor buffer (qpb_factor.h), one small launch; fstatus may be NULL
typedef hipError_t qpb_gi_factor_launcher(int n, int m, const double *H, const double *A, double *fac,
                                          int32_t *fstatus, hipStream_t stream);
QPB_LAUNCHER qpb_gi_factor_launcher qpb_launch_gi_factor,  // n <= 16, m <= 32 (qpb_gi.hip)
    qpb_launch_gi_wave_factor;                             // n <= 32, m <= 64 (qpb_gi_wave.hip)
// qpb_solve_factored: the solve on such a buffer; meq == 0 is the plain form, meq > 0 the EQ form
typedef hipError_t qpb_gi_factored_launcher(const qpb_desc *d, int meq, const double *fac, const double *f,
                                            const double *b, double *x, double *lam, uint32_t *active,
                                            int32_t *status, int32_t *iters, hipStream_t stream);
QPB_LAUNCHER qpb_gi_factored_launcher qpb_launch_gi_factored,  // n <= 16, m <= 32 (qpb_gi.hip)
    qpb_launch_gi_wave_factored;                               // n <= 32, m <= 64 (qpb_gi_wave.hip)
// qpb_solve_range_factored: the range launchers' rows and outputs on such a
// buffer; d->m >= 1, d->flags == 0, meq >= 0; either of bl, bu and lower may be NULL
typedef hipError_t qpb_gi_range_factored_launcher(const qpb_desc *d, int meq, const double *fac, const double *f,
                                                  const double *bl, const double *bu, double *x, double *lam,
                                                  uint32_t *active, uint32_t *lower, int32_t *status, int32_t *iters,
                                                  hipStream_t stream);
QPB_LAUNCHER qpb_gi_range_factored_launcher qpb_launch_gi_range_factored,  // n <= 16, m <= 32 (qpb_gi.hip)
    qpb_launch_gi_wave_range_factored;                                     // n <= 32, m <= 64 (qpb_gi_wave.hip)
// qpb_solve_shared_backward, pass 1: qpb_launch_kkt_bwd with the same strides
// (gH / gA NULL where pass 2 sums the gradient)
QPB_LAUNCHER hipError_t qpb_launch_kkt_bwd_shared(const qpb_desc *d, long long strideH, long long strideA,
                                                  const double *H, const double *A, const double *x,
                                                  const double *lam, const uint32_t *active, const int32_t *status,
                                                  const double *gx, double *gH, double *gf, double *gA, double *gb,
                                                  hipStream_t stream);
// qpb_solve_backward_dual, pass 1 (d->m > 0, glam not NULL): the DU forms of the
// same kernels on the same strides, with glam (B x m) as the lower right-hand side
QPB_LAUNCHER hipError_t qpb_launch_kkt_bwd_dual(const qpb_desc *d, long long strideH, long long strideA,
                                                const double *H, const double *A, const double *x, const double *lam,
                                                const uint32_t *active, const int32_t *status, const double *gx,
                                                const double *glam, double *gH, double *gf, double *gA, double *gb,
                                                hipStream_t stream);
// ... pass 2 (qpb_kkt_bwd_sum.hip): the n x n and / or m x n sums over the whole
// batch from pass 1's gf (dx) and gb; slots: qpb::sum_plan(batch).slots times
// qpb::sum_slot_doubles(n, m) doubles of scratch
QPB_LAUNCHER hipError_t qpb_launch_kkt_bwd_sum(const qpb_desc *d, const double *x, const double *dx, const double *gb,
                                               const double *lam, const uint32_t *active, const int32_t *status,
                                               double *slots, double *gH, double *gA, hipStream_t stream);
// qpb_solve_range_box_backward, pass 1: the BX forms of the same kernels.  d->m
// counts all rows, mg + n (lam, glam, active and lower in that layout); G is
// mg x n per QP (strideG 0 or mg n, unread at mg == 0), gG its gradient (NULL
// where pass 2 sums it).  gb's elements go to gbl / gbu (B x mg) and glb / gub
// (B x n) by the `lower` bits, and the rows < mg unrouted to gbw (B x mg) for
// pass 2.  glam, lower and every output may be NULL.
QPB_LAUNCHER hipError_t qpb_launch_kkt_bwd_range_box(const qpb_desc *d, int mg, long long strideH, long long strideG,
                                                     const double *H, const double *G, const double *x,
                                                     const double *lam, const uint32_t *active, const uint32_t *lower,
                                                     const int32_t *status, const double *gx, const double *glam,
                                                     double *gH, double *gf, double *gG, double *gbl, double *gbu,
                                                     double *glb, double *gub, double *gbw, hipStream_t stream);
// ... pass 2: qpb_launch_kkt_bwd_sum over the rows < mg (d->m is mg + n: the row
// stride of lam and active; gbw is pass 1's, B x mg).  slots:
// qpb::sum_plan(batch).slots times qpb::sum_slot_doubles(n, mg) doubles.
QPB_LAUNCHER hipError_t qpb_launch_kkt_bwd_sum_range_box(const qpb_desc *d, int mg, const double *x, const double *dx,
                                                         const double *gbw, const double *lam, const uint32_t *active,
                                                         const int32_t *status, double *slots, double *gH, double *gG,
                                                         hipStream_t stream);
// qpb_factor_shared_backward: ONE H and ONE A (NULL at m == 0) into the class's
// backward buffer (qpb_factor.h, bfct), one small launch of the class's own
// kernel in its factor form (qpb_kkt_bwd.hip); fstatus may be NULL
QPB_LAUNCHER hipError_t qpb_launch_kkt_bwd_factor(int n, int m, const double *H, const double *A, double *bfac,
                                                  int32_t *fstatus, hipStream_t stream);
// qpb_solve_factored_backward, pass 1: qpb_launch_kkt_bwd_shared with both
// operands shared, on such a buffer (pass 2 is qpb_launch_kkt_bwd_sum unchanged)
QPB_LAUNCHER hipError_t qpb_launch_kkt_bwd_factored(const qpb_desc *d, const double *bfac, const double *x,
                                                    const double *lam, const uint32_t *active, const int32_t *status,
                                                    const double *gx, double *gf, double *gb, hipStream_t stream);
// qpb_solve_factored_backward_dual, pass 1 (d->m > 0, glam not NULL): the DU
// forms of those factored forms, with glam (B x m) as the lower right-hand side
QPB_LAUNCHER hipError_t qpb_launch_kkt_bwd_factored_dual(const qpb_desc *d, const double *bfac, const double *x,
                                                         const double *lam, const uint32_t *active,
                                                         const int32_t *status, const double *gx, const double *glam,
                                                         double *gf, double *gb, hipStream_t stream);
// qpb_solve_box_backward_dual (glam not NULL, B x 2n): the DU forms of
// qpb_launch_kkt_bwd_box (strideH == n n) and of qpb_launch_kkt_bwd_box_shared
// (strideH == 0: pass 1, gH NULL)
QPB_LAUNCHER hipError_t qpb_launch_kkt_bwd_box_dual(const qpb_desc *d, long long strideH, const double *H,
                                                    const double *x, const uint32_t *active, const int32_t *status,
                                                    const double *gx, const double *glam, double *gH, double *gf,
                                                    double *glb, double *gub, hipStream_t stream);
// qpb_solve_factored_backward_multi: the MU forms of the factored forms (glam
// NULL or d->m == 0: without the DU steps).  T right-hand sides per QP,
// direction-major; rstride is their QP stride in directions: T, or 0 for one
// set (T x n, T x m) that every QP reads.  gf is batch x T x n, gb batch x T x m.
QPB_LAUNCHER hipError_t qpb_launch_kkt_bwd_factored_multi(const qpb_desc *d, const double *bfac,
                                                          const uint32_t *active, const int32_t *status, int T,
                                                          long long rstride, const double *gx, const double *glam,
                                                          double *gf, double *gb, hipStream_t stream);
// qpb_solve_box_backward_multi: the MU forms of the box kernels on H's run-time
// stride (0 or n n), glam (T x 2n per QP) NULL or not; gf, glb, gub batch x T x n
QPB_LAUNCHER hipError_t qpb_launch_kkt_bwd_box_multi(const qpb_desc *d, long long strideH, const double *H,
                                                     const uint32_t *active, const int32_t *status, int T,
                                                     long long rstride, const double *gx, const double *glam,
                                                     double *gf, double *glb, double *gub, hipStream_t stream);
// with per-section wave ticks into sections[256][20] (the stamped diagnostic builds)
typedef hipError_t qpb_gi_sections_launcher(const qpb_desc *d, const double *H, const double *f, const double *A,
                                            const double *b, double *x, double *lam, uint32_t *active,
                                            int32_t *status, int32_t *iters, unsigned long long *sections,
                                            hipStream_t stream);
QPB_LAUNCHER qpb_gi_sections_launcher qpb_launch_gi_sections,  // n = 16, 16 < m <= 32
    qpb_launch_gi_wave_sections,                               // 16 < n <= 32, m <= 64
    qpb_launch_gi_gram;  // n <= 128, m <= 256 (qpb_gi_gram.hip); sections NULL: the shipped kernel

// ---- the reference-semantics kernels (qpb_ref.hip) --------------------------
QPB_LAUNCHER hipError_t qpb_launch_ref(const qpb_ref_desc *d, const double *P, const double *q, const double *x0,
                                       double *x, int32_t *iters, hipStream_t stream);
QPB_LAUNCHER hipError_t qpb_launch_qf_eval(int n, long long batch, const double *P, const double *q, double r,
                                           const double *x, double *out, hipStream_t stream);
QPB_LAUNCHER hipError_t qpb_launch_ref_invert(int n, long long batch, const double *P, double *Pinv,
                                              hipStream_t stream);

// ---- the problem generators (qpb_gen.hip) -----------------------------------
QPB_LAUNCHER hipError_t qpb_launch_ref_generate(int n, long long batch, unsigned long long first, unsigned seed,
                                                const double *range, double *P, double *q, double *x0,
                                                hipStream_t stream);
QPB_LAUNCHER hipError_t qpb_launch_generate(int n, int m, long long batch, unsigned long long first,
                                            unsigned long long seed, int family, double shift, double box, double *H,
                                            double *f, double *A, double *b, hipStream_t stream);
}  // extern "C"

// The limits a launcher hands its kernel: the descriptor's, or the defaults
// where it leaves them at 0.  The box form has m = 2n.
struct qpb_limits {
  int max_iter;
  double feas_tol;
};
static inline qpb_limits qpb_resolve_limits(const qpb_desc *d) {
  return {d->max_iter > 0 ? d->max_iter : 4 * (d->n + d->m) + 8, d->feas_tol > 0 ? d->feas_tol : 1e-10};
}
