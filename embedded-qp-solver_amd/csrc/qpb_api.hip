// qpb_api.hip -- the C-ABI of include/qpb.h: argument checking, launches,
// host-pointer convenience wrappers.  No computation happens here: every
// solve runs in the HIP kernels (qpb_gi.hip, qpb_ref.hip); there is no CPU
// fallback -- without a usable HIP device the calls fail with
// QPB_ERR_NO_DEVICE / QPB_ERR_HIP.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include "qpb.h"
#include "qpb_common.h"  // kSectionSlots, kSections
#include "qpb_factor.h"  // the size of a factor buffer
#include "qpb_launch.h"
#include "qpb_route.h"

static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

// error reporting for the host-only C parts of the library (qpb_wire.c)
extern "C" __attribute__((visibility("hidden"))) void qpb_set_error(int code, const char *msg) {
  fail(code, "%s", msg);
}

static int hip_fail(hipError_t e, const char *what) {
  return fail(QPB_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

// The device census is taken once per process (a HIP runtime query per solve
// cost ~8 us of host time on every launch); a process without a device keeps
// failing with QPB_ERR_NO_DEVICE.
static int device_census(void) {
  static const int count = [] {
    int c = 0;
    return hipGetDeviceCount(&c) == hipSuccess ? c : 0;
  }();
  return count;
}

static int check_device(void) {
  if (device_census() <= 0) return fail(QPB_ERR_NO_DEVICE, "no HIP device available");
  return 0;
}

static int check_desc(const qpb_desc *d) {
  if (!d) return fail(QPB_ERR_INVALID_ARG, "desc is NULL");
  if (d->batch < 0) return fail(QPB_ERR_INVALID_ARG, "batch < 0");
  if (d->n < 1 || d->m < 0) return fail(QPB_ERR_INVALID_ARG, "n must be >= 1 and m >= 0");
  if (d->n > QPB_MAX_N || d->m > QPB_MAX_M)
    return fail(QPB_ERR_UNSUPPORTED, "n=%d m=%d outside this build's kernels (n<=%d, m<=%d)", d->n, d->m,
                QPB_MAX_N, QPB_MAX_M);
  return 0;
}

// The arrays a dense solve reads and writes (qpb_solve, qpb_solve_sections);
// iters may be NULL
static int check_solve_arrays(const qpb_desc *d, const double *H, const double *f, const double *A, const double *b,
                              const double *x, const double *lam, const uint32_t *active, const int32_t *status) {
  if (!H || !f || !x || !status) return fail(QPB_ERR_INVALID_ARG, "H, f, x and status are required");
  if (d->m > 0 && (!A || !b || !lam || !active))
    return fail(QPB_ERR_INVALID_ARG, "A, b, lam and active are required when m > 0");
  return 0;
}

// The launcher of a kernel class, except gi_gram's (it takes the sections pointer too)
static qpb_gi_launcher *launcher_of(qpb::Kernel k) {
  switch (k) {
    case qpb::Kernel::gi_dense: return qpb_launch_gi;
    case qpb::Kernel::gi_wave: return qpb_launch_gi_wave;
    case qpb::Kernel::gi_mixed: return qpb_launch_gi_mixed;
    case qpb::Kernel::gi_box: return qpb_launch_gi_box;
    case qpb::Kernel::gi_wave_box: return qpb_launch_gi_wave_box;
    case qpb::Kernel::gi_gram_box: return qpb_launch_gi_gram_box;
    case qpb::Kernel::gi_gram: break;
  }
  return nullptr;
}

// The batch in chunks of the route's step, one launch each (Ab, bb: A and b, or
// lb and ub for the box kernels).  lam and active are NULL only at m = 0, iters
// whenever the caller does not want it.
static int solve_chunks(const qpb_desc *d, qpb::Route r, const double *H, const double *f,
                        qpb::Batched<const double> Ab, qpb::Batched<const double> bb, double *x, double *lam,
                        uint32_t *active, int32_t *status, int32_t *iters, hipStream_t stream, const char *what) {
  const long long n = d->n, m = d->m;
  return qpb::for_each_chunk(
      d->batch, r.step,
      [&](long long count, const double *Hc, const double *fc, const double *Ac, const double *bc, double *xc,
          double *lc, uint32_t *ac, int32_t *sc, int32_t *ic) {
        qpb_desc c = *d;
        c.batch = count;
        qpb_gi_launcher *const fn = launcher_of(r.kernel);
        const hipError_t e = fn ? fn(&c, Hc, fc, Ac, bc, xc, lc, ac, sc, ic, stream)
                                : qpb_launch_gi_gram(&c, Hc, fc, Ac, bc, xc, lc, ac, sc, ic, nullptr, stream);
        return e == hipSuccess ? 0 : hip_fail(e, what);
      },
      qpb::required(H, n * n), qpb::required(f, n), Ab, bb, qpb::required(x, n), qpb::optional(lam, m),
      qpb::optional(active, (m + 31) / 32), qpb::required(status, 1), qpb::optional(iters, 1));
}

extern "C" int qpb_solve(const qpb_desc *d, const double *H, const double *f, const double *A,
                         const double *b, double *x, double *lam, uint32_t *active, int32_t *status,
                         int32_t *iters, void *stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  if (d->batch == 0) return 0;
  rc = check_solve_arrays(d, H, f, A, b, x, lam, active, status);
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  return solve_chunks(d, qpb::route(d->n, d->m, d->flags, false), H, f, qpb::optional(A, (long long)d->m * d->n),
                      qpb::optional(b, d->m), x, lam, active, status, iters, (hipStream_t)stream, "qpb_solve launch");
}

// qpb_solve_eq's own argument rules, after check_desc: the flags select
// nothing here, and with meq > 0 the shape must have an EQ kernel form
static int check_eq(const qpb_desc *d, int32_t meq) {
  if (meq < 0) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_eq: meq < 0");
  if (d->flags != 0) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_eq: flags must be 0 (got %d)", d->flags);
  if (meq > 0 && qpb::route_eq(d->n, d->m).step == 0)
    return fail(QPB_ERR_UNSUPPORTED, "qpb_solve_eq: n=%d m=%d outside the kernels with equality rows (n<=%d, m<=%d)",
                d->n, d->m, qpb::kEqMaxN, qpb::kEqMaxM);
  if (meq > d->m) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_eq: meq=%d > m=%d", meq, d->m);
  return 0;
}

extern "C" int qpb_solve_eq(const qpb_desc *d, int32_t meq, const double *H, const double *f, const double *A,
                            const double *b, double *x, double *lam, uint32_t *active, int32_t *status,
                            int32_t *iters, void *stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_eq(d, meq);
  if (rc) return rc;
  // no equality rows: the call is qpb_solve, launch for launch
  if (meq == 0) return qpb_solve(d, H, f, A, b, x, lam, active, status, iters, stream);
  if (d->batch == 0) return 0;
  rc = check_solve_arrays(d, H, f, A, b, x, lam, active, status);
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  const qpb::Route r = qpb::route_eq(d->n, d->m);
  qpb_gi_eq_launcher *const fn = r.kernel == qpb::Kernel::gi_dense ? qpb_launch_gi_eq : qpb_launch_gi_wave_eq;
  const long long n = d->n, m = d->m;
  return qpb::for_each_chunk(
      d->batch, r.step,
      [&](long long count, const double *Hc, const double *fc, const double *Ac, const double *bc, double *xc,
          double *lc, uint32_t *ac, int32_t *sc, int32_t *ic) {
        qpb_desc c = *d;
        c.batch = count;
        const hipError_t e = fn(&c, meq, Hc, fc, Ac, bc, xc, lc, ac, sc, ic, (hipStream_t)stream);
        return e == hipSuccess ? 0 : hip_fail(e, "qpb_solve_eq launch");
      },
      qpb::required(H, n * n), qpb::required(f, n), qpb::required(A, m * n), qpb::required(b, m),
      qpb::required(x, n), qpb::required(lam, m), qpb::required(active, (m + 31) / 32), qpb::required(status, 1),
      qpb::optional(iters, 1));
}

// qpb_solve_backward's argument rules after check_desc, up to the pointers
static int check_bwd(const qpb_desc *d) {
  if (d->flags != 0) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_backward: flags must be 0 (got %d)", d->flags);
  if (qpb::route_bwd(d->n, d->m).step == 0)
    return fail(QPB_ERR_UNSUPPORTED, "qpb_solve_backward: n=%d m=%d outside the backward kernels (n<=%d, m<=%d)", d->n,
                d->m, qpb::kBwdMaxN, qpb::kBwdMaxM);
  return 0;
}
static int check_bwd_arrays(const qpb_desc *d, const double *H, const double *A, const double *x, const double *lam,
                            const uint32_t *active, const double *gx, const double *gH, const double *gf,
                            const double *gA, const double *gb) {
  if (!H || !x || !gx) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_backward: H, x and gx are required");
  if (d->m > 0 && (!A || !lam || !active))
    return fail(QPB_ERR_INVALID_ARG, "qpb_solve_backward: A, lam and active are required when m > 0");
  if (!gH && !gf && !(d->m > 0 && (gA || gb)))
    return fail(QPB_ERR_INVALID_ARG, "qpb_solve_backward: at least one of gH, gf, gA and gb is required");
  return 0;
}

extern "C" int qpb_solve_backward(const qpb_desc *d, const double *H, const double *A, const double *x,
                                  const double *lam, const uint32_t *active, const int32_t *status, const double *gx,
                                  double *gH, double *gf, double *gA, double *gb, void *stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_bwd(d);
  if (rc) return rc;
  if (d->batch == 0) return 0;
  rc = check_bwd_arrays(d, H, A, x, lam, active, gx, gH, gf, gA, gb);
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  const qpb::Route r = qpb::route_bwd(d->n, d->m);
  const long long n = d->n, m = d->m;
  return qpb::for_each_chunk(
      d->batch, r.step,
      [&](long long count, const double *Hc, const double *Ac, const double *xc, const double *lc,
          const uint32_t *ac, const int32_t *sc, const double *gxc, double *gHc, double *gfc, double *gAc,
          double *gbc) {
        qpb_desc c = *d;
        c.batch = count;
        const hipError_t e = qpb_launch_kkt_bwd(&c, Hc, Ac, xc, lc, ac, sc, gxc, gHc, gfc, gAc, gbc, (hipStream_t)stream);
        return e == hipSuccess ? 0 : hip_fail(e, "qpb_solve_backward launch");
      },
      qpb::required(H, n * n), qpb::optional(A, m * n), qpb::required(x, n), qpb::optional(lam, m),
      qpb::optional(active, (m + 31) / 32), qpb::optional(status, 1), qpb::required(gx, n), qpb::optional(gH, n * n),
      qpb::optional(gf, n), qpb::optional(gA, m * n), qpb::optional(gb, m));
}

// ---- one H and / or one A for the whole batch --------------------------------
// `shared` with the bits that select nothing taken out: QPB_SHARED_A at m == 0
static int32_t shared_of(const qpb_desc *d, int32_t shared) { return d->m == 0 ? shared & ~QPB_SHARED_A : shared; }

// qpb_solve_shared's argument rules after check_desc: check_eq's, with the
// shared bits beside the flags and a size limit and message of its own
static int check_shared(const qpb_desc *d, int32_t meq, int32_t shared) {
  if (meq < 0) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_shared: meq < 0");
  if (d->flags != 0) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_shared: flags must be 0 (got %d)", d->flags);
  if (shared & ~(QPB_SHARED_H | QPB_SHARED_A))
    return fail(QPB_ERR_INVALID_ARG, "qpb_solve_shared: shared must be a combination of QPB_SHARED_H and QPB_SHARED_A (got %d)",
                shared);
  if (shared_of(d, shared) != 0 && qpb::route_shared(d->n, d->m).step == 0)
    return fail(QPB_ERR_UNSUPPORTED,
                "qpb_solve_shared: n=%d m=%d outside the kernels with a shared H or A (n<=%d, m<=%d)", d->n, d->m,
                qpb::kSharedMaxN, qpb::kSharedMaxM);
  return 0;
}

extern "C" int qpb_solve_shared(const qpb_desc *d, int32_t meq, int32_t shared, const double *H, const double *f,
                                const double *A, const double *b, double *x, double *lam, uint32_t *active,
                                int32_t *status, int32_t *iters, void *stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_shared(d, meq, shared);
  if (rc) return rc;
  shared = shared_of(d, shared);
  // nothing shared: the call is qpb_solve_eq, with its remaining rules
  if (shared == 0) return qpb_solve_eq(d, meq, H, f, A, b, x, lam, active, status, iters, stream);
  if (meq > d->m) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_shared: meq=%d > m=%d", meq, d->m);
  if (d->batch == 0) return 0;
  rc = check_solve_arrays(d, H, f, A, b, x, lam, active, status);
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  const qpb::Route r = qpb::route_shared(d->n, d->m);
  qpb_gi_shared_launcher *const fn =
      r.kernel == qpb::Kernel::gi_dense ? qpb_launch_gi_shared : qpb_launch_gi_wave_shared;
  const long long n = d->n, m = d->m;
  // a shared operand's QP stride is 0, in the kernels and in the chunk walk
  const long long sH = (shared & QPB_SHARED_H) ? 0 : n * n, sA = (shared & QPB_SHARED_A) ? 0 : m * n;
  return qpb::for_each_chunk(
      d->batch, r.step,
      [&](long long count, const double *Hc, const double *fc, const double *Ac, const double *bc, double *xc,
          double *lc, uint32_t *ac, int32_t *sc, int32_t *ic) {
        qpb_desc c = *d;
        c.batch = count;
        const hipError_t e = fn(&c, meq, sH, sA, Hc, fc, Ac, bc, xc, lc, ac, sc, ic, (hipStream_t)stream);
        return e == hipSuccess ? 0 : hip_fail(e, "qpb_solve_shared launch");
      },
      qpb::required(H, sH), qpb::required(f, n), qpb::optional(A, sA), qpb::optional(b, m), qpb::required(x, n),
      qpb::optional(lam, m), qpb::optional(active, (m + 31) / 32), qpb::required(status, 1), qpb::optional(iters, 1));
}

// qpb_solve_shared_backward's argument rules after check_desc, up to the pointers
static int check_shared_bwd(const qpb_desc *d, int32_t shared) {
  if (d->flags != 0)
    return fail(QPB_ERR_INVALID_ARG, "qpb_solve_shared_backward: flags must be 0 (got %d)", d->flags);
  if (shared & ~(QPB_SHARED_H | QPB_SHARED_A))
    return fail(QPB_ERR_INVALID_ARG,
                "qpb_solve_shared_backward: shared must be a combination of QPB_SHARED_H and QPB_SHARED_A (got %d)",
                shared);
  if (shared_of(d, shared) != 0 && qpb::route_shared_bwd(d->n, d->m).step == 0)
    return fail(QPB_ERR_UNSUPPORTED,
                "qpb_solve_shared_backward: n=%d m=%d outside the kernels with a shared H or A (n<=%d, m<=%d)", d->n,
                d->m, qpb::kSharedMaxN, qpb::kSharedMaxM);
  return 0;
}

// The two passes of qpb_solve_shared_backward (glam == NULL: its launches and
// nothing else) and of qpb_solve_backward_dual (glam given, m > 0, any `shared`,
// 0 included: pass 1 is the DU forms), after the checks.  `what` names the call.
static int shared_bwd_passes(const qpb_desc *d, int32_t shared, const double *H, const double *A, const double *x,
                             const double *lam, const uint32_t *active, const int32_t *status, const double *gx,
                             const double *glam, double *gH, double *gf, double *gA, double *gb, void *stream,
                             const char *what);

extern "C" int qpb_solve_shared_backward(const qpb_desc *d, int32_t shared, const double *H, const double *A,
                                         const double *x, const double *lam, const uint32_t *active,
                                         const int32_t *status, const double *gx, double *gH, double *gf, double *gA,
                                         double *gb, void *stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_shared_bwd(d, shared);
  if (rc) return rc;
  shared = shared_of(d, shared);
  // nothing shared: the call is qpb_solve_backward, with its remaining rules
  if (shared == 0) return qpb_solve_backward(d, H, A, x, lam, active, status, gx, gH, gf, gA, gb, stream);
  if (d->batch == 0) return 0;
  rc = check_bwd_arrays(d, H, A, x, lam, active, gx, gH, gf, gA, gb);
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  return shared_bwd_passes(d, shared, H, A, x, lam, active, status, gx, nullptr, gH, gf, gA, gb, stream,
                           "qpb_solve_shared_backward");
}

// qpb_solve_backward_dual's argument rules after check_desc, up to the pointers
static int check_bwd_dual(const qpb_desc *d, int32_t shared) {
  if (d->flags != 0) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_backward_dual: flags must be 0 (got %d)", d->flags);
  if (shared & ~(QPB_SHARED_H | QPB_SHARED_A))
    return fail(QPB_ERR_INVALID_ARG,
                "qpb_solve_backward_dual: shared must be a combination of QPB_SHARED_H and QPB_SHARED_A (got %d)",
                shared);
  if (qpb::route_bwd_dual(d->n, d->m).step == 0)
    return fail(QPB_ERR_UNSUPPORTED, "qpb_solve_backward_dual: n=%d m=%d outside the backward kernels (n<=%d, m<=%d)",
                d->n, d->m, qpb::kBwdDualMaxN, qpb::kBwdDualMaxM);
  return 0;
}

extern "C" int qpb_solve_backward_dual(const qpb_desc *d, int32_t shared, const double *H, const double *A,
                                       const double *x, const double *lam, const uint32_t *active,
                                       const int32_t *status, const double *gx, const double *glam, double *gH,
                                       double *gf, double *gA, double *gb, void *stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_bwd_dual(d, shared);
  if (rc) return rc;
  // no cotangent on lam: the call is qpb_solve_shared_backward, with its remaining rules
  if (!glam || d->m == 0)
    return qpb_solve_shared_backward(d, shared, H, A, x, lam, active, status, gx, gH, gf, gA, gb, stream);
  if (d->batch == 0) return 0;
  rc = check_bwd_arrays(d, H, A, x, lam, active, gx, gH, gf, gA, gb);
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  return shared_bwd_passes(d, shared, H, A, x, lam, active, status, gx, glam, gH, gf, gA, gb, stream,
                           "qpb_solve_backward_dual");
}

static int shared_bwd_passes(const qpb_desc *d, int32_t shared, const double *H, const double *A, const double *x,
                             const double *lam, const uint32_t *active, const int32_t *status, const double *gx,
                             const double *glam, double *gH, double *gf, double *gA, double *gb, void *stream,
                             const char *what) {
  int rc = 0;
  const qpb::Route r = qpb::route_shared_bwd(d->n, d->m);
  const long long n = d->n, m = d->m, B = d->batch;
  if (m == 0) gA = gb = nullptr;  // ignored
  const long long sH = (shared & QPB_SHARED_H) ? 0 : n * n, sA = (shared & QPB_SHARED_A) ? 0 : m * n;
  // the gradients pass 2 sums; pass 1 is launched without them
  double *const sumH = (shared & QPB_SHARED_H) ? gH : nullptr, *const sumA = (shared & QPB_SHARED_A) ? gA : nullptr;
  double *const gH1 = (shared & QPB_SHARED_H) ? nullptr : gH, *const gA1 = (shared & QPB_SHARED_A) ? nullptr : gA;
  const hipStream_t st = (hipStream_t)stream;
  // pass 1 over the batch in chunks; gf1 and gb1 are the caller's, or the workspace's where pass 2 needs them
  auto pass1 = [&](double *gf1, double *gb1) {
    return qpb::for_each_chunk(
        B, r.step,
        [&](long long count, const double *Hc, const double *Ac, const double *xc, const double *lc,
            const uint32_t *ac, const int32_t *sc, const double *gxc, const double *glc, double *gHc, double *gfc,
            double *gAc, double *gbc) {
          qpb_desc c = *d;
          c.batch = count;
          const hipError_t e =
              glam ? qpb_launch_kkt_bwd_dual(&c, sH, sA, Hc, Ac, xc, lc, ac, sc, gxc, glc, gHc, gfc, gAc, gbc, st)
                   : qpb_launch_kkt_bwd_shared(&c, sH, sA, Hc, Ac, xc, lc, ac, sc, gxc, gHc, gfc, gAc, gbc, st);
          return e == hipSuccess ? 0 : fail(QPB_ERR_HIP, "%s launch: %s", what, hipGetErrorString(e));
        },
        qpb::required(H, sH), qpb::optional(A, sA), qpb::required(x, n), qpb::optional(lam, m),
        qpb::optional(active, (m + 31) / 32), qpb::optional(status, 1), qpb::required(gx, n), qpb::optional(glam, m),
        qpb::optional(gH1, n * n), qpb::optional(gf1, n), qpb::optional(gA1, m * n), qpb::optional(gb1, m));
  };
  if (!sumH && !sumA) return pass1(gf, gb);  // the summed gradients are not wanted: pass 1 alone
  // workspace: the slots, then dx (B n) where gf is not given, then gb (B m)
  // where gA is summed and gb is not given
  const long long slot_doubles = qpb::sum_plan(B).slots * qpb::sum_slot_doubles(d->n, d->m);
  const long long ws_dx = gf ? 0 : B * n, ws_gb = (sumA && !gb) ? B * m : 0;
  const hipError_t e = qpb_with_workspace(st, (size_t)(slot_doubles + ws_dx + ws_gb) * 8, [&](void *ws) {
    double *const slots = (double *)ws;
    double *const dx = gf ? gf : slots + slot_doubles;
    double *const gbs = gb ? gb : sumA ? slots + slot_doubles + ws_dx : nullptr;
    rc = pass1(dx, gbs);
    if (rc) return hipSuccess;  // reported through rc
    return qpb_launch_kkt_bwd_sum(d, x, dx, gbs, lam, active, status, slots, sumH, sumA, st);
  });
  if (rc) return rc;
  return e == hipSuccess ? 0 : fail(QPB_ERR_HIP, "%s sum launch: %s", what, hipGetErrorString(e));
}

extern "C" int qpb_solve_box(const qpb_desc *d, const double *H, const double *f, const double *lb,
                             const double *ub, double *x, double *lam, uint32_t *active, int32_t *status,
                             int32_t *iters, void *stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  if (d->m != 2 * d->n) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_box: m must be 2n (got n=%d m=%d)", d->n, d->m);
  if (d->batch == 0) return 0;
  if (!H || !f || !x || !lam || !active || !status)
    return fail(QPB_ERR_INVALID_ARG, "H, f, x, lam, active and status are required");
  rc = check_device();
  if (rc) return rc;
  // n <= 16: qpb_gi_box.hip; 16 < n <= 32 and 32 < n <= 128: the BOX
  // instantiations of qpb_gi_wave.hip and qpb_gi_gram.hip.  lb / ub may be NULL
  return solve_chunks(d, qpb::route(d->n, d->m, d->flags, true), H, f, qpb::optional(lb, d->n),
                      qpb::optional(ub, d->n), x, lam, active, status, iters, (hipStream_t)stream,
                      "qpb_solve_box launch");
}

// qpb_solve_box_backward's argument rules after check_desc, up to the pointers
// (and qpb_solve_box_shared_backward's: `what` names the call)
static int check_bwd_box(const qpb_desc *d, const char *what = "qpb_solve_box_backward") {
  if (d->m != 2 * d->n) return fail(QPB_ERR_INVALID_ARG, "%s: m must be 2n (got n=%d m=%d)", what, d->n, d->m);
  if (d->flags != 0) return fail(QPB_ERR_INVALID_ARG, "%s: flags must be 0 (got %d)", what, d->flags);
  if (qpb::route_bwd_box(d->n).step == 0)
    return fail(QPB_ERR_UNSUPPORTED, "%s: n=%d outside the backward box kernels (n<=%d)", what, d->n,
                qpb::kBwdBoxMaxN);
  return 0;
}
static int check_bwd_box_arrays(const double *H, const double *x, const uint32_t *active, const double *gx,
                                const double *gH, const double *gf, const double *glb, const double *gub,
                                const char *what = "qpb_solve_box_backward") {
  if (!H || !x || !active || !gx) return fail(QPB_ERR_INVALID_ARG, "%s: H, x, active and gx are required", what);
  if (!gH && !gf && !glb && !gub)
    return fail(QPB_ERR_INVALID_ARG, "%s: at least one of gH, gf, glb and gub is required", what);
  return 0;
}

extern "C" int qpb_solve_box_backward(const qpb_desc *d, const double *H, const double *x, const uint32_t *active,
                                      const int32_t *status, const double *gx, double *gH, double *gf, double *glb,
                                      double *gub, void *stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_bwd_box(d);
  if (rc) return rc;
  if (d->batch == 0) return 0;
  rc = check_bwd_box_arrays(H, x, active, gx, gH, gf, glb, gub);
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  const qpb::Route r = qpb::route_bwd_box(d->n);
  const long long n = d->n, m = d->m;
  return qpb::for_each_chunk(
      d->batch, r.step,
      [&](long long count, const double *Hc, const double *xc, const uint32_t *ac, const int32_t *sc,
          const double *gxc, double *gHc, double *gfc, double *glc, double *guc) {
        qpb_desc c = *d;
        c.batch = count;
        const hipError_t e = qpb_launch_kkt_bwd_box(&c, Hc, xc, ac, sc, gxc, gHc, gfc, glc, guc, (hipStream_t)stream);
        return e == hipSuccess ? 0 : hip_fail(e, "qpb_solve_box_backward launch");
      },
      qpb::required(H, n * n), qpb::required(x, n), qpb::required(active, (m + 31) / 32), qpb::optional(status, 1),
      qpb::required(gx, n), qpb::optional(gH, n * n), qpb::optional(gf, n), qpb::optional(glb, n),
      qpb::optional(gub, n));
}

// ---- one H for a batch of box QPs -----------------------------------------------
// qpb_solve_box's argument rules, in its order, up to the device
static int check_box_shared(const qpb_desc *d, const double *H, const double *f, const double *x, const double *lam,
                            const uint32_t *active, const int32_t *status, bool *empty) {
  const int rc = check_desc(d);
  if (rc) return rc;
  if (d->m != 2 * d->n)
    return fail(QPB_ERR_INVALID_ARG, "qpb_solve_box_shared: m must be 2n (got n=%d m=%d)", d->n, d->m);
  *empty = d->batch == 0;
  if (*empty) return 0;
  if (!H || !f || !x || !lam || !active || !status)
    return fail(QPB_ERR_INVALID_ARG, "qpb_solve_box_shared: H, f, x, lam, active and status are required");
  return check_device();
}

extern "C" int qpb_solve_box_shared(const qpb_desc *d, const double *H, const double *f, const double *lb,
                                    const double *ub, double *x, double *lam, uint32_t *active, int32_t *status,
                                    int32_t *iters, void *stream) {
  bool empty = false;
  const int rc = check_box_shared(d, H, f, x, lam, active, status, &empty);
  if (rc || empty) return rc;
  // qpb_solve_box's class and chunks; the SH forms read H through a QP stride of 0
  const qpb::Route r = qpb::route_box_shared(d->n);
  qpb_gi_box_shared_launcher *const fn = r.kernel == qpb::Kernel::gi_box        ? qpb_launch_gi_box_shared
                                         : r.kernel == qpb::Kernel::gi_wave_box ? qpb_launch_gi_wave_box_shared
                                                                                : qpb_launch_gi_gram_box_shared;
  const long long n = d->n, m = d->m;
  return qpb::for_each_chunk(
      d->batch, r.step,
      [&](long long count, const double *fc, const double *lbc, const double *ubc, double *xc, double *lc,
          uint32_t *ac, int32_t *sc, int32_t *ic) {
        qpb_desc c = *d;
        c.batch = count;
        const hipError_t e = fn(&c, H, fc, lbc, ubc, xc, lc, ac, sc, ic, 0LL, (hipStream_t)stream);
        return e == hipSuccess ? 0 : hip_fail(e, "qpb_solve_box_shared launch");
      },
      qpb::required(f, n), qpb::optional(lb, n), qpb::optional(ub, n), qpb::required(x, n), qpb::required(lam, m),
      qpb::required(active, (m + 31) / 32), qpb::required(status, 1), qpb::optional(iters, 1));
}

// ---- that one H factored once -----------------------------------------------------
extern "C" int64_t qpb_factor_box_doubles(int32_t n) {
  if (n < 1) return fail(QPB_ERR_INVALID_ARG, "qpb_factor_box_doubles: n must be >= 1");
  if (qpb::route_box_factored(n).step == 0)
    return fail(QPB_ERR_UNSUPPORTED, "qpb_factor_box_doubles: n=%d outside the factored box kernels (n<=%d)", n,
                qpb::kBoxFactoredMaxN);
  return qpb::bxfct::layout(n).size;
}

// the rules of qpb_factor_box up to the alignment and the device
static int check_factor_box(int32_t n, const double *H, const double *bxfac) {
  if (n < 1) return fail(QPB_ERR_INVALID_ARG, "qpb_factor_box: n must be >= 1");
  if (qpb::route_box_factored(n).step == 0)
    return fail(QPB_ERR_UNSUPPORTED, "qpb_factor_box: n=%d outside the factored box kernels (n<=%d)", n,
                qpb::kBoxFactoredMaxN);
  if (!H || !bxfac) return fail(QPB_ERR_INVALID_ARG, "qpb_factor_box: H and bxfac are required");
  return 0;
}

extern "C" int qpb_factor_box(int32_t n, const double *H, double *bxfac, int32_t *fstatus, void *stream) {
  int rc = check_factor_box(n, H, bxfac);
  if (rc) return rc;
  if ((uintptr_t)bxfac & 15) return fail(QPB_ERR_INVALID_ARG, "qpb_factor_box: bxfac must be 16-byte aligned");
  rc = check_device();
  if (rc) return rc;
  qpb_gi_box_factor_launcher *const fn = qpb::route_box_factored(n).kernel == qpb::Kernel::gi_box
                                             ? qpb_launch_gi_box_factor
                                             : qpb_launch_gi_wave_box_factor;
  const hipError_t e = fn(n, H, bxfac, fstatus, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(e, "qpb_factor_box launch");
}

// qpb_solve_box_factored's argument rules, in its order, up to the alignment and the device
static int check_box_factored(const qpb_desc *d, const double *bxfac, const double *f, const double *x,
                              const double *lam, const uint32_t *active, const int32_t *status, bool *empty) {
  const int rc = check_desc(d);
  if (rc) return rc;
  if (d->m != 2 * d->n)
    return fail(QPB_ERR_INVALID_ARG, "qpb_solve_box_factored: m must be 2n (got n=%d m=%d)", d->n, d->m);
  if (d->flags != 0) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_box_factored: flags must be 0 (got %d)", d->flags);
  if (qpb::route_box_factored(d->n).step == 0)
    return fail(QPB_ERR_UNSUPPORTED, "qpb_solve_box_factored: n=%d outside the factored box kernels (n<=%d)", d->n,
                qpb::kBoxFactoredMaxN);
  *empty = d->batch == 0;
  if (*empty) return 0;
  if (!bxfac || !f || !x || !lam || !active || !status)
    return fail(QPB_ERR_INVALID_ARG, "qpb_solve_box_factored: bxfac, f, x, lam, active and status are required");
  return 0;
}

extern "C" int qpb_solve_box_factored(const qpb_desc *d, const double *bxfac, const double *f, const double *lb,
                                      const double *ub, double *x, double *lam, uint32_t *active, int32_t *status,
                                      int32_t *iters, void *stream) {
  bool empty = false;
  int rc = check_box_factored(d, bxfac, f, x, lam, active, status, &empty);
  if (rc || empty) return rc;
  if ((uintptr_t)bxfac & 15)
    return fail(QPB_ERR_INVALID_ARG, "qpb_solve_box_factored: bxfac must be 16-byte aligned");
  rc = check_device();
  if (rc) return rc;
  const qpb::Route r = qpb::route_box_factored(d->n);
  qpb_gi_box_factored_launcher *const fn =
      r.kernel == qpb::Kernel::gi_box ? qpb_launch_gi_box_factored : qpb_launch_gi_wave_box_factored;
  const long long n = d->n, m = d->m;
  // the chunk walk of the shared form: the buffer's QP stride is 0
  return qpb::for_each_chunk(
      d->batch, r.step,
      [&](long long count, const double *fc, const double *lbc, const double *ubc, double *xc, double *lc,
          uint32_t *ac, int32_t *sc, int32_t *ic) {
        qpb_desc c = *d;
        c.batch = count;
        const hipError_t e = fn(&c, bxfac, fc, lbc, ubc, xc, lc, ac, sc, ic, (hipStream_t)stream);
        return e == hipSuccess ? 0 : hip_fail(e, "qpb_solve_box_factored launch");
      },
      qpb::required(f, n), qpb::optional(lb, n), qpb::optional(ub, n), qpb::required(x, n), qpb::required(lam, m),
      qpb::required(active, (m + 31) / 32), qpb::required(status, 1), qpb::optional(iters, 1));
}

// The two passes of qpb_solve_box_shared_backward (glam == NULL: its launches
// and nothing else) and of qpb_solve_box_backward_dual on one H (glam given:
// pass 1 is the SH DU forms), after the checks.  `what` names the call.
static int box_shared_bwd_passes(const qpb_desc *d, const double *H, const double *x, const uint32_t *active,
                                 const int32_t *status, const double *gx, const double *glam, double *gH, double *gf,
                                 double *glb, double *gub, void *stream, const char *what);

extern "C" int qpb_solve_box_shared_backward(const qpb_desc *d, const double *H, const double *x,
                                             const uint32_t *active, const int32_t *status, const double *gx,
                                             double *gH, double *gf, double *glb, double *gub, void *stream) {
  static const char what[] = "qpb_solve_box_shared_backward";
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_bwd_box(d, what);
  if (rc) return rc;
  if (d->batch == 0) return 0;
  rc = check_bwd_box_arrays(H, x, active, gx, gH, gf, glb, gub, what);
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  return box_shared_bwd_passes(d, H, x, active, status, gx, nullptr, gH, gf, glb, gub, stream, what);
}

static int box_shared_bwd_passes(const qpb_desc *d, const double *H, const double *x, const uint32_t *active,
                                 const int32_t *status, const double *gx, const double *glam, double *gH, double *gf,
                                 double *glb, double *gub, void *stream, const char *what) {
  int rc = 0;
  const qpb::Route r = qpb::route_bwd_box_dual(d->n);  // (route_bwd_box_shared's, with or without glam)
  const long long n = d->n, m = d->m, B = d->batch;
  const hipStream_t st = (hipStream_t)stream;
  // pass 1 over the batch in chunks, without gH: dx goes to gf1 (the caller's gf, or the workspace's)
  auto pass1 = [&](double *gf1) {
    return qpb::for_each_chunk(
        B, r.step,
        [&](long long count, const double *xc, const uint32_t *ac, const int32_t *sc, const double *gxc,
            const double *gmc, double *gfc, double *glc, double *guc) {
          qpb_desc c = *d;
          c.batch = count;
          const hipError_t e =
              glam ? qpb_launch_kkt_bwd_box_dual(&c, 0LL, H, xc, ac, sc, gxc, gmc, nullptr, gfc, glc, guc, st)
                   : qpb_launch_kkt_bwd_box_shared(&c, 0LL, H, xc, ac, sc, gxc, nullptr, gfc, glc, guc, st);
          return e == hipSuccess ? 0 : fail(QPB_ERR_HIP, "%s launch: %s", what, hipGetErrorString(e));
        },
        qpb::required(x, n), qpb::required(active, (m + 31) / 32), qpb::optional(status, 1), qpb::required(gx, n),
        qpb::optional(glam, m), qpb::optional(gf1, n), qpb::optional(glb, n), qpb::optional(gub, n));
  };
  if (!gH) return pass1(gf);  // the sum is not wanted: pass 1 alone, no workspace
  // pass 2 is the batch sum of qpb_solve_shared_backward at m == 0: S = 1/2 sum (dx x^T + x dx^T) alone.
  // workspace: the slots, then dx (B n) where gf is not given
  qpb_desc ds = *d;
  ds.m = 0;
  const long long slot_doubles = qpb::sum_plan(B).slots * qpb::sum_slot_doubles(d->n, 0);
  const long long ws_dx = gf ? 0 : B * n;
  const hipError_t e = qpb_with_workspace(st, (size_t)(slot_doubles + ws_dx) * 8, [&](void *ws) {
    double *const slots = (double *)ws;
    double *const dx = gf ? gf : slots + slot_doubles;
    rc = pass1(dx);
    if (rc) return hipSuccess;  // reported through rc
    return qpb_launch_kkt_bwd_sum(&ds, x, dx, nullptr, nullptr, nullptr, status, slots, gH, nullptr, st);
  });
  if (rc) return rc;
  return e == hipSuccess ? 0 : fail(QPB_ERR_HIP, "%s sum launch: %s", what, hipGetErrorString(e));
}

// qpb_solve_box_backward_dual's argument rules after check_desc, up to the
// pointers: check_bwd_box's, with the shared bit beside the flags
static int check_bwd_box_dual(const qpb_desc *d, int32_t shared) {
  static const char what[] = "qpb_solve_box_backward_dual";
  if (d->m != 2 * d->n) return fail(QPB_ERR_INVALID_ARG, "%s: m must be 2n (got n=%d m=%d)", what, d->n, d->m);
  if (d->flags != 0) return fail(QPB_ERR_INVALID_ARG, "%s: flags must be 0 (got %d)", what, d->flags);
  if (shared & ~QPB_SHARED_H)
    return fail(QPB_ERR_INVALID_ARG, "%s: shared must be 0 or QPB_SHARED_H (got %d)", what, shared);
  if (qpb::route_bwd_box_dual(d->n).step == 0)
    return fail(QPB_ERR_UNSUPPORTED, "%s: n=%d outside the backward box kernels (n<=%d)", what, d->n,
                qpb::kBwdBoxDualMaxN);
  return 0;
}

extern "C" int qpb_solve_box_backward_dual(const qpb_desc *d, int32_t shared, const double *H, const double *x,
                                           const uint32_t *active, const int32_t *status, const double *gx,
                                           const double *glam, double *gH, double *gf, double *glb, double *gub,
                                           void *stream) {
  static const char what[] = "qpb_solve_box_backward_dual";
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_bwd_box_dual(d, shared);
  if (rc) return rc;
  // no cotangent on lam: the call is one of the two box backward calls, with their remaining rules
  if (!glam)
    return shared ? qpb_solve_box_shared_backward(d, H, x, active, status, gx, gH, gf, glb, gub, stream)
                  : qpb_solve_box_backward(d, H, x, active, status, gx, gH, gf, glb, gub, stream);
  if (d->batch == 0) return 0;
  rc = check_bwd_box_arrays(H, x, active, gx, gH, gf, glb, gub, what);
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  if (shared) return box_shared_bwd_passes(d, H, x, active, status, gx, glam, gH, gf, glb, gub, stream, what);
  const qpb::Route r = qpb::route_bwd_box_dual(d->n);
  const long long n = d->n, m = d->m;
  return qpb::for_each_chunk(
      d->batch, r.step,
      [&](long long count, const double *Hc, const double *xc, const uint32_t *ac, const int32_t *sc,
          const double *gxc, const double *gmc, double *gHc, double *gfc, double *glc, double *guc) {
        qpb_desc c = *d;
        c.batch = count;
        const hipError_t e =
            qpb_launch_kkt_bwd_box_dual(&c, n * n, Hc, xc, ac, sc, gxc, gmc, gHc, gfc, glc, guc, (hipStream_t)stream);
        return e == hipSuccess ? 0 : hip_fail(e, "qpb_solve_box_backward_dual launch");
      },
      qpb::required(H, n * n), qpb::required(x, n), qpb::required(active, (m + 31) / 32), qpb::optional(status, 1),
      qpb::required(gx, n), qpb::required(glam, m), qpb::optional(gH, n * n), qpb::optional(gf, n),
      qpb::optional(glb, n), qpb::optional(gub, n));
}

extern "C" int qpb_solve_sections(const qpb_desc *d, const double *H, const double *f, const double *A,
                                  const double *b, double *x, double *lam, uint32_t *active, int32_t *status,
                                  int32_t *iters, unsigned long long *sections, int64_t sections_len,
                                  void *stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  static_assert(QPB_SECTIONS_LEN == qpb::kSectionSlots * qpb::kSections, "sections buffer shape");
  if (sections && sections_len < QPB_SECTIONS_LEN)
    return fail(QPB_ERR_INVALID_ARG, "sections: the buffer must hold QPB_SECTIONS_LEN (256 x 20) counters");
  if (d->batch == 0) return 0;
  rc = check_solve_arrays(d, H, f, A, b, x, lam, active, status);
  if (rc) return rc;
  // the stamped builds exist per size class, whatever the flags; one launch
  const qpb::Route r = qpb::route(d->n, d->m, 0, false);
  const bool n16 = r.kernel == qpb::Kernel::gi_dense && d->n == 16 && d->m > 16;
  const bool wave = r.kernel == qpb::Kernel::gi_wave && d->n > 16;
  const bool gram = r.kernel == qpb::Kernel::gi_gram && d->batch <= r.step;
  if (!(n16 || wave || gram) || !sections)
    return fail(QPB_ERR_UNSUPPORTED, "sections: n=16 with 16<m<=32, 16<n<=32 with m<=64, or the n<=128 class");
  rc = check_device();
  if (rc) return rc;
  qpb_gi_sections_launcher *const fn =
      n16 ? qpb_launch_gi_sections : wave ? qpb_launch_gi_wave_sections : qpb_launch_gi_gram;
  const hipError_t e = fn(d, H, f, A, b, x, lam, active, status, iters, sections, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "qpb_solve_sections launch");
  return 0;
}

// ---- host-pointer wrappers -------------------------------------------------
struct DevBuf {
  void *p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

static hipError_t up(DevBuf &b, const void *src, size_t bytes) {
  if (!src || !bytes) return hipSuccess;
  hipError_t e = hipMalloc(&b.p, bytes);
  if (e != hipSuccess) return e;
  return hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice);
}
static hipError_t alloc(DevBuf &b, const void *dst, size_t bytes) {
  if (!dst || !bytes) return hipSuccess;
  return hipMalloc(&b.p, bytes);
}
static hipError_t down(void *dst, const DevBuf &b, size_t bytes) {
  if (!dst || !bytes) return hipSuccess;
  return hipMemcpy(dst, b.p, bytes, hipMemcpyDeviceToHost);
}

#define HIPCHK(expr, what)                  \
  do {                                      \
    hipError_t e_ = (expr);                 \
    if (e_ != hipSuccess) return hip_fail(e_, what); \
  } while (0)

// qpb_solve_host (meq < 0), qpb_solve_eq_host and qpb_solve_shared_host
// (shared >= 0: a shared operand is one matrix): copy in, solve, copy out
static int solve_host(const qpb_desc *d, int32_t meq, const double *H, const double *f, const double *A,
                      const double *b, double *x, double *lam, uint32_t *active, int32_t *status, int32_t *iters,
                      int32_t shared = -1) {
  if (d->batch == 0) return 0;
  int rc = check_device();
  if (rc) return rc;
  const size_t B = (size_t)d->batch, n = d->n, m = d->m, w = (m + 31) / 32;
  DevBuf dH, df, dA, db, dx, dl, da, ds, di;
  const size_t BH = (shared > 0 && (shared & QPB_SHARED_H)) ? 1 : B, BA = (shared > 0 && (shared & QPB_SHARED_A)) ? 1 : B;
  HIPCHK(up(dH, H, BH * n * n * 8), "H");
  HIPCHK(up(df, f, B * n * 8), "f");
  HIPCHK(up(dA, m ? A : nullptr, BA * m * n * 8), "A");
  HIPCHK(up(db, m ? b : nullptr, B * m * 8), "b");
  HIPCHK(alloc(dx, x, B * n * 8), "x");
  HIPCHK(alloc(dl, m ? lam : nullptr, B * m * 8), "lam");
  HIPCHK(alloc(da, m ? active : nullptr, B * w * 4), "active");
  HIPCHK(alloc(ds, status, B * 4), "status");
  HIPCHK(alloc(di, iters, B * 4), "iters");
  rc = meq < 0 ? qpb_solve(d, (double *)dH.p, (double *)df.p, (double *)dA.p, (double *)db.p, (double *)dx.p,
                           (double *)dl.p, (uint32_t *)da.p, (int32_t *)ds.p, (int32_t *)di.p, nullptr)
       : shared >= 0
           ? qpb_solve_shared(d, meq, shared, (double *)dH.p, (double *)df.p, (double *)dA.p, (double *)db.p,
                              (double *)dx.p, (double *)dl.p, (uint32_t *)da.p, (int32_t *)ds.p, (int32_t *)di.p,
                              nullptr)
           : qpb_solve_eq(d, meq, (double *)dH.p, (double *)df.p, (double *)dA.p, (double *)db.p, (double *)dx.p,
                              (double *)dl.p, (uint32_t *)da.p, (int32_t *)ds.p, (int32_t *)di.p, nullptr);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize(), "qpb_solve_host kernel");
  HIPCHK(down(x, dx, B * n * 8), "x D2H");
  HIPCHK(down(m ? lam : nullptr, dl, B * m * 8), "lam D2H");
  HIPCHK(down(m ? active : nullptr, da, B * w * 4), "active D2H");
  HIPCHK(down(status, ds, B * 4), "status D2H");
  HIPCHK(down(iters, di, B * 4), "iters D2H");
  return 0;
}

extern "C" int qpb_solve_host(const qpb_desc *d, const double *H, const double *f, const double *A,
                              const double *b, double *x, double *lam, uint32_t *active, int32_t *status,
                              int32_t *iters) {
  const int rc = check_desc(d);
  if (rc) return rc;
  return solve_host(d, -1, H, f, A, b, x, lam, active, status, iters);
}

extern "C" int qpb_solve_eq_host(const qpb_desc *d, int32_t meq, const double *H, const double *f, const double *A,
                                 const double *b, double *x, double *lam, uint32_t *active, int32_t *status,
                                 int32_t *iters) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_eq(d, meq);
  if (rc) return rc;
  if (d->batch > 0) {
    rc = check_solve_arrays(d, H, f, A, b, x, lam, active, status);  // host pointers: the same rules
    if (rc) return rc;
  }
  return solve_host(d, meq, H, f, A, b, x, lam, active, status, iters);
}

extern "C" int qpb_solve_shared_host(const qpb_desc *d, int32_t meq, int32_t shared, const double *H,
                                     const double *f, const double *A, const double *b, double *x, double *lam,
                                     uint32_t *active, int32_t *status, int32_t *iters) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_shared(d, meq, shared);
  if (rc) return rc;
  shared = shared_of(d, shared);
  if (shared == 0) return qpb_solve_eq_host(d, meq, H, f, A, b, x, lam, active, status, iters);
  if (meq > d->m) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_shared: meq=%d > m=%d", meq, d->m);
  if (d->batch > 0) {
    rc = check_solve_arrays(d, H, f, A, b, x, lam, active, status);  // host pointers: the same rules
    if (rc) return rc;
  }
  return solve_host(d, meq, H, f, A, b, x, lam, active, status, iters, shared);
}

// ---- a shared H and A factored once --------------------------------------------
extern "C" int64_t qpb_factor_doubles(int32_t n, int32_t m) {
  if (n < 1 || m < 0) return fail(QPB_ERR_INVALID_ARG, "qpb_factor_doubles: n must be >= 1 and m >= 0");
  if (qpb::route_factored(n, m).step == 0)
    return fail(QPB_ERR_UNSUPPORTED, "qpb_factor_doubles: n=%d m=%d outside the factored kernels (n<=%d, m<=%d)", n, m,
                qpb::kFactoredMaxN, qpb::kFactoredMaxM);
  return qpb::fct::layout(n, m).size;
}

// the rules of qpb_factor_shared up to the device: the shape as a descriptor's,
// the size limit, the pointers (fac on a 16-byte boundary: the solve's loads)
static int check_factor(int32_t n, int32_t m, const double *H, const double *A, const double *fac) {
  if (n < 1 || m < 0) return fail(QPB_ERR_INVALID_ARG, "qpb_factor_shared: n must be >= 1 and m >= 0");
  if (qpb::route_factored(n, m).step == 0)
    return fail(QPB_ERR_UNSUPPORTED, "qpb_factor_shared: n=%d m=%d outside the factored kernels (n<=%d, m<=%d)", n, m,
                qpb::kFactoredMaxN, qpb::kFactoredMaxM);
  if (!H || !fac) return fail(QPB_ERR_INVALID_ARG, "qpb_factor_shared: H and fac are required");
  if (m > 0 && !A) return fail(QPB_ERR_INVALID_ARG, "qpb_factor_shared: A is required when m > 0");
  return 0;
}

extern "C" int qpb_factor_shared(int32_t n, int32_t m, const double *H, const double *A, double *fac,
                                 int32_t *fstatus, void *stream) {
  int rc = check_factor(n, m, H, A, fac);
  if (rc) return rc;
  if ((uintptr_t)fac & 15) return fail(QPB_ERR_INVALID_ARG, "qpb_factor_shared: fac must be 16-byte aligned");
  rc = check_device();
  if (rc) return rc;
  qpb_gi_factor_launcher *const fn =
      qpb::route_factored(n, m).kernel == qpb::Kernel::gi_dense ? qpb_launch_gi_factor : qpb_launch_gi_wave_factor;
  const hipError_t e = fn(n, m, H, m > 0 ? A : nullptr, fac, fstatus, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(e, "qpb_factor_shared launch");
}

// qpb_solve_factored's argument rules after check_desc, up to batch == 0
static int check_factored(const qpb_desc *d, int32_t meq) {
  if (meq < 0) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_factored: meq < 0");
  if (d->flags != 0) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_factored: flags must be 0 (got %d)", d->flags);
  if (qpb::route_factored(d->n, d->m).step == 0)
    return fail(QPB_ERR_UNSUPPORTED, "qpb_solve_factored: n=%d m=%d outside the factored kernels (n<=%d, m<=%d)", d->n,
                d->m, qpb::kFactoredMaxN, qpb::kFactoredMaxM);
  if (meq > d->m) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_factored: meq=%d > m=%d", meq, d->m);
  return 0;
}
static int check_factored_arrays(const qpb_desc *d, const double *fac, const double *f, const double *b,
                                 const double *x, const double *lam, const uint32_t *active, const int32_t *status) {
  if (!fac || !f || !x || !status) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_factored: fac, f, x and status are required");
  if (d->m > 0 && (!b || !lam || !active))
    return fail(QPB_ERR_INVALID_ARG, "qpb_solve_factored: b, lam and active are required when m > 0");
  return 0;
}

extern "C" int qpb_solve_factored(const qpb_desc *d, int32_t meq, const double *fac, const double *f, const double *b,
                                  double *x, double *lam, uint32_t *active, int32_t *status, int32_t *iters,
                                  void *stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_factored(d, meq);
  if (rc) return rc;
  if (d->batch == 0) return 0;
  rc = check_factored_arrays(d, fac, f, b, x, lam, active, status);
  if (rc) return rc;
  if ((uintptr_t)fac & 15) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_factored: fac must be 16-byte aligned");
  rc = check_device();
  if (rc) return rc;
  const qpb::Route r = qpb::route_factored(d->n, d->m);
  qpb_gi_factored_launcher *const fn =
      r.kernel == qpb::Kernel::gi_dense ? qpb_launch_gi_factored : qpb_launch_gi_wave_factored;
  const long long n = d->n, m = d->m;
  // the chunk walk of the shared form: the buffer's QP stride is 0
  return qpb::for_each_chunk(
      d->batch, r.step,
      [&](long long count, const double *Fc, const double *fc, const double *bc, double *xc, double *lc, uint32_t *ac,
          int32_t *sc, int32_t *ic) {
        qpb_desc c = *d;
        c.batch = count;
        const hipError_t e = fn(&c, meq, Fc, fc, bc, xc, lc, ac, sc, ic, (hipStream_t)stream);
        return e == hipSuccess ? 0 : hip_fail(e, "qpb_solve_factored launch");
      },
      qpb::required(fac, 0), qpb::required(f, n), qpb::optional(b, m), qpb::required(x, n), qpb::optional(lam, m),
      qpb::optional(active, (m + 31) / 32), qpb::required(status, 1), qpb::optional(iters, 1));
}

extern "C" int qpb_factor_shared_host(int32_t n, int32_t m, const double *H, const double *A, double *fac,
                                      int32_t *fstatus) {
  int rc = check_factor(n, m, H, A, fac);  // host pointers: the same rules
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  const size_t N = n, M = m, doubles = (size_t)qpb::fct::layout(n, m).size;
  DevBuf dH, dA, dF, dS;
  HIPCHK(up(dH, H, N * N * 8), "H");
  HIPCHK(up(dA, M ? A : nullptr, M * N * 8), "A");
  HIPCHK(alloc(dF, fac, doubles * 8), "fac");
  HIPCHK(alloc(dS, fstatus, 4), "fstatus");
  rc = qpb_factor_shared(n, m, (double *)dH.p, (double *)dA.p, (double *)dF.p, (int32_t *)dS.p, nullptr);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize(), "qpb_factor_shared_host kernel");
  HIPCHK(down(fac, dF, doubles * 8), "fac D2H");
  HIPCHK(down(fstatus, dS, 4), "fstatus D2H");
  return 0;
}

extern "C" int qpb_solve_factored_host(const qpb_desc *d, int32_t meq, const double *fac, const double *f,
                                       const double *b, double *x, double *lam, uint32_t *active, int32_t *status,
                                       int32_t *iters) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_factored(d, meq);
  if (rc) return rc;
  if (d->batch == 0) return 0;
  rc = check_factored_arrays(d, fac, f, b, x, lam, active, status);  // host pointers: the same rules
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  const size_t B = (size_t)d->batch, n = d->n, m = d->m, w = (m + 31) / 32;
  DevBuf dF, df, db, dx, dl, da, ds, di;
  HIPCHK(up(dF, fac, (size_t)qpb::fct::layout(d->n, d->m).size * 8), "fac");
  HIPCHK(up(df, f, B * n * 8), "f");
  HIPCHK(up(db, m ? b : nullptr, B * m * 8), "b");
  HIPCHK(alloc(dx, x, B * n * 8), "x");
  HIPCHK(alloc(dl, m ? lam : nullptr, B * m * 8), "lam");
  HIPCHK(alloc(da, m ? active : nullptr, B * w * 4), "active");
  HIPCHK(alloc(ds, status, B * 4), "status");
  HIPCHK(alloc(di, iters, B * 4), "iters");
  rc = qpb_solve_factored(d, meq, (double *)dF.p, (double *)df.p, (double *)db.p, (double *)dx.p, (double *)dl.p,
                          (uint32_t *)da.p, (int32_t *)ds.p, (int32_t *)di.p, nullptr);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize(), "qpb_solve_factored_host kernel");
  HIPCHK(down(x, dx, B * n * 8), "x D2H");
  HIPCHK(down(m ? lam : nullptr, dl, B * m * 8), "lam D2H");
  HIPCHK(down(m ? active : nullptr, da, B * w * 4), "active D2H");
  HIPCHK(down(status, ds, B * 4), "status D2H");
  HIPCHK(down(iters, di, B * 4), "iters D2H");
  return 0;
}

// ---- the backward on a buffer of its own ----------------------------------------
extern "C" int64_t qpb_factor_backward_doubles(int32_t n, int32_t m) {
  if (n < 1 || m < 0) return fail(QPB_ERR_INVALID_ARG, "qpb_factor_backward_doubles: n must be >= 1 and m >= 0");
  if (qpb::route_factored_bwd(n, m).step == 0)
    return fail(QPB_ERR_UNSUPPORTED,
                "qpb_factor_backward_doubles: n=%d m=%d outside the factored backward kernels (n<=%d, m<=%d)", n, m,
                qpb::kFactoredBwdMaxN, qpb::kFactoredBwdMaxM);
  return qpb::bfct::layout(n, m).size;
}

// the rules of qpb_factor_shared_backward up to the device: check_factor's
static int check_factor_bwd(int32_t n, int32_t m, const double *H, const double *A, const double *bfac) {
  if (n < 1 || m < 0) return fail(QPB_ERR_INVALID_ARG, "qpb_factor_shared_backward: n must be >= 1 and m >= 0");
  if (qpb::route_factored_bwd(n, m).step == 0)
    return fail(QPB_ERR_UNSUPPORTED,
                "qpb_factor_shared_backward: n=%d m=%d outside the factored backward kernels (n<=%d, m<=%d)", n, m,
                qpb::kFactoredBwdMaxN, qpb::kFactoredBwdMaxM);
  if (!H || !bfac) return fail(QPB_ERR_INVALID_ARG, "qpb_factor_shared_backward: H and bfac are required");
  if (m > 0 && !A) return fail(QPB_ERR_INVALID_ARG, "qpb_factor_shared_backward: A is required when m > 0");
  return 0;
}

extern "C" int qpb_factor_shared_backward(int32_t n, int32_t m, const double *H, const double *A, double *bfac,
                                          int32_t *fstatus, void *stream) {
  int rc = check_factor_bwd(n, m, H, A, bfac);
  if (rc) return rc;
  if ((uintptr_t)bfac & 15)
    return fail(QPB_ERR_INVALID_ARG, "qpb_factor_shared_backward: bfac must be 16-byte aligned");
  rc = check_device();
  if (rc) return rc;
  const hipError_t e = qpb_launch_kkt_bwd_factor(n, m, H, m > 0 ? A : nullptr, bfac, fstatus, (hipStream_t)stream);
  return e == hipSuccess ? 0 : hip_fail(e, "qpb_factor_shared_backward launch");
}

// qpb_solve_factored_backward's argument rules after check_desc, up to batch == 0
// (and qpb_solve_factored_backward_dual's: `what` names the call)
static int check_factored_bwd(const qpb_desc *d, const char *what = "qpb_solve_factored_backward") {
  if (d->flags != 0) return fail(QPB_ERR_INVALID_ARG, "%s: flags must be 0 (got %d)", what, d->flags);
  if (qpb::route_factored_bwd(d->n, d->m).step == 0)
    return fail(QPB_ERR_UNSUPPORTED, "%s: n=%d m=%d outside the factored backward kernels (n<=%d, m<=%d)", what, d->n,
                d->m, qpb::kFactoredBwdMaxN, qpb::kFactoredBwdMaxM);
  return 0;
}
static int check_factored_bwd_arrays(const qpb_desc *d, const double *bfac, const double *x, const double *lam,
                                     const uint32_t *active, const double *gx, const double *gH, const double *gf,
                                     const double *gA, const double *gb,
                                     const char *what = "qpb_solve_factored_backward") {
  if (!bfac || !x || !gx) return fail(QPB_ERR_INVALID_ARG, "%s: bfac, x and gx are required", what);
  if (d->m > 0 && (!lam || !active))
    return fail(QPB_ERR_INVALID_ARG, "%s: lam and active are required when m > 0", what);
  if (!gH && !gf && !(d->m > 0 && (gA || gb)))
    return fail(QPB_ERR_INVALID_ARG, "%s: at least one of gH, gf, gA and gb is required", what);
  return 0;
}

// qpb_solve_factored_backward (glam == NULL: its launches and nothing else) and
// qpb_solve_factored_backward_dual (glam given, m > 0: pass 1 is the DU forms).
// qpb_solve_shared_backward's body with both operands shared and the factored
// pass 1: the same chunk walk, workspace and pass 2.  `what` names the call.
static int factored_bwd(const qpb_desc *d, const double *bfac, const double *x, const double *lam,
                        const uint32_t *active, const int32_t *status, const double *gx, const double *glam,
                        double *gH, double *gf, double *gA, double *gb, void *stream, const char *what) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_factored_bwd(d, what);
  if (rc) return rc;
  if (d->batch == 0) return 0;
  rc = check_factored_bwd_arrays(d, bfac, x, lam, active, gx, gH, gf, gA, gb, what);
  if (rc) return rc;
  if ((uintptr_t)bfac & 15) return fail(QPB_ERR_INVALID_ARG, "%s: bfac must be 16-byte aligned", what);
  rc = check_device();
  if (rc) return rc;
  const qpb::Route r = qpb::route_factored_bwd_dual(d->n, d->m);  // (route_factored_bwd's, with or without glam)
  const long long n = d->n, m = d->m, B = d->batch;
  if (m == 0) gA = gb = nullptr;  // ignored
  const hipStream_t st = (hipStream_t)stream;
  // pass 1 over the batch in chunks (the buffer's QP stride is 0); gf1 and gb1
  // are the caller's, or the workspace's where pass 2 needs them
  auto pass1 = [&](double *gf1, double *gb1) {
    return qpb::for_each_chunk(
        B, r.step,
        [&](long long count, const double *Fc, const double *xc, const double *lc, const uint32_t *ac,
            const int32_t *sc, const double *gxc, const double *glc, double *gfc, double *gbc) {
          qpb_desc c = *d;
          c.batch = count;
          const hipError_t e = glam ? qpb_launch_kkt_bwd_factored_dual(&c, Fc, xc, lc, ac, sc, gxc, glc, gfc, gbc, st)
                                    : qpb_launch_kkt_bwd_factored(&c, Fc, xc, lc, ac, sc, gxc, gfc, gbc, st);
          return e == hipSuccess ? 0 : fail(QPB_ERR_HIP, "%s launch: %s", what, hipGetErrorString(e));
        },
        qpb::required(bfac, 0), qpb::required(x, n), qpb::optional(lam, m), qpb::optional(active, (m + 31) / 32),
        qpb::optional(status, 1), qpb::required(gx, n), qpb::optional(glam, m), qpb::optional(gf1, n),
        qpb::optional(gb1, m));
  };
  if (!gH && !gA) return pass1(gf, gb);  // the summed gradients are not wanted: pass 1 alone
  // workspace, as qpb_solve_shared_backward's: the slots, then dx (B n) where gf
  // is not given, then gb (B m) where gA is summed and gb is not given
  const long long slot_doubles = qpb::sum_plan(B).slots * qpb::sum_slot_doubles(d->n, d->m);
  const long long ws_dx = gf ? 0 : B * n, ws_gb = (gA && !gb) ? B * m : 0;
  const hipError_t e = qpb_with_workspace(st, (size_t)(slot_doubles + ws_dx + ws_gb) * 8, [&](void *ws) {
    double *const slots = (double *)ws;
    double *const dx = gf ? gf : slots + slot_doubles;
    double *const gbs = gb ? gb : gA ? slots + slot_doubles + ws_dx : nullptr;
    rc = pass1(dx, gbs);
    if (rc) return hipSuccess;  // reported through rc
    return qpb_launch_kkt_bwd_sum(d, x, dx, gbs, lam, active, status, slots, gH, gA, st);
  });
  if (rc) return rc;
  return e == hipSuccess ? 0 : fail(QPB_ERR_HIP, "%s sum launch: %s", what, hipGetErrorString(e));
}

extern "C" int qpb_solve_factored_backward(const qpb_desc *d, const double *bfac, const double *x, const double *lam,
                                           const uint32_t *active, const int32_t *status, const double *gx,
                                           double *gH, double *gf, double *gA, double *gb, void *stream) {
  return factored_bwd(d, bfac, x, lam, active, status, gx, nullptr, gH, gf, gA, gb, stream,
                      "qpb_solve_factored_backward");
}

extern "C" int qpb_solve_factored_backward_dual(const qpb_desc *d, const double *bfac, const double *x,
                                                const double *lam, const uint32_t *active, const int32_t *status,
                                                const double *gx, const double *glam, double *gH, double *gf,
                                                double *gA, double *gb, void *stream) {
  // no cotangent on lam: the call is qpb_solve_factored_backward
  if (!glam || (d && d->m == 0))
    return qpb_solve_factored_backward(d, bfac, x, lam, active, status, gx, gH, gf, gA, gb, stream);
  return factored_bwd(d, bfac, x, lam, active, status, gx, glam, gH, gf, gA, gb, stream,
                      "qpb_solve_factored_backward_dual");
}

extern "C" int qpb_factor_shared_backward_host(int32_t n, int32_t m, const double *H, const double *A, double *bfac,
                                               int32_t *fstatus) {
  int rc = check_factor_bwd(n, m, H, A, bfac);  // host pointers: the same rules
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  const size_t N = n, M = m, doubles = (size_t)qpb::bfct::layout(n, m).size;
  DevBuf dH, dA, dF, dS;
  HIPCHK(up(dH, H, N * N * 8), "H");
  HIPCHK(up(dA, M ? A : nullptr, M * N * 8), "A");
  HIPCHK(alloc(dF, bfac, doubles * 8), "bfac");
  HIPCHK(alloc(dS, fstatus, 4), "fstatus");
  rc = qpb_factor_shared_backward(n, m, (double *)dH.p, (double *)dA.p, (double *)dF.p, (int32_t *)dS.p, nullptr);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize(), "qpb_factor_shared_backward_host kernel");
  HIPCHK(down(bfac, dF, doubles * 8), "bfac D2H");
  HIPCHK(down(fstatus, dS, 4), "fstatus D2H");
  return 0;
}

// qpb_solve_factored_backward_host and qpb_solve_factored_backward_dual_host
// (glam, may be NULL): copy in, run, copy out
static int factored_bwd_host(const qpb_desc *d, const double *bfac, const double *x, const double *lam,
                             const uint32_t *active, const int32_t *status, const double *gx, const double *glam,
                             double *gH, double *gf, double *gA, double *gb, const char *what) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_factored_bwd(d, what);
  if (rc) return rc;
  if (d->batch == 0) return 0;
  rc = check_factored_bwd_arrays(d, bfac, x, lam, active, gx, gH, gf, gA, gb, what);  // host pointers: the same rules
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  const size_t B = (size_t)d->batch, n = d->n, m = d->m, w = (m + 31) / 32;
  DevBuf dF, dx, dl, da, ds, dg, dgl, oH, of, oA, ob;
  HIPCHK(up(dF, bfac, (size_t)qpb::bfct::layout(d->n, d->m).size * 8), "bfac");
  HIPCHK(up(dx, x, B * n * 8), "x");
  HIPCHK(up(dl, m ? lam : nullptr, B * m * 8), "lam");
  HIPCHK(up(da, m ? active : nullptr, B * w * 4), "active");
  HIPCHK(up(ds, status, B * 4), "status");
  HIPCHK(up(dg, gx, B * n * 8), "gx");
  HIPCHK(up(dgl, m ? glam : nullptr, B * m * 8), "glam");
  HIPCHK(alloc(oH, gH, n * n * 8), "gH");
  HIPCHK(alloc(of, gf, B * n * 8), "gf");
  HIPCHK(alloc(oA, m ? gA : nullptr, m * n * 8), "gA");
  HIPCHK(alloc(ob, m ? gb : nullptr, B * m * 8), "gb");
  rc = qpb_solve_factored_backward_dual(d, (double *)dF.p, (double *)dx.p, (double *)dl.p, (uint32_t *)da.p,
                                        (int32_t *)ds.p, (double *)dg.p, (double *)dgl.p, (double *)oH.p,
                                        (double *)of.p, (double *)oA.p, (double *)ob.p, nullptr);
  if (rc) return rc;
  if (const hipError_t e = hipDeviceSynchronize(); e != hipSuccess)
    return fail(QPB_ERR_HIP, "%s_host kernel: %s", what, hipGetErrorString(e));
  HIPCHK(down(gH, oH, n * n * 8), "gH D2H");
  HIPCHK(down(gf, of, B * n * 8), "gf D2H");
  HIPCHK(down(m ? gA : nullptr, oA, m * n * 8), "gA D2H");
  HIPCHK(down(m ? gb : nullptr, ob, B * m * 8), "gb D2H");
  return 0;
}

extern "C" int qpb_solve_factored_backward_host(const qpb_desc *d, const double *bfac, const double *x,
                                                const double *lam, const uint32_t *active, const int32_t *status,
                                                const double *gx, double *gH, double *gf, double *gA, double *gb) {
  return factored_bwd_host(d, bfac, x, lam, active, status, gx, nullptr, gH, gf, gA, gb,
                           "qpb_solve_factored_backward");
}

extern "C" int qpb_solve_factored_backward_dual_host(const qpb_desc *d, const double *bfac, const double *x,
                                                     const double *lam, const uint32_t *active,
                                                     const int32_t *status, const double *gx, const double *glam,
                                                     double *gH, double *gf, double *gA, double *gb) {
  return factored_bwd_host(d, bfac, x, lam, active, status, gx, glam, gH, gf, gA, gb,
                           glam ? "qpb_solve_factored_backward_dual" : "qpb_solve_factored_backward");
}

// ---- two-sided rows bl <= A x <= bu -------------------------------------------
// qpb_solve_range's argument rules after check_desc, up to batch == 0
static int check_range(const qpb_desc *d, int32_t meq, int32_t shared) {
  if (meq < 0) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_range: meq < 0");
  if (d->flags != 0) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_range: flags must be 0 (got %d)", d->flags);
  if (shared & ~(QPB_SHARED_H | QPB_SHARED_A))
    return fail(QPB_ERR_INVALID_ARG, "qpb_solve_range: shared must be a combination of QPB_SHARED_H and QPB_SHARED_A (got %d)",
                shared);
  if (d->n > qpb::kRangeMaxN || d->m > qpb::kRangeMaxM)
    return fail(QPB_ERR_UNSUPPORTED, "qpb_solve_range: n=%d m=%d outside the kernels with range rows (n<=%d, m<=%d)",
                d->n, d->m, qpb::kRangeMaxN, qpb::kRangeMaxM);
  if (meq > d->m) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_range: meq=%d > m=%d", meq, d->m);
  return 0;
}
// ... and the pointers (m > 0; device or host)
static int check_range_arrays(const double *H, const double *f, const double *A, const double *bl, const double *bu,
                              const double *x, const double *lam, const uint32_t *active, const int32_t *status) {
  if (!H || !f || !x || !status) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_range: H, f, x and status are required");
  if (!A || !lam || !active || (!bl && !bu))
    return fail(QPB_ERR_INVALID_ARG, "qpb_solve_range: A, lam, active and at least one of bl and bu are required when m > 0");
  return 0;
}

extern "C" int qpb_solve_range(const qpb_desc *d, int32_t meq, int32_t shared, const double *H, const double *f,
                               const double *A, const double *bl, const double *bu, double *x, double *lam,
                               uint32_t *active, uint32_t *lower, int32_t *status, int32_t *iters, void *stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_range(d, meq, shared);
  if (rc) return rc;
  // no rows: the call is qpb_solve (one H for the batch: qpb_solve_shared), launch for launch
  if (d->m == 0)
    return qpb_solve_shared(d, 0, shared, H, f, nullptr, nullptr, x, lam, active, status, iters, stream);
  if (d->batch == 0) return 0;
  rc = check_range_arrays(H, f, A, bl, bu, x, lam, active, status);
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  const qpb::Route r = qpb::route_range(d->n, d->m);
  qpb_gi_range_launcher *const fn = r.kernel == qpb::Kernel::gi_dense ? qpb_launch_gi_range : qpb_launch_gi_wave_range;
  const long long n = d->n, m = d->m;
  // a shared operand's QP stride is 0, in the kernels and in the chunk walk
  const long long sH = (shared & QPB_SHARED_H) ? 0 : n * n, sA = (shared & QPB_SHARED_A) ? 0 : m * n;
  return qpb::for_each_chunk(
      d->batch, r.step,
      [&](long long count, const double *Hc, const double *fc, const double *Ac, const double *blc, const double *buc,
          double *xc, double *lc, uint32_t *ac, uint32_t *wc, int32_t *sc, int32_t *ic) {
        qpb_desc c = *d;
        c.batch = count;
        const hipError_t e = fn(&c, meq, sH, sA, Hc, fc, Ac, blc, buc, xc, lc, ac, wc, sc, ic, (hipStream_t)stream);
        return e == hipSuccess ? 0 : hip_fail(e, "qpb_solve_range launch");
      },
      qpb::required(H, sH), qpb::required(f, n), qpb::required(A, sA), qpb::optional(bl, m), qpb::optional(bu, m),
      qpb::required(x, n), qpb::required(lam, m), qpb::required(active, (m + 31) / 32),
      qpb::optional(lower, (m + 31) / 32), qpb::required(status, 1), qpb::optional(iters, 1));
}

extern "C" int qpb_solve_range_host(const qpb_desc *d, int32_t meq, int32_t shared, const double *H, const double *f,
                                    const double *A, const double *bl, const double *bu, double *x, double *lam,
                                    uint32_t *active, uint32_t *lower, int32_t *status, int32_t *iters) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_range(d, meq, shared);
  if (rc) return rc;
  if (d->m == 0) return qpb_solve_shared_host(d, 0, shared, H, f, nullptr, nullptr, x, lam, active, status, iters);
  if (d->batch == 0) return 0;
  rc = check_range_arrays(H, f, A, bl, bu, x, lam, active, status);  // host pointers: the same rules
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  const size_t B = (size_t)d->batch, n = d->n, m = d->m, w = (m + 31) / 32;
  const size_t BH = (shared & QPB_SHARED_H) ? 1 : B, BA = (shared & QPB_SHARED_A) ? 1 : B;
  DevBuf dH, df, dA, dbl, dbu, dx, dl, da, dw, ds, di;
  HIPCHK(up(dH, H, BH * n * n * 8), "H");
  HIPCHK(up(df, f, B * n * 8), "f");
  HIPCHK(up(dA, A, BA * m * n * 8), "A");
  HIPCHK(up(dbl, bl, B * m * 8), "bl");
  HIPCHK(up(dbu, bu, B * m * 8), "bu");
  HIPCHK(alloc(dx, x, B * n * 8), "x");
  HIPCHK(alloc(dl, lam, B * m * 8), "lam");
  HIPCHK(alloc(da, active, B * w * 4), "active");
  HIPCHK(alloc(dw, lower, B * w * 4), "lower");
  HIPCHK(alloc(ds, status, B * 4), "status");
  HIPCHK(alloc(di, iters, B * 4), "iters");
  rc = qpb_solve_range(d, meq, shared, (double *)dH.p, (double *)df.p, (double *)dA.p, (double *)dbl.p,
                       (double *)dbu.p, (double *)dx.p, (double *)dl.p, (uint32_t *)da.p, (uint32_t *)dw.p,
                       (int32_t *)ds.p, (int32_t *)di.p, nullptr);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize(), "qpb_solve_range_host kernel");
  HIPCHK(down(x, dx, B * n * 8), "x D2H");
  HIPCHK(down(lam, dl, B * m * 8), "lam D2H");
  HIPCHK(down(active, da, B * w * 4), "active D2H");
  HIPCHK(down(lower, dw, B * w * 4), "lower D2H");
  HIPCHK(down(status, ds, B * 4), "status D2H");
  HIPCHK(down(iters, di, B * 4), "iters D2H");
  return 0;
}

// ---- two-sided rows beside variable bounds ---------------------------------------
// qpb_solve_range_box's argument rules after check_desc (d->m is mg), up to batch == 0
static int check_range_box(const qpb_desc *d, int32_t meq, int32_t shared) {
  if (meq < 0) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_range_box: meq < 0");
  if (d->flags != 0) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_range_box: flags must be 0 (got %d)", d->flags);
  if (shared & ~(QPB_SHARED_H | QPB_SHARED_A))
    return fail(QPB_ERR_INVALID_ARG,
                "qpb_solve_range_box: shared must be a combination of QPB_SHARED_H and QPB_SHARED_A (got %d)", shared);
  if (qpb::route_range_box(d->n, d->m).step == 0)
    return fail(QPB_ERR_UNSUPPORTED,
                "qpb_solve_range_box: n=%d mg=%d outside the kernels with range rows beside a box (n<=%d, mg+n<=%d)",
                d->n, d->m, qpb::kRangeBoxMaxN, qpb::kRangeBoxMaxRows);
  if (meq > d->m) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_range_box: meq=%d > mg=%d", meq, d->m);
  return 0;
}
// ... and the pointers (device or host)
static int check_range_box_arrays(const qpb_desc *d, const double *H, const double *f, const double *G,
                                  const double *bl, const double *bu, const double *lb, const double *ub,
                                  const double *x, const double *lam, const uint32_t *active, const int32_t *status) {
  if (!H || !f || !x || !lam || !active || !status)
    return fail(QPB_ERR_INVALID_ARG, "qpb_solve_range_box: H, f, x, lam, active and status are required");
  if (d->m > 0 && !G) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_range_box: G is required when mg > 0");
  if (!bl && !bu && !lb && !ub)
    return fail(QPB_ERR_INVALID_ARG, "qpb_solve_range_box: at least one of bl, bu, lb and ub is required");
  return 0;
}

extern "C" int qpb_solve_range_box(const qpb_desc *d, int32_t meq, int32_t shared, const double *H, const double *f,
                                   const double *G, const double *bl, const double *bu, const double *lb,
                                   const double *ub, double *x, double *lam, uint32_t *active, uint32_t *lower,
                                   int32_t *status, int32_t *iters, void *stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_range_box(d, meq, shared);
  if (rc) return rc;
  if (d->batch == 0) return 0;
  rc = check_range_box_arrays(d, H, f, G, bl, bu, lb, ub, x, lam, active, status);
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  const qpb::Route r = qpb::route_range_box(d->n, d->m);
  qpb_gi_range_box_launcher *const fn =
      r.kernel == qpb::Kernel::gi_dense ? qpb_launch_gi_range_box : qpb_launch_gi_wave_range_box;
  // the kernels count all the rows, m' = mg + n (the default max_iter is the materialised problem's)
  const long long n = d->n, mg = d->m, m = mg + n;
  // a shared operand's QP stride is 0, in the kernels and in the chunk walk (mg == 0: no G at all)
  const long long sH = (shared & QPB_SHARED_H) ? 0 : n * n, sG = (shared & QPB_SHARED_A) ? 0 : mg * n;
  return qpb::for_each_chunk(
      d->batch, r.step,
      [&](long long count, const double *Hc, const double *fc, const double *Gc, const double *blc, const double *buc,
          const double *lbc, const double *ubc, double *xc, double *lc, uint32_t *ac, uint32_t *wc, int32_t *sc,
          int32_t *ic) {
        qpb_desc c = *d;
        c.batch = count;
        c.m = (int32_t)m;
        const hipError_t e = fn(&c, (int)mg, meq, sH, sG, Hc, fc, Gc, blc, buc, lbc, ubc, xc, lc, ac, wc, sc, ic,
                                (hipStream_t)stream);
        return e == hipSuccess ? 0 : hip_fail(e, "qpb_solve_range_box launch");
      },
      qpb::required(H, sH), qpb::required(f, n), qpb::optional(G, sG), qpb::optional(bl, mg), qpb::optional(bu, mg),
      qpb::optional(lb, n), qpb::optional(ub, n), qpb::required(x, n), qpb::required(lam, m),
      qpb::required(active, (m + 31) / 32), qpb::optional(lower, (m + 31) / 32), qpb::required(status, 1),
      qpb::optional(iters, 1));
}

extern "C" int qpb_solve_range_box_host(const qpb_desc *d, int32_t meq, int32_t shared, const double *H,
                                        const double *f, const double *G, const double *bl, const double *bu,
                                        const double *lb, const double *ub, double *x, double *lam, uint32_t *active,
                                        uint32_t *lower, int32_t *status, int32_t *iters) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_range_box(d, meq, shared);
  if (rc) return rc;
  if (d->batch == 0) return 0;
  rc = check_range_box_arrays(d, H, f, G, bl, bu, lb, ub, x, lam, active, status);  // host pointers: the same rules
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  const size_t B = (size_t)d->batch, n = d->n, mg = d->m, m = mg + n, w = (m + 31) / 32;
  const size_t BH = (shared & QPB_SHARED_H) ? 1 : B, BG = (shared & QPB_SHARED_A) ? 1 : B;
  DevBuf dH, df, dG, dbl, dbu, dlb, dub, dx, dl, da, dw, ds, di;
  HIPCHK(up(dH, H, BH * n * n * 8), "H");
  HIPCHK(up(df, f, B * n * 8), "f");
  if (mg > 0) {
    HIPCHK(up(dG, G, BG * mg * n * 8), "G");
    HIPCHK(up(dbl, bl, B * mg * 8), "bl");
    HIPCHK(up(dbu, bu, B * mg * 8), "bu");
  }
  HIPCHK(up(dlb, lb, B * n * 8), "lb");
  HIPCHK(up(dub, ub, B * n * 8), "ub");
  HIPCHK(alloc(dx, x, B * n * 8), "x");
  HIPCHK(alloc(dl, lam, B * m * 8), "lam");
  HIPCHK(alloc(da, active, B * w * 4), "active");
  HIPCHK(alloc(dw, lower, B * w * 4), "lower");
  HIPCHK(alloc(ds, status, B * 4), "status");
  HIPCHK(alloc(di, iters, B * 4), "iters");
  // (mg == 0: bl and bu have no element; a side counts as given if the caller gave it)
  rc = qpb_solve_range_box(d, meq, shared, (double *)dH.p, (double *)df.p, (double *)dG.p,
                           mg > 0 ? (double *)dbl.p : bl, mg > 0 ? (double *)dbu.p : bu, (double *)dlb.p,
                           (double *)dub.p, (double *)dx.p, (double *)dl.p, (uint32_t *)da.p, (uint32_t *)dw.p,
                           (int32_t *)ds.p, (int32_t *)di.p, nullptr);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize(), "qpb_solve_range_box_host kernel");
  HIPCHK(down(x, dx, B * n * 8), "x D2H");
  HIPCHK(down(lam, dl, B * m * 8), "lam D2H");
  HIPCHK(down(active, da, B * w * 4), "active D2H");
  HIPCHK(down(lower, dw, B * w * 4), "lower D2H");
  HIPCHK(down(status, ds, B * 4), "status D2H");
  HIPCHK(down(iters, di, B * 4), "iters D2H");
  return 0;
}

// ---- the backward of two-sided rows beside variable bounds -------------------------
// qpb_solve_range_box_backward's argument rules after check_desc (d->m is mg), up to batch == 0
static int check_range_box_bwd(const qpb_desc *d, int32_t shared) {
  if (d->flags != 0)
    return fail(QPB_ERR_INVALID_ARG, "qpb_solve_range_box_backward: flags must be 0 (got %d)", d->flags);
  if (shared & ~(QPB_SHARED_H | QPB_SHARED_A))
    return fail(QPB_ERR_INVALID_ARG,
                "qpb_solve_range_box_backward: shared must be a combination of QPB_SHARED_H and QPB_SHARED_A (got %d)",
                shared);
  if (qpb::route_bwd_range_box(d->n, d->m).step == 0)
    return fail(QPB_ERR_UNSUPPORTED,
                "qpb_solve_range_box_backward: n=%d mg=%d outside the backward kernels with a box (n<=%d, mg+n<=%d)",
                d->n, d->m, qpb::kBwdRangeBoxMaxN, qpb::kBwdRangeBoxMaxRows);
  return 0;
}
// ... and the pointers (device or host)
static int check_range_box_bwd_arrays(const qpb_desc *d, const double *H, const double *G, const double *x,
                                      const double *lam, const uint32_t *active, const uint32_t *lower,
                                      const double *gx, const double *gH, const double *gf, const double *gG,
                                      const double *gbl, const double *gbu, const double *glb, const double *gub) {
  if (!H || !x || !lam || !active || !gx)
    return fail(QPB_ERR_INVALID_ARG, "qpb_solve_range_box_backward: H, x, lam, active and gx are required");
  if (d->m > 0 && !G) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_range_box_backward: G is required when mg > 0");
  if (!lower && (gbl || glb))
    return fail(QPB_ERR_INVALID_ARG, "qpb_solve_range_box_backward: lower is required when gbl or glb is given");
  if (!gH && !gf && !glb && !gub && !(d->m > 0 && (gG || gbl || gbu)))
    return fail(QPB_ERR_INVALID_ARG,
                "qpb_solve_range_box_backward: at least one of gH, gf, gG, gbl, gbu, glb and gub is required");
  return 0;
}

extern "C" int qpb_solve_range_box_backward(const qpb_desc *d, int32_t shared, const double *H, const double *G,
                                            const double *x, const double *lam, const uint32_t *active,
                                            const uint32_t *lower, const int32_t *status, const double *gx,
                                            const double *glam, double *gH, double *gf, double *gG, double *gbl,
                                            double *gbu, double *glb, double *gub, void *stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_range_box_bwd(d, shared);
  if (rc) return rc;
  if (d->batch == 0) return 0;
  rc = check_range_box_bwd_arrays(d, H, G, x, lam, active, lower, gx, gH, gf, gG, gbl, gbu, glb, gub);
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  shared = shared_of(d, shared);  // (mg == 0: no G to share)
  // the kernels count all the rows, m' = mg + n: the class and the chunks of the call on [G; I]
  const qpb::Route r = qpb::route_bwd_range_box(d->n, d->m);
  const long long n = d->n, mg = d->m, m = mg + n, B = d->batch, w = (m + 31) / 32;
  if (mg == 0) gG = gbl = gbu = nullptr;  // ignored
  const long long sH = (shared & QPB_SHARED_H) ? 0 : n * n, sG = (shared & QPB_SHARED_A) ? 0 : mg * n;
  // the gradients pass 2 sums; pass 1 is launched without them
  double *const sumH = (shared & QPB_SHARED_H) ? gH : nullptr, *const sumG = (shared & QPB_SHARED_A) ? gG : nullptr;
  double *const gH1 = (shared & QPB_SHARED_H) ? nullptr : gH, *const gG1 = (shared & QPB_SHARED_A) ? nullptr : gG;
  const hipStream_t st = (hipStream_t)stream;
  qpb_desc dm = *d;
  dm.m = (int32_t)m;
  // pass 1 over the batch in chunks; gf1 is the caller's, or the workspace's where pass 2 needs it, gbw the workspace's
  auto pass1 = [&](double *gf1, double *gbw) {
    return qpb::for_each_chunk(
        B, r.step,
        [&](long long count, const double *Hc, const double *Gc, const double *xc, const double *lc,
            const uint32_t *ac, const uint32_t *wc, const int32_t *sc, const double *gxc, const double *glc,
            double *gHc, double *gfc, double *gGc, double *gblc, double *gbuc, double *glbc, double *gubc,
            double *gbwc) {
          qpb_desc c = dm;
          c.batch = count;
          const hipError_t e = qpb_launch_kkt_bwd_range_box(&c, (int)mg, sH, sG, Hc, Gc, xc, lc, ac, wc, sc, gxc, glc,
                                                            gHc, gfc, gGc, gblc, gbuc, glbc, gubc, gbwc, st);
          return e == hipSuccess ? 0 : hip_fail(e, "qpb_solve_range_box_backward launch");
        },
        qpb::required(H, sH), qpb::optional(G, sG), qpb::required(x, n), qpb::required(lam, m),
        qpb::required(active, w), qpb::optional(lower, w), qpb::optional(status, 1), qpb::required(gx, n),
        qpb::optional(glam, m), qpb::optional(gH1, n * n), qpb::optional(gf1, n), qpb::optional(gG1, mg * n),
        qpb::optional(gbl, mg), qpb::optional(gbu, mg), qpb::optional(glb, n), qpb::optional(gub, n),
        qpb::optional(gbw, mg));
  };
  if (!sumH && !sumG) return pass1(gf, nullptr);  // the summed gradients are not wanted: pass 1 alone
  // workspace: the slots, then dx (B n) where gf is not given, then pass 1's
  // unrouted gb of the rows of G (B mg) where gG is summed
  const long long slot_doubles = qpb::sum_plan(B).slots * qpb::sum_slot_doubles(d->n, (int)mg);
  const long long ws_dx = gf ? 0 : B * n, ws_gb = sumG ? B * mg : 0;
  const hipError_t e = qpb_with_workspace(st, (size_t)(slot_doubles + ws_dx + ws_gb) * 8, [&](void *ws) {
    double *const slots = (double *)ws;
    double *const dx = gf ? gf : slots + slot_doubles;
    double *const gbw = sumG ? slots + slot_doubles + ws_dx : nullptr;
    rc = pass1(dx, gbw);
    if (rc) return hipSuccess;  // reported through rc
    return qpb_launch_kkt_bwd_sum_range_box(&dm, (int)mg, x, dx, gbw, lam, active, status, slots, sumH, sumG, st);
  });
  if (rc) return rc;
  return e == hipSuccess ? 0 : hip_fail(e, "qpb_solve_range_box_backward sum launch");
}

extern "C" int qpb_solve_range_box_backward_host(const qpb_desc *d, int32_t shared, const double *H, const double *G,
                                                 const double *x, const double *lam, const uint32_t *active,
                                                 const uint32_t *lower, const int32_t *status, const double *gx,
                                                 const double *glam, double *gH, double *gf, double *gG, double *gbl,
                                                 double *gbu, double *glb, double *gub) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_range_box_bwd(d, shared);
  if (rc) return rc;
  if (d->batch == 0) return 0;
  // host pointers: the same rules
  rc = check_range_box_bwd_arrays(d, H, G, x, lam, active, lower, gx, gH, gf, gG, gbl, gbu, glb, gub);
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  shared = shared_of(d, shared);
  const size_t B = (size_t)d->batch, n = d->n, mg = d->m, m = mg + n, w = (m + 31) / 32;
  const size_t BH = (shared & QPB_SHARED_H) ? 1 : B, BG = (shared & QPB_SHARED_A) ? 1 : B;
  DevBuf dH, dG, dx, dl, da, dw, ds, dg, dgl, oH, of, oG, obl, obu, olb, oub;
  HIPCHK(up(dH, H, BH * n * n * 8), "H");
  HIPCHK(up(dG, mg ? G : nullptr, BG * mg * n * 8), "G");
  HIPCHK(up(dx, x, B * n * 8), "x");
  HIPCHK(up(dl, lam, B * m * 8), "lam");
  HIPCHK(up(da, active, B * w * 4), "active");
  HIPCHK(up(dw, lower, B * w * 4), "lower");
  HIPCHK(up(ds, status, B * 4), "status");
  HIPCHK(up(dg, gx, B * n * 8), "gx");
  HIPCHK(up(dgl, glam, B * m * 8), "glam");
  HIPCHK(alloc(oH, gH, BH * n * n * 8), "gH");
  HIPCHK(alloc(of, gf, B * n * 8), "gf");
  HIPCHK(alloc(oG, mg ? gG : nullptr, BG * mg * n * 8), "gG");
  HIPCHK(alloc(obl, gbl, B * mg * 8), "gbl");
  HIPCHK(alloc(obu, gbu, B * mg * 8), "gbu");
  HIPCHK(alloc(olb, glb, B * n * 8), "glb");
  HIPCHK(alloc(oub, gub, B * n * 8), "gub");
  rc = qpb_solve_range_box_backward(d, shared, (double *)dH.p, (double *)dG.p, (double *)dx.p, (double *)dl.p,
                                    (uint32_t *)da.p, (uint32_t *)dw.p, (int32_t *)ds.p, (double *)dg.p,
                                    (double *)dgl.p, (double *)oH.p, (double *)of.p, (double *)oG.p, (double *)obl.p,
                                    (double *)obu.p, (double *)olb.p, (double *)oub.p, nullptr);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize(), "qpb_solve_range_box_backward_host kernel");
  HIPCHK(down(gH, oH, BH * n * n * 8), "gH D2H");
  HIPCHK(down(gf, of, B * n * 8), "gf D2H");
  HIPCHK(down(mg ? gG : nullptr, oG, BG * mg * n * 8), "gG D2H");
  HIPCHK(down(gbl, obl, B * mg * 8), "gbl D2H");
  HIPCHK(down(gbu, obu, B * mg * 8), "gbu D2H");
  HIPCHK(down(glb, olb, B * n * 8), "glb D2H");
  HIPCHK(down(gub, oub, B * n * 8), "gub D2H");
  return 0;
}

// ---- two-sided rows on a factor buffer ------------------------------------------
// qpb_solve_range_factored's argument rules after check_desc, up to batch == 0
static int check_range_factored(const qpb_desc *d, int32_t meq) {
  if (meq < 0) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_range_factored: meq < 0");
  if (d->flags != 0) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_range_factored: flags must be 0 (got %d)", d->flags);
  if (qpb::route_factored(d->n, d->m).step == 0)
    return fail(QPB_ERR_UNSUPPORTED,
                "qpb_solve_range_factored: n=%d m=%d outside the factored kernels with range rows (n<=%d, m<=%d)", d->n,
                d->m, qpb::kFactoredMaxN, qpb::kFactoredMaxM);
  if (meq > d->m) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_range_factored: meq=%d > m=%d", meq, d->m);
  return 0;
}
// ... and the pointers (m > 0; device or host)
static int check_range_factored_arrays(const double *fac, const double *f, const double *bl, const double *bu,
                                       const double *x, const double *lam, const uint32_t *active,
                                       const int32_t *status) {
  if (!fac || !f || !x || !status)
    return fail(QPB_ERR_INVALID_ARG, "qpb_solve_range_factored: fac, f, x and status are required");
  if (!lam || !active || (!bl && !bu))
    return fail(QPB_ERR_INVALID_ARG,
                "qpb_solve_range_factored: lam, active and at least one of bl and bu are required when m > 0");
  return 0;
}

extern "C" int qpb_solve_range_factored(const qpb_desc *d, int32_t meq, const double *fac, const double *f,
                                        const double *bl, const double *bu, double *x, double *lam, uint32_t *active,
                                        uint32_t *lower, int32_t *status, int32_t *iters, void *stream) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_range_factored(d, meq);
  if (rc) return rc;
  // no rows: the call is qpb_solve_factored, launch for launch (the same rules from here on)
  if (d->m == 0) return qpb_solve_factored(d, 0, fac, f, nullptr, x, lam, active, status, iters, stream);
  if (d->batch == 0) return 0;
  rc = check_range_factored_arrays(fac, f, bl, bu, x, lam, active, status);
  if (rc) return rc;
  if ((uintptr_t)fac & 15) return fail(QPB_ERR_INVALID_ARG, "qpb_solve_range_factored: fac must be 16-byte aligned");
  rc = check_device();
  if (rc) return rc;
  const qpb::Route r = qpb::route_factored(d->n, d->m);
  qpb_gi_range_factored_launcher *const fn =
      r.kernel == qpb::Kernel::gi_dense ? qpb_launch_gi_range_factored : qpb_launch_gi_wave_range_factored;
  const long long n = d->n, m = d->m;
  // the chunk walk of the factored form: the buffer's QP stride is 0
  return qpb::for_each_chunk(
      d->batch, r.step,
      [&](long long count, const double *Fc, const double *fc, const double *blc, const double *buc, double *xc,
          double *lc, uint32_t *ac, uint32_t *wc, int32_t *sc, int32_t *ic) {
        qpb_desc c = *d;
        c.batch = count;
        const hipError_t e = fn(&c, meq, Fc, fc, blc, buc, xc, lc, ac, wc, sc, ic, (hipStream_t)stream);
        return e == hipSuccess ? 0 : hip_fail(e, "qpb_solve_range_factored launch");
      },
      qpb::required(fac, 0), qpb::required(f, n), qpb::optional(bl, m), qpb::optional(bu, m), qpb::required(x, n),
      qpb::required(lam, m), qpb::required(active, (m + 31) / 32), qpb::optional(lower, (m + 31) / 32),
      qpb::required(status, 1), qpb::optional(iters, 1));
}

extern "C" int qpb_solve_range_factored_host(const qpb_desc *d, int32_t meq, const double *fac, const double *f,
                                             const double *bl, const double *bu, double *x, double *lam,
                                             uint32_t *active, uint32_t *lower, int32_t *status, int32_t *iters) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_range_factored(d, meq);
  if (rc) return rc;
  if (d->m == 0) return qpb_solve_factored_host(d, 0, fac, f, nullptr, x, lam, active, status, iters);
  if (d->batch == 0) return 0;
  rc = check_range_factored_arrays(fac, f, bl, bu, x, lam, active, status);  // host pointers: the same rules
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  const size_t B = (size_t)d->batch, n = d->n, m = d->m, w = (m + 31) / 32;
  DevBuf dF, df, dbl, dbu, dx, dl, da, dw, ds, di;
  HIPCHK(up(dF, fac, (size_t)qpb::fct::layout(d->n, d->m).size * 8), "fac");
  HIPCHK(up(df, f, B * n * 8), "f");
  HIPCHK(up(dbl, bl, B * m * 8), "bl");
  HIPCHK(up(dbu, bu, B * m * 8), "bu");
  HIPCHK(alloc(dx, x, B * n * 8), "x");
  HIPCHK(alloc(dl, lam, B * m * 8), "lam");
  HIPCHK(alloc(da, active, B * w * 4), "active");
  HIPCHK(alloc(dw, lower, B * w * 4), "lower");
  HIPCHK(alloc(ds, status, B * 4), "status");
  HIPCHK(alloc(di, iters, B * 4), "iters");
  rc = qpb_solve_range_factored(d, meq, (double *)dF.p, (double *)df.p, (double *)dbl.p, (double *)dbu.p,
                                (double *)dx.p, (double *)dl.p, (uint32_t *)da.p, (uint32_t *)dw.p, (int32_t *)ds.p,
                                (int32_t *)di.p, nullptr);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize(), "qpb_solve_range_factored_host kernel");
  HIPCHK(down(x, dx, B * n * 8), "x D2H");
  HIPCHK(down(lam, dl, B * m * 8), "lam D2H");
  HIPCHK(down(active, da, B * w * 4), "active D2H");
  HIPCHK(down(lower, dw, B * w * 4), "lower D2H");
  HIPCHK(down(status, ds, B * 4), "status D2H");
  HIPCHK(down(iters, di, B * 4), "iters D2H");
  return 0;
}

// qpb_solve_backward_host, qpb_solve_shared_backward_host (shared > 0: a
// shared operand and its gradient are one matrix) and qpb_solve_backward_dual_host
// (glam, may be NULL): copy in, run, copy out
static int backward_host(const qpb_desc *d, int32_t shared, const double *H, const double *A, const double *x,
                         const double *lam, const uint32_t *active, const int32_t *status, const double *gx,
                         const double *glam, double *gH, double *gf, double *gA, double *gb);

extern "C" int qpb_solve_backward_host(const qpb_desc *d, const double *H, const double *A, const double *x,
                                       const double *lam, const uint32_t *active, const int32_t *status,
                                       const double *gx, double *gH, double *gf, double *gA, double *gb) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_bwd(d);
  if (rc) return rc;
  return backward_host(d, 0, H, A, x, lam, active, status, gx, nullptr, gH, gf, gA, gb);
}

extern "C" int qpb_solve_shared_backward_host(const qpb_desc *d, int32_t shared, const double *H, const double *A,
                                              const double *x, const double *lam, const uint32_t *active,
                                              const int32_t *status, const double *gx, double *gH, double *gf,
                                              double *gA, double *gb) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_shared_bwd(d, shared);
  if (rc) return rc;
  shared = shared_of(d, shared);
  if (shared == 0) return qpb_solve_backward_host(d, H, A, x, lam, active, status, gx, gH, gf, gA, gb);
  return backward_host(d, shared, H, A, x, lam, active, status, gx, nullptr, gH, gf, gA, gb);
}

extern "C" int qpb_solve_backward_dual_host(const qpb_desc *d, int32_t shared, const double *H, const double *A,
                                            const double *x, const double *lam, const uint32_t *active,
                                            const int32_t *status, const double *gx, const double *glam, double *gH,
                                            double *gf, double *gA, double *gb) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_bwd_dual(d, shared);
  if (rc) return rc;
  if (!glam || d->m == 0) return qpb_solve_shared_backward_host(d, shared, H, A, x, lam, active, status, gx, gH, gf, gA, gb);
  return backward_host(d, shared, H, A, x, lam, active, status, gx, glam, gH, gf, gA, gb);
}

static int backward_host(const qpb_desc *d, int32_t shared, const double *H, const double *A, const double *x,
                         const double *lam, const uint32_t *active, const int32_t *status, const double *gx,
                         const double *glam, double *gH, double *gf, double *gA, double *gb) {
  int rc;
  if (d->batch == 0) return 0;
  rc = check_bwd_arrays(d, H, A, x, lam, active, gx, gH, gf, gA, gb);  // host pointers: the same rules
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  const size_t B = (size_t)d->batch, n = d->n, m = d->m, w = (m + 31) / 32;
  DevBuf dH, dA, dx, dl, da, ds, dg, dgl, oH, of, oA, ob;
  const size_t BH = (shared & QPB_SHARED_H) ? 1 : B, BA = (shared & QPB_SHARED_A) ? 1 : B;
  HIPCHK(up(dH, H, BH * n * n * 8), "H");
  HIPCHK(up(dA, m ? A : nullptr, BA * m * n * 8), "A");
  HIPCHK(up(dx, x, B * n * 8), "x");
  HIPCHK(up(dl, m ? lam : nullptr, B * m * 8), "lam");
  HIPCHK(up(da, m ? active : nullptr, B * w * 4), "active");
  HIPCHK(up(ds, status, B * 4), "status");
  HIPCHK(up(dg, gx, B * n * 8), "gx");
  HIPCHK(up(dgl, m ? glam : nullptr, B * m * 8), "glam");
  HIPCHK(alloc(oH, gH, BH * n * n * 8), "gH");
  HIPCHK(alloc(of, gf, B * n * 8), "gf");
  HIPCHK(alloc(oA, m ? gA : nullptr, BA * m * n * 8), "gA");
  HIPCHK(alloc(ob, m ? gb : nullptr, B * m * 8), "gb");
  rc = qpb_solve_backward_dual(d, shared, (double *)dH.p, (double *)dA.p, (double *)dx.p, (double *)dl.p,
                               (uint32_t *)da.p, (int32_t *)ds.p, (double *)dg.p, (double *)dgl.p, (double *)oH.p,
                               (double *)of.p, (double *)oA.p, (double *)ob.p, nullptr);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize(), "qpb_solve_backward_host kernel");
  HIPCHK(down(gH, oH, BH * n * n * 8), "gH D2H");
  HIPCHK(down(gf, of, B * n * 8), "gf D2H");
  HIPCHK(down(m ? gA : nullptr, oA, BA * m * n * 8), "gA D2H");
  HIPCHK(down(m ? gb : nullptr, ob, B * m * 8), "gb D2H");
  return 0;
}

extern "C" int qpb_solve_box_backward_host(const qpb_desc *d, const double *H, const double *x,
                                           const uint32_t *active, const int32_t *status, const double *gx, double *gH,
                                           double *gf, double *glb, double *gub) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_bwd_box(d);
  if (rc) return rc;
  if (d->batch == 0) return 0;
  rc = check_bwd_box_arrays(H, x, active, gx, gH, gf, glb, gub);  // host pointers: the same rules
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  const size_t B = (size_t)d->batch, n = d->n, w = (2 * n + 31) / 32;
  DevBuf dH, dx, da, ds, dg, oH, of, ol, ou;
  HIPCHK(up(dH, H, B * n * n * 8), "H");
  HIPCHK(up(dx, x, B * n * 8), "x");
  HIPCHK(up(da, active, B * w * 4), "active");
  HIPCHK(up(ds, status, B * 4), "status");
  HIPCHK(up(dg, gx, B * n * 8), "gx");
  HIPCHK(alloc(oH, gH, B * n * n * 8), "gH");
  HIPCHK(alloc(of, gf, B * n * 8), "gf");
  HIPCHK(alloc(ol, glb, B * n * 8), "glb");
  HIPCHK(alloc(ou, gub, B * n * 8), "gub");
  rc = qpb_solve_box_backward(d, (double *)dH.p, (double *)dx.p, (uint32_t *)da.p, (int32_t *)ds.p, (double *)dg.p,
                              (double *)oH.p, (double *)of.p, (double *)ol.p, (double *)ou.p, nullptr);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize(), "qpb_solve_box_backward_host kernel");
  HIPCHK(down(gH, oH, B * n * n * 8), "gH D2H");
  HIPCHK(down(gf, of, B * n * 8), "gf D2H");
  HIPCHK(down(glb, ol, B * n * 8), "glb D2H");
  HIPCHK(down(gub, ou, B * n * 8), "gub D2H");
  return 0;
}

extern "C" int qpb_solve_box_backward_dual_host(const qpb_desc *d, int32_t shared, const double *H, const double *x,
                                                const uint32_t *active, const int32_t *status, const double *gx,
                                                const double *glam, double *gH, double *gf, double *glb,
                                                double *gub) {
  static const char what[] = "qpb_solve_box_backward_dual";
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_bwd_box_dual(d, shared);
  if (rc) return rc;
  if (d->batch == 0) return 0;
  rc = check_bwd_box_arrays(H, x, active, gx, gH, gf, glb, gub, what);  // host pointers: the same rules
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  const size_t B = (size_t)d->batch, n = d->n, w = (2 * n + 31) / 32, BH = shared ? 1 : B;
  DevBuf dH, dx, da, ds, dg, dgl, oH, of, ol, ou;
  HIPCHK(up(dH, H, BH * n * n * 8), "H");
  HIPCHK(up(dx, x, B * n * 8), "x");
  HIPCHK(up(da, active, B * w * 4), "active");
  HIPCHK(up(ds, status, B * 4), "status");
  HIPCHK(up(dg, gx, B * n * 8), "gx");
  HIPCHK(up(dgl, glam, B * 2 * n * 8), "glam");
  HIPCHK(alloc(oH, gH, BH * n * n * 8), "gH");
  HIPCHK(alloc(of, gf, B * n * 8), "gf");
  HIPCHK(alloc(ol, glb, B * n * 8), "glb");
  HIPCHK(alloc(ou, gub, B * n * 8), "gub");
  rc = qpb_solve_box_backward_dual(d, shared, (double *)dH.p, (double *)dx.p, (uint32_t *)da.p, (int32_t *)ds.p,
                                   (double *)dg.p, (double *)dgl.p, (double *)oH.p, (double *)of.p, (double *)ol.p,
                                   (double *)ou.p, nullptr);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize(), "qpb_solve_box_backward_dual_host kernel");
  HIPCHK(down(gH, oH, BH * n * n * 8), "gH D2H");
  HIPCHK(down(gf, of, B * n * 8), "gf D2H");
  HIPCHK(down(glb, ol, B * n * 8), "glb D2H");
  HIPCHK(down(gub, ou, B * n * 8), "gub D2H");
  return 0;
}

extern "C" int qpb_solve_box_shared_host(const qpb_desc *d, const double *H, const double *f, const double *lb,
                                         const double *ub, double *x, double *lam, uint32_t *active,
                                         int32_t *status, int32_t *iters) {
  bool empty = false;
  int rc = check_box_shared(d, H, f, x, lam, active, status, &empty);  // host pointers: the same rules
  if (rc || empty) return rc;
  const size_t B = (size_t)d->batch, n = d->n, m = d->m, w = (m + 31) / 32;
  DevBuf dH, df, dlb, dub, dx, dl, da, ds, di;
  HIPCHK(up(dH, H, n * n * 8), "H");
  HIPCHK(up(df, f, B * n * 8), "f");
  HIPCHK(up(dlb, lb, B * n * 8), "lb");
  HIPCHK(up(dub, ub, B * n * 8), "ub");
  HIPCHK(alloc(dx, x, B * n * 8), "x");
  HIPCHK(alloc(dl, lam, B * m * 8), "lam");
  HIPCHK(alloc(da, active, B * w * 4), "active");
  HIPCHK(alloc(ds, status, B * 4), "status");
  HIPCHK(alloc(di, iters, B * 4), "iters");
  rc = qpb_solve_box_shared(d, (double *)dH.p, (double *)df.p, (double *)dlb.p, (double *)dub.p, (double *)dx.p,
                            (double *)dl.p, (uint32_t *)da.p, (int32_t *)ds.p, (int32_t *)di.p, nullptr);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize(), "qpb_solve_box_shared_host kernel");
  HIPCHK(down(x, dx, B * n * 8), "x D2H");
  HIPCHK(down(lam, dl, B * m * 8), "lam D2H");
  HIPCHK(down(active, da, B * w * 4), "active D2H");
  HIPCHK(down(status, ds, B * 4), "status D2H");
  HIPCHK(down(iters, di, B * 4), "iters D2H");
  return 0;
}

extern "C" int qpb_factor_box_host(int32_t n, const double *H, double *bxfac, int32_t *fstatus) {
  int rc = check_factor_box(n, H, bxfac);  // host pointers: the same rules (no alignment: the call's own buffer is loaded)
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  const size_t N = n, doubles = (size_t)qpb::bxfct::layout(n).size;
  DevBuf dH, dF, dS;
  HIPCHK(up(dH, H, N * N * 8), "H");
  HIPCHK(alloc(dF, bxfac, doubles * 8), "bxfac");
  HIPCHK(alloc(dS, fstatus, 4), "fstatus");
  rc = qpb_factor_box(n, (double *)dH.p, (double *)dF.p, (int32_t *)dS.p, nullptr);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize(), "qpb_factor_box_host kernel");
  HIPCHK(down(bxfac, dF, doubles * 8), "bxfac D2H");
  HIPCHK(down(fstatus, dS, 4), "fstatus D2H");
  return 0;
}

extern "C" int qpb_solve_box_factored_host(const qpb_desc *d, const double *bxfac, const double *f, const double *lb,
                                           const double *ub, double *x, double *lam, uint32_t *active,
                                           int32_t *status, int32_t *iters) {
  bool empty = false;
  int rc = check_box_factored(d, bxfac, f, x, lam, active, status, &empty);  // host pointers: the same rules
  if (rc || empty) return rc;
  rc = check_device();
  if (rc) return rc;
  const size_t B = (size_t)d->batch, n = d->n, m = d->m, w = (m + 31) / 32;
  DevBuf dF, df, dlb, dub, dx, dl, da, ds, di;
  HIPCHK(up(dF, bxfac, (size_t)qpb::bxfct::layout(d->n).size * 8), "bxfac");
  HIPCHK(up(df, f, B * n * 8), "f");
  HIPCHK(up(dlb, lb, B * n * 8), "lb");
  HIPCHK(up(dub, ub, B * n * 8), "ub");
  HIPCHK(alloc(dx, x, B * n * 8), "x");
  HIPCHK(alloc(dl, lam, B * m * 8), "lam");
  HIPCHK(alloc(da, active, B * w * 4), "active");
  HIPCHK(alloc(ds, status, B * 4), "status");
  HIPCHK(alloc(di, iters, B * 4), "iters");
  rc = qpb_solve_box_factored(d, (double *)dF.p, (double *)df.p, (double *)dlb.p, (double *)dub.p, (double *)dx.p,
                              (double *)dl.p, (uint32_t *)da.p, (int32_t *)ds.p, (int32_t *)di.p, nullptr);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize(), "qpb_solve_box_factored_host kernel");
  HIPCHK(down(x, dx, B * n * 8), "x D2H");
  HIPCHK(down(lam, dl, B * m * 8), "lam D2H");
  HIPCHK(down(active, da, B * w * 4), "active D2H");
  HIPCHK(down(status, ds, B * 4), "status D2H");
  HIPCHK(down(iters, di, B * 4), "iters D2H");
  return 0;
}

extern "C" int qpb_solve_box_shared_backward_host(const qpb_desc *d, const double *H, const double *x,
                                                  const uint32_t *active, const int32_t *status, const double *gx,
                                                  double *gH, double *gf, double *glb, double *gub) {
  static const char what[] = "qpb_solve_box_shared_backward";
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_bwd_box(d, what);
  if (rc) return rc;
  if (d->batch == 0) return 0;
  rc = check_bwd_box_arrays(H, x, active, gx, gH, gf, glb, gub, what);  // host pointers: the same rules
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  const size_t B = (size_t)d->batch, n = d->n, w = (2 * n + 31) / 32;
  DevBuf dH, dx, da, ds, dg, oH, of, ol, ou;
  HIPCHK(up(dH, H, n * n * 8), "H");
  HIPCHK(up(dx, x, B * n * 8), "x");
  HIPCHK(up(da, active, B * w * 4), "active");
  HIPCHK(up(ds, status, B * 4), "status");
  HIPCHK(up(dg, gx, B * n * 8), "gx");
  HIPCHK(alloc(oH, gH, n * n * 8), "gH");
  HIPCHK(alloc(of, gf, B * n * 8), "gf");
  HIPCHK(alloc(ol, glb, B * n * 8), "glb");
  HIPCHK(alloc(ou, gub, B * n * 8), "gub");
  rc = qpb_solve_box_shared_backward(d, (double *)dH.p, (double *)dx.p, (uint32_t *)da.p, (int32_t *)ds.p,
                                     (double *)dg.p, (double *)oH.p, (double *)of.p, (double *)ol.p, (double *)ou.p,
                                     nullptr);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize(), "qpb_solve_box_shared_backward_host kernel");
  HIPCHK(down(gH, oH, n * n * 8), "gH D2H");
  HIPCHK(down(gf, of, B * n * 8), "gf D2H");
  HIPCHK(down(glb, ol, B * n * 8), "glb D2H");
  HIPCHK(down(gub, ou, B * n * 8), "gub D2H");
  return 0;
}

static int check_ref(const qpb_ref_desc *d) {
  if (!d) return fail(QPB_ERR_INVALID_ARG, "desc is NULL");
  if (d->batch < 0 || d->n < 1 || d->iterations < 0) return fail(QPB_ERR_INVALID_ARG, "bad n/batch/iterations");
  if (d->mode != QPB_REF_NEWTON && d->mode != QPB_REF_ADMM && d->mode != QPB_REF_GD)
    return fail(QPB_ERR_INVALID_ARG, "unknown ref mode %d", d->mode);
  if (d->n > QPB_REF_MAX_N) return fail(QPB_ERR_UNSUPPORTED, "qpb_ref_solve: n=%d > %d", d->n, QPB_REF_MAX_N);
  return 0;
}

extern "C" int qpb_ref_solve(const qpb_ref_desc *d, const double *P, const double *q, const double *x0,
                             double *x, int32_t *iters, void *stream) {
  int rc = check_ref(d);
  if (rc) return rc;
  if (d->batch == 0) return 0;
  if (!P || !q || !x || (!x0 && d->mode != QPB_REF_ADMM)) return fail(QPB_ERR_INVALID_ARG, "P, q, x0, x required");
  rc = check_device();
  if (rc) return rc;
  // n <= 64: one 64-thread workgroup per QP, at most 2^25 QPs per launch
  // (n > 64: a grid of one workgroup per CU walks the batch)
  const long long n = d->n;
  return qpb::for_each_chunk(
      d->batch, 1LL << 25,
      [&](long long count, const double *Pc, const double *qc, const double *x0c, double *xc, int32_t *ic) {
        qpb_ref_desc c = *d;
        c.batch = count;
        const hipError_t e = qpb_launch_ref(&c, Pc, qc, x0c, xc, ic, (hipStream_t)stream);
        return e == hipSuccess ? 0 : hip_fail(e, "qpb_ref_solve launch");
      },
      qpb::required(P, n * n), qpb::required(q, n), qpb::optional(x0, n), qpb::required(x, n),
      qpb::optional(iters, 1));
}

extern "C" int qpb_ref_solve_host(const qpb_ref_desc *d, const double *P, const double *q, const double *x0,
                                  double *x, int32_t *iters) {
  int rc = check_ref(d);
  if (rc) return rc;
  if (d->batch == 0) return 0;
  rc = check_device();
  if (rc) return rc;
  const size_t B = (size_t)d->batch, n = d->n;
  DevBuf dP, dq, dx0, dx, di;
  HIPCHK(up(dP, P, B * n * n * 8), "P");
  HIPCHK(up(dq, q, B * n * 8), "q");
  HIPCHK(up(dx0, x0, B * n * 8), "x0");
  HIPCHK(alloc(dx, x, B * n * 8), "x");
  HIPCHK(alloc(di, iters, B * 4), "iters");
  rc = qpb_ref_solve(d, (double *)dP.p, (double *)dq.p, (double *)dx0.p, (double *)dx.p, (int32_t *)di.p,
                     nullptr);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize(), "qpb_ref_solve_host kernel");
  HIPCHK(down(x, dx, B * n * 8), "x D2H");
  HIPCHK(down(iters, di, B * 4), "iters D2H");
  return 0;
}

extern "C" int qpb_matrix_invert(int32_t n, int64_t batch, const double *P, double *Pinv, void *stream) {
  if (n < 1 || batch < 0) return fail(QPB_ERR_INVALID_ARG, "bad qpb_matrix_invert arguments");
  if (n > QPB_REF_MAX_N) return fail(QPB_ERR_UNSUPPORTED, "qpb_matrix_invert: n=%d > %d", n, QPB_REF_MAX_N);
  if (batch == 0) return 0;
  if (!P || !Pinv) return fail(QPB_ERR_INVALID_ARG, "P and Pinv are required");
  int rc = check_device();
  if (rc) return rc;
  const long long nn = (long long)n * n;
  return qpb::for_each_chunk(
      batch, 1LL << 25,  // one 64-thread workgroup per matrix
      [&](long long count, const double *Pc, double *Ic) {
        const hipError_t e = qpb_launch_ref_invert(n, count, Pc, Ic, (hipStream_t)stream);
        return e == hipSuccess ? 0 : hip_fail(e, "qpb_matrix_invert launch");
      },
      qpb::required(P, nn), qpb::required(Pinv, nn));
}

extern "C" int qpb_qf_eval(int32_t n, int64_t batch, const double *P, const double *q, double r, const double *x,
                           double *out, void *stream) {
  if (n < 1 || batch < 0 || !P || !q || !x || !out) return fail(QPB_ERR_INVALID_ARG, "bad qpb_qf_eval arguments");
  if (batch == 0) return 0;
  int rc = check_device();
  if (rc) return rc;
  hipError_t e = qpb_launch_qf_eval(n, batch, P, q, r, x, out, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "qpb_qf_eval launch");
  return 0;
}

extern "C" int qpb_ref_generate(const qpb_ref_gen_desc *d, double *P, double *q, double *x0, void *stream) {
  if (!d) return fail(QPB_ERR_INVALID_ARG, "desc is NULL");
  if (d->n < 1 || d->batch < 0) return fail(QPB_ERR_INVALID_ARG, "n must be >= 1 and batch >= 0");
  if (d->n > QPB_MAX_N) return fail(QPB_ERR_UNSUPPORTED, "qpb_ref_generate: n=%d > %d", d->n, QPB_MAX_N);
  if (d->batch > (1LL << 25))  // one 64-thread workgroup per QP: 2^32 work-items per launch
    return fail(QPB_ERR_UNSUPPORTED, "batch > 2^25 QPs per generator call (split it with `first`)");
  if (d->batch > 0 && (!P || !q || !x0)) return fail(QPB_ERR_INVALID_ARG, "NULL output pointer");
  int rc = check_device();
  if (rc) return rc;
  const double range[6] = {d->p_min, d->p_max, d->q_min, d->q_max, d->x_min, d->x_max};
  hipError_t e = qpb_launch_ref_generate(d->n, d->batch, d->first, d->seed, range, P, q, x0, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "qpb_ref_generate launch");
  return 0;
}

extern "C" int qpb_generate(const qpb_gen_desc *d, double *H, double *f, double *A, double *b, void *stream) {
  if (!d) return fail(QPB_ERR_INVALID_ARG, "desc is NULL");
  if (d->n < 1 || d->m < 1 || d->batch < 0) return fail(QPB_ERR_INVALID_ARG, "n, m must be >= 1 and batch >= 0");
  if (d->family != QPB_FAMILY_BOX && d->family != QPB_FAMILY_DENSE)
    return fail(QPB_ERR_INVALID_ARG, "unknown family %d", d->family);
  if (d->family == QPB_FAMILY_BOX && d->m != 2 * d->n)
    return fail(QPB_ERR_INVALID_ARG, "the box family has m = 2n (got n=%d m=%d)", d->n, d->m);
  if (d->n > 128) return fail(QPB_ERR_UNSUPPORTED, "qpb_generate: n=%d > 128", d->n);
  if (d->n > 16 && d->m < d->n) return fail(QPB_ERR_UNSUPPORTED, "qpb_generate: n > 16 needs m >= n");
  if (d->batch > (1LL << 25))  // one 64-thread workgroup per QP: 2^32 work-items per launch
    return fail(QPB_ERR_UNSUPPORTED, "batch > 2^25 QPs per generator call (split it with `first`)");
  if (d->batch > 0 && (!H || !f || !A || !b)) return fail(QPB_ERR_INVALID_ARG, "NULL output pointer");
  int rc = check_device();
  if (rc) return rc;
  hipError_t e = qpb_launch_generate(d->n, d->m, d->batch, d->first, d->seed, d->family, d->shift, d->box, H, f, A,
                                     b, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail(e, "qpb_generate launch");
  return 0;
}

// ---- T right-hand sides per QP in one launch ----------------------------------
static_assert(QPB_MAX_RHS == qpb::kMaxRhs && (QPB_SHARED_RHS & (QPB_SHARED_H | QPB_SHARED_A)) == 0);

// qpb_solve_factored_backward_multi's argument rules after check_desc, up to batch == 0
static int check_factored_bwd_multi(const qpb_desc *d, int32_t nrhs, int32_t shared) {
  static const char what[] = "qpb_solve_factored_backward_multi";
  if (d->flags != 0) return fail(QPB_ERR_INVALID_ARG, "%s: flags must be 0 (got %d)", what, d->flags);
  if (shared & ~QPB_SHARED_RHS)
    return fail(QPB_ERR_INVALID_ARG, "%s: shared must be 0 or QPB_SHARED_RHS (got %d)", what, shared);
  if (nrhs < 1 || nrhs > QPB_MAX_RHS)
    return fail(QPB_ERR_INVALID_ARG, "%s: nrhs must be 1..%d (got %d)", what, QPB_MAX_RHS, nrhs);
  if (qpb::route_factored_bwd_multi(d->n, d->m).step == 0)
    return fail(QPB_ERR_UNSUPPORTED, "%s: n=%d m=%d outside the factored backward kernels (n<=%d, m<=%d)", what, d->n,
                d->m, qpb::kBwdMultiMaxN, qpb::kBwdMultiMaxM);
  return 0;
}
// ... and the pointers (device or host)
static int check_factored_bwd_multi_arrays(const qpb_desc *d, const double *bfac, const uint32_t *active,
                                           const double *gx, const double *gf, const double *gb) {
  static const char what[] = "qpb_solve_factored_backward_multi";
  if (!bfac || !gx) return fail(QPB_ERR_INVALID_ARG, "%s: bfac and gx are required", what);
  if (d->m > 0 && !active) return fail(QPB_ERR_INVALID_ARG, "%s: active is required when m > 0", what);
  if (!gf && !(d->m > 0 && gb)) return fail(QPB_ERR_INVALID_ARG, "%s: at least one of gf and gb is required", what);
  return 0;
}

extern "C" int qpb_solve_factored_backward_multi(const qpb_desc *d, const double *bfac, const uint32_t *active,
                                                 const int32_t *status, int32_t nrhs, int32_t shared,
                                                 const double *gx, const double *glam, double *gf, double *gb,
                                                 void *stream) {
  static const char what[] = "qpb_solve_factored_backward_multi";
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_factored_bwd_multi(d, nrhs, shared);
  if (rc) return rc;
  if (d->batch == 0) return 0;
  rc = check_factored_bwd_multi_arrays(d, bfac, active, gx, gf, gb);
  if (rc) return rc;
  if ((uintptr_t)bfac & 15) return fail(QPB_ERR_INVALID_ARG, "%s: bfac must be 16-byte aligned", what);
  rc = check_device();
  if (rc) return rc;
  const qpb::Route r = qpb::route_factored_bwd_multi(d->n, d->m);
  const long long n = d->n, m = d->m, T = nrhs;
  if (m == 0) glam = nullptr, gb = nullptr;  // ignored
  // the right-hand sides' QP stride in directions: 0 for the one shared set, in the kernels and in the chunk walk
  const long long rs = (shared & QPB_SHARED_RHS) ? 0 : T;
  return qpb::for_each_chunk(
      d->batch, r.step,
      [&](long long count, const double *Fc, const uint32_t *ac, const int32_t *sc, const double *gxc,
          const double *glc, double *gfc, double *gbc) {
        qpb_desc c = *d;
        c.batch = count;
        const hipError_t e =
            qpb_launch_kkt_bwd_factored_multi(&c, Fc, ac, sc, nrhs, rs, gxc, glc, gfc, gbc, (hipStream_t)stream);
        return e == hipSuccess ? 0 : fail(QPB_ERR_HIP, "%s launch: %s", what, hipGetErrorString(e));
      },
      qpb::required(bfac, 0), qpb::optional(active, (m + 31) / 32), qpb::optional(status, 1),
      qpb::required(gx, rs * n), qpb::optional(glam, rs * m), qpb::optional(gf, T * n), qpb::optional(gb, T * m));
}

extern "C" int qpb_solve_factored_backward_multi_host(const qpb_desc *d, const double *bfac, const uint32_t *active,
                                                      const int32_t *status, int32_t nrhs, int32_t shared,
                                                      const double *gx, const double *glam, double *gf, double *gb) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_factored_bwd_multi(d, nrhs, shared);
  if (rc) return rc;
  if (d->batch == 0) return 0;
  rc = check_factored_bwd_multi_arrays(d, bfac, active, gx, gf, gb);  // host pointers: the same rules
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  const size_t B = (size_t)d->batch, n = d->n, m = d->m, w = (m + 31) / 32, T = (size_t)nrhs;
  const size_t BR = (shared & QPB_SHARED_RHS) ? 1 : B;
  DevBuf dF, da, ds, dg, dgl, of, ob;
  HIPCHK(up(dF, bfac, (size_t)qpb::bfct::layout(d->n, d->m).size * 8), "bfac");
  HIPCHK(up(da, m ? active : nullptr, B * w * 4), "active");
  HIPCHK(up(ds, status, B * 4), "status");
  HIPCHK(up(dg, gx, BR * T * n * 8), "gx");
  HIPCHK(up(dgl, m ? glam : nullptr, BR * T * m * 8), "glam");
  HIPCHK(alloc(of, gf, B * T * n * 8), "gf");
  HIPCHK(alloc(ob, m ? gb : nullptr, B * T * m * 8), "gb");
  rc = qpb_solve_factored_backward_multi(d, (double *)dF.p, (uint32_t *)da.p, (int32_t *)ds.p, nrhs, shared,
                                         (double *)dg.p, (double *)dgl.p, (double *)of.p, (double *)ob.p, nullptr);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize(), "qpb_solve_factored_backward_multi_host kernel");
  HIPCHK(down(gf, of, B * T * n * 8), "gf D2H");
  HIPCHK(down(m ? gb : nullptr, ob, B * T * m * 8), "gb D2H");
  return 0;
}

// qpb_solve_box_backward_multi's argument rules after check_desc, up to batch == 0
static int check_bwd_box_multi(const qpb_desc *d, int32_t nrhs, int32_t shared) {
  static const char what[] = "qpb_solve_box_backward_multi";
  if (d->m != 2 * d->n) return fail(QPB_ERR_INVALID_ARG, "%s: m must be 2n (got n=%d m=%d)", what, d->n, d->m);
  if (d->flags != 0) return fail(QPB_ERR_INVALID_ARG, "%s: flags must be 0 (got %d)", what, d->flags);
  if (shared & ~(QPB_SHARED_H | QPB_SHARED_RHS))
    return fail(QPB_ERR_INVALID_ARG, "%s: shared must be a combination of QPB_SHARED_H and QPB_SHARED_RHS (got %d)",
                what, shared);
  if (nrhs < 1 || nrhs > QPB_MAX_RHS)
    return fail(QPB_ERR_INVALID_ARG, "%s: nrhs must be 1..%d (got %d)", what, QPB_MAX_RHS, nrhs);
  if (qpb::route_bwd_box_multi(d->n).step == 0)
    return fail(QPB_ERR_UNSUPPORTED, "%s: n=%d outside the backward box kernels (n<=%d)", what, d->n,
                qpb::kBwdBoxMultiMaxN);
  return 0;
}
// ... and the pointers (device or host)
static int check_bwd_box_multi_arrays(const double *H, const uint32_t *active, const double *gx, const double *gf,
                                      const double *glb, const double *gub) {
  static const char what[] = "qpb_solve_box_backward_multi";
  if (!H || !active || !gx) return fail(QPB_ERR_INVALID_ARG, "%s: H, active and gx are required", what);
  if (!gf && !glb && !gub) return fail(QPB_ERR_INVALID_ARG, "%s: at least one of gf, glb and gub is required", what);
  return 0;
}

extern "C" int qpb_solve_box_backward_multi(const qpb_desc *d, int32_t shared, const double *H,
                                            const uint32_t *active, const int32_t *status, int32_t nrhs,
                                            const double *gx, const double *glam, double *gf, double *glb,
                                            double *gub, void *stream) {
  static const char what[] = "qpb_solve_box_backward_multi";
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_bwd_box_multi(d, nrhs, shared);
  if (rc) return rc;
  if (d->batch == 0) return 0;
  rc = check_bwd_box_multi_arrays(H, active, gx, gf, glb, gub);
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  const qpb::Route r = qpb::route_bwd_box_multi(d->n);
  const long long n = d->n, m = d->m, T = nrhs;
  // a shared operand's QP stride is 0, in the kernels and in the chunk walk
  const long long sH = (shared & QPB_SHARED_H) ? 0 : n * n, rs = (shared & QPB_SHARED_RHS) ? 0 : T;
  return qpb::for_each_chunk(
      d->batch, r.step,
      [&](long long count, const double *Hc, const uint32_t *ac, const int32_t *sc, const double *gxc,
          const double *gmc, double *gfc, double *glc, double *guc) {
        qpb_desc c = *d;
        c.batch = count;
        const hipError_t e =
            qpb_launch_kkt_bwd_box_multi(&c, sH, Hc, ac, sc, nrhs, rs, gxc, gmc, gfc, glc, guc, (hipStream_t)stream);
        return e == hipSuccess ? 0 : fail(QPB_ERR_HIP, "%s launch: %s", what, hipGetErrorString(e));
      },
      qpb::required(H, sH), qpb::required(active, (m + 31) / 32), qpb::optional(status, 1), qpb::required(gx, rs * n),
      qpb::optional(glam, rs * m), qpb::optional(gf, T * n), qpb::optional(glb, T * n), qpb::optional(gub, T * n));
}

extern "C" int qpb_solve_box_backward_multi_host(const qpb_desc *d, int32_t shared, const double *H,
                                                 const uint32_t *active, const int32_t *status, int32_t nrhs,
                                                 const double *gx, const double *glam, double *gf, double *glb,
                                                 double *gub) {
  int rc = check_desc(d);
  if (rc) return rc;
  rc = check_bwd_box_multi(d, nrhs, shared);
  if (rc) return rc;
  if (d->batch == 0) return 0;
  rc = check_bwd_box_multi_arrays(H, active, gx, gf, glb, gub);  // host pointers: the same rules
  if (rc) return rc;
  rc = check_device();
  if (rc) return rc;
  const size_t B = (size_t)d->batch, n = d->n, w = (2 * n + 31) / 32, T = (size_t)nrhs;
  const size_t BH = (shared & QPB_SHARED_H) ? 1 : B, BR = (shared & QPB_SHARED_RHS) ? 1 : B;
  DevBuf dH, da, ds, dg, dgl, of, ol, ou;
  HIPCHK(up(dH, H, BH * n * n * 8), "H");
  HIPCHK(up(da, active, B * w * 4), "active");
  HIPCHK(up(ds, status, B * 4), "status");
  HIPCHK(up(dg, gx, BR * T * n * 8), "gx");
  HIPCHK(up(dgl, glam, BR * T * 2 * n * 8), "glam");
  HIPCHK(alloc(of, gf, B * T * n * 8), "gf");
  HIPCHK(alloc(ol, glb, B * T * n * 8), "glb");
  HIPCHK(alloc(ou, gub, B * T * n * 8), "gub");
  rc = qpb_solve_box_backward_multi(d, shared, (double *)dH.p, (uint32_t *)da.p, (int32_t *)ds.p, nrhs, (double *)dg.p,
                                    (double *)dgl.p, (double *)of.p, (double *)ol.p, (double *)ou.p, nullptr);
  if (rc) return rc;
  HIPCHK(hipDeviceSynchronize(), "qpb_solve_box_backward_multi_host kernel");
  HIPCHK(down(gf, of, B * T * n * 8), "gf D2H");
  HIPCHK(down(glb, ol, B * T * n * 8), "glb D2H");
  HIPCHK(down(gub, ou, B * T * n * 8), "gub D2H");
  return 0;
}

extern "C" int qpb_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}

extern "C" int qpb_set_device(int device) {
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
  return 0;
}

extern "C" int qpb_synchronize(void *stream) {
  hipError_t e = stream ? hipStreamSynchronize((hipStream_t)stream) : hipDeviceSynchronize();
  if (e != hipSuccess) return hip_fail(e, "synchronize");
  return 0;
}

extern "C" const char *qpb_last_error(void) { return g_err; }

// the hot kernel revision is part of the string: profiles/pmc_traffic.json is
// only trusted for the revision it was measured on (bench.py)
extern "C" const char *qpb_version(void) { return "qpb 0.14 (gfx950; gi_dense v11.7: a scalar base per group of four QPs and 32-bit lane offsets for every load and store (outputs bit for bit those of gi_dense v11.6), DROP argmin taken in the DROP, back-substitution tests grouped 15..8 / 7..4 / 3..1, x gather as one DPP-fused 32-bit add per row, dual steepest-edge select -s/|D[r,q:]| with a nonzero key floor, dependency scale clamped to FLT_MAX, setup slacks from the sweep's DPP-read f, output stores under the A-row loads, DPP-fused slack product and Householder update, Householder product as u + alpha D[:,q], exact ratio step, one-trip loads and x gather, 3 waves/SIMD and 12 per CU (12,608 B of LDS per wave: the exchange row in R's column 0, Givens parameters in registers), built without machine LICM; gi_box v2.2: lb <= x <= ub, A implicit, dual steepest-edge select with a nonzero key floor, DPP-fused slack and Householder products, one-pass R column shift, 12 waves per CU; gi_wave v6.7 (+ BOX, n <= 32; absent bounds as +inf slacks): x solves with the components captured in LDS (no lane masks, no SGPR spills), dual steepest-edge select with a nonzero key floor, ratio reduction only when a partial step is possible, active A rows for x gathered 16 at a time, DPP-fused sweep, slack product, Householder update and back substitution (no LDS vector reads), Householder product as u + alpha D[:,q], odd-stride R with the exchange row in its column 0 (12 waves per CU), one-trip A gather for x, split setup sweep, 3 waves/SIMD; gi_gram v4.5 (+ BOX, n <= 128: qpb_solve_box with A generated in place) n<=128 on fp64 MFMA, no next-QP prefetch, lane ids opaque per iteration (2 VGPR spills instead of 29), active set as Q1 rows and Z = R^{-1} (parallel passes only), |u|^2 published with the key, broadcast row products, conflict-free diagonal-tile inverses, one-trip loads, cached workspace launched under its lock; ref v6: n <= 1024 (above 128: 1024-thread workgroups, the matrices in a global workspace slice), 64 < n <= 128 one LDS matrix per workgroup (LU, W / V, P in turn), LU rows staged for the solves, branch-free chunked sums; gi_eq v1.0: qpb_solve_eq for n <= 32 and m <= 64, equality rows 0 .. meq-1 in the EQ forms of gi_dense and gi_wave, taken first and never dropped, sign chosen at selection, free multipliers, consistent dependent rows left out; kkt_bwd v1.1: qpb_solve_backward for n <= 32 and m <= 64, gradients of a solve through its KKT system at fixed active set, H factored and the active rows of A L^-T orthogonalised in row order (two Gram-Schmidt passes, and two projections of L^-1 g: A_W dx = 0 holds at cond(H) = 1e10 with |W| = n), four QPs per wavefront for n <= 16 and m <= 32, one per wavefront above; kkt_bwd_box v1.0: qpb_solve_box_backward for n <= 32, gradients of a box solve for H, f, lb and ub at fixed active set, one Cholesky of H with the fixed variables' rows and columns replaced by the identity (no gather, no A, no lam), r = gx + H dx on the active bounds, four QPs per wavefront for n <= 16, one per wavefront above; gi_shared v1.0: qpb_solve_shared for n <= 32 and m <= 64, one H and / or one A for the whole batch read from one copy through run-time QP strides in the SH forms of gi_dense and gi_wave, plain and EQ, outputs bit for bit those of qpb_solve_eq on copies; kkt_bwd_sum v1.0: qpb_solve_shared_backward, the gradient of a shared H or A summed over the batch on the fp64 matrix cores, four QPs per MFMA step, one wave per slice of a plan that depends on the batch size alone, slots added in order by a finish kernel, no atomics; gi_range v1.0: qpb_solve_range for n <= 32 and m <= 64, two-sided rows bl <= A x <= bu in the RG forms of gi_dense and gi_wave (on their EQ and SH forms: equality rows and a shared H or A at run time), one row of D and an orientation bit per row, the row negated in place when its other side is selected, the side kept with the active position through a DROP, signed multipliers in OSQP's convention and a `lower` bit set beside `active`; gi_fact v1.0: qpb_factor_shared and qpb_solve_factored for n <= 32 and m <= 64, one shared H and A factored once by the class's own load and sweep into a buffer that holds L, D = A L^-T, the rows' norms and A in the order the solve's lanes load them, the factored forms of gi_dense and gi_wave, plain and EQ, start from a forward substitution for y and s = b + D y in place of the set-up sweep; gi_rfact v1.0: qpb_solve_range_factored for n <= 32 and m <= 64, two-sided rows on the same factor buffer in the RG forms of the factored kernels, thresholds from the stored |a_r| bit for bit the range form's, a lower-only row's stored row of D negated before the slacks are formed; kkt_bwd_fact v1.0: qpb_solve_factored_backward for n <= 32 and m <= 64, a shared H and A factored once by the backward kernels' own set-up into a buffer of the backward's own that holds L, 1 / L_kk, D = A L^-T and the sweep's multipliers, the factored forms of kkt_bwd take u from them by the set-up's own operations, outputs bit for bit those of qpb_solve_shared_backward; box_shared v1.0: qpb_solve_box_shared for n <= 128 and qpb_solve_box_shared_backward for n <= 32, one H for a batch of box QPs read from one copy through a run-time QP stride in the SH forms of gi_box, gi_wave's and gi_gram's BOX kernels and kkt_bwd_box, outputs bit for bit those of qpb_solve_box and qpb_solve_box_backward on copies, gH summed over the batch by kkt_bwd_sum at m = 0; box_fact v1.0: qpb_factor_box and qpb_solve_box_factored for n <= 32, the one H of a batch of box QPs factored once by the class's own load and sweep into a buffer that holds L, the rows of L^-T and their squared norms in the order the solve's lanes load them and neither H nor A, the factored forms of gi_box and of gi_wave's BOX kernel start from a forward substitution for y = L^-1 f with e = L^-T y accumulated alongside and the slacks ub + e and -lb - e in place of the set-up sweep, the lower bounds' rows negated as they are loaded; gi_range_box v1.0: qpb_solve_range_box for n <= 32 and mg + n <= 64, two-sided rows beside variable bounds lb <= x <= ub in the BX forms of the RG forms of gi_dense and gi_wave, the identity's rows made in registers where the materialised [G; I] would put them and added as lam e_j in the x recovery, outputs bit for bit those of qpb_solve_range on the materialised problem; kkt_bwd_range_box v1.0: qpb_solve_range_box_backward for n <= 32 and mg + n <= 64, the BX forms of kkt_bwd (plain, shared and with glam) and of kkt_bwd_sum, unit rows made in registers, the gradient of the identity neither computed nor stored, gb routed to the four bound arrays by the lower bits, outputs bit for bit those of qpb_solve_backward_dual on the materialised problem)"; }
