// route_check.cpp -- stand-alone host check of csrc/qpb_route.h (tests/test_route.py
// builds it with the host compiler under ASan + UBSan and runs it):
//   * the route table against a second statement of it, the if-chains that
//     qpb_solve / qpb_solve_box carried before the table existed;
//   * the chunk walker at step 4 on fake base addresses (nothing is dereferenced).
#include "qpb_route.h"

#include <cstdint>
#include <cstdio>
#include <initializer_list>

static int failures = 0;
#define CHECK(cond, ...)                  \
  do {                                    \
    if (!(cond)) {                        \
      if (failures++ < 20) {              \
        std::printf("FAIL %s: ", #cond);  \
        std::printf(__VA_ARGS__);         \
        std::printf("\n");                \
      }                                   \
    }                                     \
  } while (0)

// ---- the reference: the former dispatch of qpb_api.hip as plain code ---------
static long long ref_chunk_qps(int n, int m, int flags) {
  if (n <= 16 && m <= 32 && !(flags & QPB_FLAG_DIAG_WAVE)) return 1LL << 27;
  if (n <= 32 && m <= 64) return 1LL << 25;
  return 1LL << 21;
}
static qpb::Kernel ref_solve_kernel(int n, int m, int flags) {
  if (n <= 16 && m <= 32 && !(flags & QPB_FLAG_DIAG_WAVE))
    return qpb::Kernel::gi_dense;
  else if (n > 16 && n <= 32 && m <= 64 && (flags & QPB_FLAG_MIXED))
    return qpb::Kernel::gi_mixed;
  else if (n <= 32 && m <= 64)
    return qpb::Kernel::gi_wave;
  else
    return qpb::Kernel::gi_gram;
}
static long long ref_box_step(int n) { return n <= 16 ? 1LL << 27 : 1LL << 25; }
static qpb::Kernel ref_box_kernel(int n) {
  return n <= 16 ? qpb::Kernel::gi_box : n <= 32 ? qpb::Kernel::gi_wave_box : qpb::Kernel::gi_gram_box;
}

static void check_routes() {
  const int flag_sets[4] = {0, QPB_FLAG_MIXED, QPB_FLAG_DIAG_WAVE, QPB_FLAG_MIXED | QPB_FLAG_DIAG_WAVE};
  for (int flags : flag_sets)
    for (int n = 1; n <= 129; ++n)
      for (int m = 0; m <= 257; ++m) {
        const qpb::Route r = qpb::route(n, m, flags, false);
        CHECK(r.kernel == ref_solve_kernel(n, m, flags), "dense n=%d m=%d flags=%d: kernel %d", n, m, flags,
              (int)r.kernel);
        CHECK(r.step == ref_chunk_qps(n, m, flags), "dense n=%d m=%d flags=%d: step %lld", n, m, flags, r.step);
        CHECK(r.step == qpb::step_of(r.kernel), "dense n=%d m=%d flags=%d: step is not its kernel's", n, m, flags);
        const qpb::Route bx = qpb::route(n, m, flags, true);
        CHECK(bx.kernel == ref_box_kernel(n), "box n=%d m=%d flags=%d: kernel %d", n, m, flags, (int)bx.kernel);
        CHECK(bx.step == ref_box_step(n), "box n=%d m=%d flags=%d: step %lld", n, m, flags, bx.step);
      }
}

// ---- the chunk walker --------------------------------------------------------
template <class T>
static T *fake(std::uintptr_t addr) {
  return reinterpret_cast<T *>(addr);
}
template <class T>
static bool at_offset(const T *got, const T *base, long long elements) {
  if (!base) return got == nullptr;
  return reinterpret_cast<std::uintptr_t>(got) ==
         reinterpret_cast<std::uintptr_t>(base) + (std::uintptr_t)elements * sizeof(T);
}

// every array of qpb_solve, qpb_solve_box and qpb_ref_solve in one walk
static void check_walk(long long batch, long long step, int n, int m, bool with_optional) {
  const long long w = (m + 31) / 32;
  const double *H = fake<const double>(0x10000000), *f = fake<const double>(0x20000000);
  const double *A = m ? fake<const double>(0x30000000) : nullptr, *b = m ? fake<const double>(0x40000000) : nullptr;
  const double *lb = with_optional ? fake<const double>(0x50000000) : nullptr;
  const double *ub = with_optional ? fake<const double>(0x60000000) : nullptr;
  const double *x0 = with_optional ? fake<const double>(0x70000000) : nullptr;
  double *x = fake<double>(0x80000000), *lam = m ? fake<double>(0x90000000) : nullptr;
  std::uint32_t *active = m ? fake<std::uint32_t>(0xA0000000) : nullptr;
  std::int32_t *status = fake<std::int32_t>(0xB0000000);
  std::int32_t *iters = with_optional ? fake<std::int32_t>(0xC0000000) : nullptr;

  long long k0 = 0, calls = 0;
  const int rc = qpb::for_each_chunk(
      batch, step,
      [&](long long count, const double *Hc, const double *fc, const double *Ac, const double *bc, const double *lbc,
          const double *ubc, const double *x0c, double *xc, double *lc, std::uint32_t *ac, std::int32_t *sc,
          std::int32_t *ic) {
        CHECK(count >= 1 && count <= step, "batch=%lld: chunk of %lld at k0=%lld", batch, count, k0);
        CHECK(at_offset(Hc, H, k0 * n * n) && at_offset(fc, f, k0 * n) && at_offset(xc, x, k0 * n),
              "batch=%lld k0=%lld: H, f or x", batch, k0);
        CHECK(at_offset(Ac, A, k0 * m * n) && at_offset(bc, b, k0 * m) && at_offset(lc, lam, k0 * m),
              "batch=%lld k0=%lld m=%d: A, b or lam", batch, k0, m);
        CHECK(at_offset(ac, active, k0 * w), "batch=%lld k0=%lld m=%d: active", batch, k0, m);
        CHECK(at_offset(lbc, lb, k0 * n) && at_offset(ubc, ub, k0 * n) && at_offset(x0c, x0, k0 * n),
              "batch=%lld k0=%lld: lb, ub or x0", batch, k0);
        CHECK(at_offset(sc, status, k0) && at_offset(ic, iters, k0), "batch=%lld k0=%lld: status or iters", batch, k0);
        if (m == 0) CHECK(!Ac && !bc && !lc && !ac, "batch=%lld k0=%lld: a NULL m = 0 array moved", batch, k0);
        if (!with_optional) CHECK(!lbc && !ubc && !x0c && !ic, "batch=%lld k0=%lld: a NULL optional moved", batch, k0);
        k0 += count;
        ++calls;
        return 0;
      },
      qpb::required(H, (long long)n * n), qpb::required(f, n), qpb::optional(A, (long long)m * n),
      qpb::optional(b, m), qpb::optional(lb, n), qpb::optional(ub, n), qpb::optional(x0, n), qpb::required(x, n),
      qpb::optional(lam, m), qpb::optional(active, w), qpb::required(status, 1), qpb::optional(iters, 1));
  CHECK(rc == 0, "batch=%lld: rc %d", batch, rc);
  CHECK(k0 == batch, "batch=%lld: the chunks sum to %lld", batch, k0);
  CHECK(calls == (batch + step - 1) / step, "batch=%lld: %lld calls", batch, calls);
  if (batch == 0) CHECK(calls == 0, "batch 0 made %lld calls", calls);
}

// a nonzero return ends the walk and is handed back
static void check_walk_stops() {
  int calls = 0;
  const int rc = qpb::for_each_chunk(
      11, 4, [&](long long, std::int32_t *) { return ++calls == 2 ? -7 : 0; }, qpb::optional<std::int32_t>(nullptr, 1));
  CHECK(rc == -7 && calls == 2, "rc=%d after %d calls", rc, calls);
}

int main() {
  check_routes();
  const long long batches[5] = {0, 1, 4, 5, 11};
  for (long long batch : batches)
    for (int m : {0, 33})
      for (bool with_optional : {false, true}) check_walk(batch, 4, 5, m, with_optional);
  check_walk_stops();
  if (failures) {
    std::printf("route_check: %d failures\n", failures);
    return 1;
  }
  std::printf("route_check ok\n");
  return 0;
}
