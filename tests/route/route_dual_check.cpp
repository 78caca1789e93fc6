// route_dual_check.cpp -- stand-alone host check of the routes of
// qpb_solve_factored_backward_dual and qpb_solve_box_backward_dual in
// csrc/qpb_route.h (tests/test_route_dual_paths.py builds it with the host
// compiler under ASan + UBSan and runs it).  Including the header compiles its
// static_asserts; the loops below hold the two routes to the calls whose bits
// and buffers they share, over every size, not only at the classes' corners.
#include "qpb_route.h"

#include <cstdio>

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

int main() {
  for (int n = 1; n <= 129; ++n)
    for (int m = 0; m <= 257; ++m) {
      const qpb::Route d = qpb::route_factored_bwd_dual(n, m);
      const qpb::Route f = qpb::route_factored_bwd(n, m), u = qpb::route_bwd_dual(n, m);
      // the buffer is the factored backward's, the bits the unfactored dual call's
      CHECK(d.kernel == f.kernel && d.step == f.step, "n=%d m=%d", n, m);
      CHECK(d.kernel == u.kernel && d.step == u.step, "n=%d m=%d", n, m);
      const bool in = n <= qpb::kFactoredBwdDualMaxN && m <= qpb::kFactoredBwdDualMaxM;
      CHECK((d.step > 0) == in, "n=%d m=%d step=%lld", n, m, d.step);
      // the class decides the buffer's layout: qpb_factor.h goes by the same two limits
      if (in) CHECK((d.kernel == qpb::Kernel::gi_dense) == (n <= 16 && m <= 32), "n=%d m=%d", n, m);
    }
  for (int n = 1; n <= 129; ++n) {
    const qpb::Route d = qpb::route_bwd_box_dual(n);
    const qpb::Route b = qpb::route_bwd_box(n), s = qpb::route_bwd_box_shared(n);
    CHECK(d.kernel == b.kernel && d.step == b.step, "n=%d", n);
    CHECK(d.kernel == s.kernel && d.step == s.step, "n=%d", n);
    CHECK((d.step > 0) == (n <= qpb::kBwdBoxDualMaxN), "n=%d step=%lld", n, d.step);
    if (d.step > 0) CHECK((d.kernel == qpb::Kernel::gi_box) == (n <= 16), "n=%d", n);
  }
  if (failures) {
    std::printf("route_dual_check: %d failures\n", failures);
    return 1;
  }
  std::printf("route_dual_check ok\n");
  return 0;
}
